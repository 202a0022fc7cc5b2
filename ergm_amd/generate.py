"""Response generation with a KV cache: ``nucleus_sampling`` of the reference trainer
(src/main.py:253-282) without its full-sequence recompute per token.

The reference re-runs the whole model on the growing sequence for every new token (and cannot run as
written: it passes no ``caption_ids``).  Here the prompt is encoded once (prefill, the
same kernels as training: causal attention over the prompt, cross-attention over the caption
embeddings), the per-layer self-attention keys/values are kept in a cache in HBM, the caption K/V of
every layer are computed once, and each new token costs one position through the stack: a row of
every GEMM, attention of one query over the cached keys (``ergm_attn_fwd`` with Sq = 1, non-causal —
all cached positions precede it), and the tied LM head for that row only.

The captions stay fixed while the response grows (the reference would need caption length == the
current sequence length, src/model.py:461, which generation cannot satisfy); the prompt's visual /
audio vectors enter at positions 0 and 1 as in training.  Batch 1, like the reference's test loop
(src/main.py:305-313).  Every op is a C-ABI kernel call; the sampling itself (softmax, sort, top-p
cut, multinomial over one [V] row) uses the reference's own torch calls on the device.

``BatchedGenerator`` is the same computation for a batch of sequences of different lengths: one padded prefill,
then per token one row per sequence through every GEMM, ``ergm_attn_decode`` over each sequence's own cache
length (the lengths stay on the device; the kernel appends the new K/V row itself), and ``ergm_topp_sample``
for the whole batch without a sort or a host round trip.  ``KVCacheGenerator`` is its single-sequence yardstick.

``ContinuousGenerator`` serves a queue of requests on a fixed set of cache slots (in-flight batching): every step runs
over all slots, a slot finishes on the device at eos or at the bound recorded when it was filled, and the host, looking
once in 8 steps, retires the finished requests and prefills waiting ones into the free slots.  ``SlotScheduler`` is its
host-only policy.  With ``num_beams`` the same generator serves beam-search requests, each in a group of slots
(``BeamScheduler``: the same policy over groups).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, replace
from typing import List, Optional

import torch
import torch.nn.functional as F

from . import _lib as L
from . import ops


class KVCacheGenerator:
    def __init__(self, model, max_len: int = 1024):
        cfg = model.config
        if max_len > cfg.n_positions:
            raise ValueError(f"max_len {max_len} > n_positions {cfg.n_positions}")
        self.m, self.cfg = model, cfg
        self.E, self.H, self.L, self.F = cfg.n_embd, cfg.n_head, cfg.n_layer, cfg.inner
        self.max_len = max_len
        dev = model.flat.device
        self.dev = dev
        # per layer: self-attention K | V of every position so far, [max_len, 2E] bf16
        self.kv = [torch.empty(max_len, 2 * self.E, dtype=torch.bfloat16, device=dev) for _ in range(self.L)]
        self.xkv: List[torch.Tensor] = []
        self.n = 0

    # parameter views: fp32 master (biases, LayerNorm) and the bf16 shadow the GEMMs read
    def _f(self, name):
        return self.m.view(name)

    def _b(self, name):
        return self.m.view(name, self.m.flat_b16)

    def _ln(self, x, name):
        y, _, _ = ops.layernorm_fwd(x, self._f(name + ".weight"), self._f(name + ".bias"), self.cfg.layer_norm_epsilon)
        return y

    def _block(self, l: int, h: torch.Tensor, p0: int) -> None:
        """Rows h [n, E] (positions p0 .. p0+n-1) through block l, in place."""
        E, H, F_ = self.E, self.H, self.F
        n = h.shape[0]
        p = f"transformer.h.{l}."
        x = self._ln(h, p + "ln_1")
        qkv = ops.gemm(x, self._b(p + "attn.c_attn.weight"), n, 3 * E, E, L.MK, L.KN, out_dtype=torch.bfloat16,
                       epilogue=L.EPI_BIAS, bias=self._f(p + "attn.c_attn.bias"))
        cache = self.kv[l]
        cache[p0:p0 + n].copy_(qkv[:, E:])
        k, v = cache[:, :E], cache[:, E:]
        if p0 == 0:   # prefill: causal over the prompt
            a, _ = ops.attn_fwd(qkv[:, :E], k, v, 1, H, n, n, True)
        else:         # one new position: every cached key precedes it
            a, _ = ops.attn_fwd(qkv[:, :E], k, v, 1, H, n, p0 + n, False)
        ops.gemm(a, self._b(p + "attn.c_proj.weight"), n, E, E, L.MK, L.KN, out=h, epilogue=L.EPI_BIAS_RESID,
                 bias=self._f(p + "attn.c_proj.bias"), aux=h)
        x = self._ln(h, p + "ln_cross_attn")
        q = ops.gemm(x, self._b(p + "crossattention.q_attn.weight"), n, E, E, L.MK, L.KN, out_dtype=torch.bfloat16,
                     epilogue=L.EPI_BIAS, bias=self._f(p + "crossattention.q_attn.bias"))
        xkv = self.xkv[l]
        a, _ = ops.attn_fwd(q, xkv[:, :E], xkv[:, E:], 1, H, n, xkv.shape[0], False)
        ops.gemm(a, self._b(p + "crossattention.c_proj.weight"), n, E, E, L.MK, L.KN, out=h,
                 epilogue=L.EPI_BIAS_RESID, bias=self._f(p + "crossattention.c_proj.bias"), aux=h)
        x = self._ln(h, p + "ln_2")
        pre = torch.empty(n, F_, dtype=torch.bfloat16, device=self.dev)
        act = ops.gemm(x, self._b(p + "mlp.c_fc.weight"), n, F_, E, L.MK, L.KN, out_dtype=torch.bfloat16,
                       epilogue=L.EPI_BIAS_GELU, bias=self._f(p + "mlp.c_fc.bias"), aux_out=pre)
        ops.gemm(act, self._b(p + "mlp.c_proj.weight"), n, E, F_, L.MK, L.KN, out=h, epilogue=L.EPI_BIAS_RESID,
                 bias=self._f(p + "mlp.c_proj.bias"), aux=h)

    def _head(self, h_last: torch.Tensor) -> torch.Tensor:
        x = self._ln(h_last, "transformer.ln_f")
        lay = self.m.layout
        logits = ops.gemm(x, self._b("__wte_pad"), 1, lay.vocab_pad, self.E, L.MK, L.NK, out_dtype=torch.float32)
        return logits[0, :lay.vocab]

    @torch.no_grad()
    def prefill(self, input_ids, token_type_ids, caption_ids, imgs=None, auds=None) -> torch.Tensor:
        """Encode the prompt [1, S0]; returns the next-token logits [V] (fp32)."""
        self.m.refresh_bf16()
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("generation runs one sequence at a time (batch 1)")
        S0 = input_ids.shape[1]
        if S0 >= self.max_len:
            raise ValueError("prompt longer than max_len")
        wte, wpe = self._f("__wte_pad"), self._f("transformer.wpe.weight")
        Fd = self.m.layout.Fd
        vis = None if imgs is None else imgs.float().reshape(1, -1, Fd)[:, 0]
        aud = None if auds is None else auds.float().reshape(1, Fd)
        if vis is not None and Fd != self.E:  # config 5: the build-side projections (Conv1D), MFMA GEMMs
            vis, aud = (ops.gemm(x.to(torch.bfloat16), self._b(f"transformer.{m}.weight"), 1, self.E, Fd, L.MK, L.KN,
                                 out_dtype=torch.float32, epilogue=L.EPI_BIAS, bias=self._f(f"transformer.{m}.bias"))
                        for x, m in ((vis, "visual_proj"), (aud, "audio_proj")))
        h, _ = ops.embed_fwd(input_ids, token_type_ids, input_ids, wte, wpe, vis, aud)
        _, cap = ops.embed_fwd(caption_ids, None, caption_ids, wte, wpe)
        Sc = caption_ids.shape[1]
        self.xkv = [ops.gemm(cap, self._b(f"transformer.h.{l}.crossattention.c_attn.weight"), Sc, 2 * self.E,
                             self.E, L.MK, L.KN, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS,
                             bias=self._f(f"transformer.h.{l}.crossattention.c_attn.bias")) for l in range(self.L)]
        for l in range(self.L):
            self._block(l, h, 0)
        self.n = S0
        return self._head(h[S0 - 1:S0])

    @torch.no_grad()
    def step(self, token: torch.Tensor, token_type: torch.Tensor) -> torch.Tensor:
        """Append one token (ids [1, 1]) at position n; returns the logits [V] for position n + 1."""
        if self.n >= self.max_len:
            raise ValueError("KV cache full")
        wte, wpe = self._f("__wte_pad"), self._f("transformer.wpe.weight")
        h, _ = ops.embed_fwd(token, token_type, token, wte, wpe[self.n:])  # wpe row n is position 0 of the view
        for l in range(self.L):
            self._block(l, h, self.n)
        self.n += 1
        return self._head(h)

    @torch.no_grad()
    def nucleus_sampling(self, input_ids, token_type_ids, caption_ids, top_p: float, eos_id: int, sp2_id: int,
                         imgs=None, auds=None, generator: Optional[torch.Generator] = None) -> List[int]:
        """src/main.py:253-282: sample until eos or max_len, the response typed as speaker 2."""
        logits = self.prefill(input_ids, token_type_ids, caption_ids, imgs, auds)
        out: List[int] = []
        tt = torch.full((1, 1), sp2_id, dtype=torch.long, device=self.dev)
        for pos in range(input_ids.shape[1], self.max_len):
            probs = F.softmax(logits.unsqueeze(0), dim=-1)
            sorted_probs, sorted_idxs = torch.sort(probs, descending=True)
            cum = torch.cumsum(sorted_probs, dim=-1)
            remove = cum > top_p
            remove[:, 1:] = remove[:, :-1].clone()
            remove[:, 0] = False
            sorted_probs[remove] = 0.0
            sorted_probs /= torch.sum(sorted_probs, dim=-1, keepdim=True)
            probs = torch.zeros_like(probs).scatter_(-1, sorted_idxs, sorted_probs)
            idx = torch.multinomial(probs, 1, generator=generator)
            tok = int(idx.item())
            out.append(tok)
            if tok == eos_id or pos + 1 >= self.max_len:
                break
            logits = self.step(idx.view(1, 1), tt)
        return out


class BatchedGenerator:
    """KV-cache generation for up to ``max_batch`` sequences of different lengths at once.

    ``prefill`` encodes the right-padded prompts with the training kernels (causal attention hides the padding
    from the real rows; the padded rows' K/V land in cache rows >= lens[b], which decode overwrites before it
    reads them); ``step`` appends one token per sequence; ``generate`` is nucleus sampling of the whole batch;
    ``beam_search`` (``beam_prefill``, ``beam_round``) is beam search with ``num_beams`` cache rows per prompt, the
    ranking and the cache reordering on the device (ergm_beam_select, ergm_beam_gather).

    ``engine``: "python" (default) drives every kernel of a step from Python; "native" hands the step and the
    sampling loop to the library's decode executor (``ergm_decode_*``), which enqueues the same kernels with the same
    arguments (bitwise the Python path); "fused" is the executor on ``ergm_linear_rows``, one launch per LayerNorm +
    GEMM pair.  The prefill is the Python path in every case and ends by binding its caches to the executor."""

    ENGINES = {"python": None, "native": 0, "fused": 1}   # the executor's engine numbers

    def __init__(self, model, max_batch: int, max_len: int = 1024, engine: str = "python"):
        if engine not in self.ENGINES:
            raise ValueError(f"engine {engine!r} is not one of {sorted(self.ENGINES)}")
        self.engine = engine
        self._plan = self._plan_ws = self._plan_params = None
        self._cap_max = 0
        cfg = model.config
        if max_len > cfg.n_positions:
            raise ValueError(f"max_len {max_len} > n_positions {cfg.n_positions}")
        if max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        self.m, self.cfg = model, cfg
        self.E, self.H, self.L, self.F = cfg.n_embd, cfg.n_head, cfg.n_layer, cfg.inner
        self.max_batch, self.max_len = max_batch, max_len
        dev = model.flat.device
        self.dev = dev
        # per layer: self-attention K | V of every sequence, [max_batch, max_len, 2E] bf16
        self.kv = [torch.empty(max_batch, max_len, 2 * self.E, dtype=torch.bfloat16, device=dev) for _ in range(self.L)]
        self.xkv: List[torch.Tensor] = []   # per layer: caption K | V, [B, Sc_max, 2E]
        self.lens = torch.zeros(max_batch, dtype=torch.int32, device=dev)
        self.cap_lens = torch.zeros(max_batch, dtype=torch.int32, device=dev)
        self.finished = torch.zeros(max_batch, dtype=torch.uint8, device=dev)
        self.B = 0
        self.n_max = 0   # host bound on max(lens): the longest prompt plus the steps taken
        self._ws = self._logits = None   # decode-attention workspace; the last logits [B, vocab_pad]

    # parameter views and LayerNorm as the single-sequence generator has them
    _f, _b, _ln = KVCacheGenerator._f, KVCacheGenerator._b, KVCacheGenerator._ln

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _drop_plan(self) -> None:
        plan, self._plan = self._plan, None
        if plan is not None:
            L.load().ergm_decode_destroy(plan)

    def __del__(self):
        try:
            self._drop_plan()
        except Exception:
            pass

    def _new_plan(self, cap_max: int, capkv: bool):
        """Create the executor plan (``_plan``, with its workspace and parameter block kept alive beside it) for
        captions of up to cap_max rows, on this generator's engine; ``capkv`` passes the caption K/V weights, which
        only an admission reads.  Returns the dimensions it was created with."""
        lib, lay = L.load(), self.m.layout
        dims = L.DecodeDims(vocab=lay.vocab, vocab_pad=lay.vocab_pad, n_embd=self.E, n_layer=self.L, n_head=self.H,
                            n_inner=self.F, n_positions=self.cfg.n_positions, max_batch=self.max_batch,
                            max_len=self.max_len, cap_max=cap_max, eps=self.cfg.layer_norm_epsilon)
        prm = L.ModelParams()
        prm.wte, prm.wte_b = self._f("__wte_pad").data_ptr(), self._b("__wte_pad").data_ptr()
        prm.wpe = self._f("transformer.wpe.weight").data_ptr()
        prm.ln_f_w = self._f("transformer.ln_f.weight").data_ptr()
        prm.ln_f_b = self._f("transformer.ln_f.bias").data_ptr()
        if capkv:
            prm.capkv_w_b, prm.capkv_b = self._b("__capkv_w").data_ptr(), self._f("__capkv_b").data_ptr()
        prm.layer_f32 = self.m.flat.data_ptr() + 4 * lay.layer_base[0]
        prm.layer_b16 = self.m.flat_b16.data_ptr() + 2 * lay.layer_base[0]
        prm.layer_stride = lay.layer_stride
        for i, o in enumerate(lay.layer_off):
            prm.layer_off[i] = o
        need = lib.ergm_decode_workspace_size(C.byref(dims))
        if need == 0:
            raise ValueError("the decode executor does not support this model's dimensions")
        self._plan_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        self._plan_params = prm
        plan = C.c_void_p()
        L.check(lib.ergm_decode_create(C.byref(dims), C.byref(prm), C.c_void_p(self._plan_ws.data_ptr()), need,
                                       C.byref(plan)), "ergm_decode_create")
        self._plan = plan
        L.call("ergm_decode_set_engine", plan, self.ENGINES[self.engine])
        return dims

    def _bind_plan(self, Sc: int) -> None:
        """(Re)create the executor plan when the captions outgrow it, then bind the state the prefill left."""
        if self._plan is None or Sc > self._cap_max:
            self._drop_plan()
            self._cap_max = max(Sc, self.max_len)
            self._new_plan(self._cap_max, capkv=False)
        ptrs = C.c_void_p * self.L
        kv = ptrs(*[t.data_ptr() for t in self.kv])
        xkv = ptrs(*[t.data_ptr() for t in self.xkv])
        L.call("ergm_decode_bind", self._plan, self.B, self.n_max, kv, xkv, Sc, C.c_void_p(self.lens.data_ptr()),
               C.c_void_p(self.cap_lens.data_ptr()), C.c_void_p(self.finished.data_ptr()),
               C.c_void_p(self._logits.data_ptr()))

    def _gemm(self, x, name, n, N, K, **kw):
        return ops.gemm(x, self._b(name + ".weight"), n, N, K, L.MK, L.KN, bias=self._f(name + ".bias"), **kw)

    def _mlp(self, p: str, h: torch.Tensor, n: int) -> None:
        x = self._ln(h, p + "ln_2")
        pre = torch.empty(n, self.F, dtype=torch.bfloat16, device=self.dev)
        act = self._gemm(x, p + "mlp.c_fc", n, self.F, self.E, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS_GELU,
                         aux_out=pre)
        self._gemm(act, p + "mlp.c_proj", n, self.E, self.F, out=h, epilogue=L.EPI_BIAS_RESID, aux=h)

    def _block(self, l: int, h: torch.Tensor, n: int, self_attn, cross_attn) -> None:
        """The n rows of h [n, E] through block l, in place: the one place the "python" engine of the batch generators
        spells the block out.  The caller supplies the two stages that differ between prefill, admission, extension
        and step: ``self_attn(l, qkv)`` takes the rows' q | k | v [n, 3E], writes their K | V to the cache and returns
        the attention output [n, E] bf16; ``cross_attn(l, q)`` takes the cross query [n, E] and returns the attention
        over the captions."""
        E = self.E
        p = f"transformer.h.{l}."
        x = self._ln(h, p + "ln_1")
        qkv = self._gemm(x, p + "attn.c_attn", n, 3 * E, E, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS)
        a = self_attn(l, qkv)
        self._gemm(a, p + "attn.c_proj", n, E, E, out=h, epilogue=L.EPI_BIAS_RESID, aux=h)
        x = self._ln(h, p + "ln_cross_attn")
        q = self._gemm(x, p + "crossattention.q_attn", n, E, E, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS)
        a = cross_attn(l, q)
        self._gemm(a, p + "crossattention.c_proj", n, E, E, out=h, epilogue=L.EPI_BIAS_RESID, aux=h)
        self._mlp(p, h, n)

    def _step_rows(self, tokens, token_types, lens, cap_lens, kv, xkv) -> torch.Tensor:
        """The "python" engine's step: one token per sequence at position lens[b], through every block over the
        per-layer caches kv [B, max_len, 2E] (the new K | V row appended) and xkv [B, Sc, 2E].  Returns the logits
        [B, vocab_pad]; the caller updates its own state."""
        E, ws = self.E, self._ws
        h = ops.embed_rows(tokens, token_types, lens, self._f("__wte_pad"), self._f("transformer.wpe.weight"))

        def self_attn(l, qkv):
            return ops.attn_decode(qkv, kv[l][:, :, :E], kv[l][:, :, E:], lens, True, ws=ws)

        def cross_attn(l, q):
            return ops.attn_decode(q, xkv[l][:, :, :E], xkv[l][:, :, E:], cap_lens, False, ws=ws)

        for l in range(self.L):
            self._block(l, h, h.shape[0], self_attn, cross_attn)
        return self._head(h)

    def _features(self, prompts):
        """(vis, aud) f32 [n_seq, E], projected when the features are wider or narrower than E (config 5), zeros for
        the sequences without features, and the per-sequence flags; (None, None, flags) when no prompt has features."""
        has = [p[3] is not None for p in prompts]
        if not any(has):
            return None, None, has
        n, Fd, dev = len(prompts), self.m.layout.Fd, self.dev
        vis = torch.zeros(n, Fd, dtype=torch.float32, device=dev)
        aud = torch.zeros(n, Fd, dtype=torch.float32, device=dev)
        for b, p in enumerate(prompts):
            if has[b]:
                vis[b] = p[3].float().reshape(-1, Fd)[0]
                aud[b] = p[4].float().reshape(Fd)
        if Fd != self.E:
            vis, aud = (self._gemm(x.to(torch.bfloat16), f"transformer.{m}", n, self.E, Fd, out_dtype=torch.float32,
                                   epilogue=L.EPI_BIAS) for x, m in ((vis, "visual_proj"), (aud, "audio_proj")))
        return vis, aud, has

    def _head(self, h_last: torch.Tensor) -> torch.Tensor:
        """Rows [B, E] -> logits [B, vocab_pad] f32 (the first ``vocab`` columns count)."""
        x = self._ln(h_last, "transformer.ln_f")
        lay = self.m.layout
        return ops.gemm(x, self._b("__wte_pad"), x.shape[0], lay.vocab_pad, self.E, L.MK, L.NK, out_dtype=torch.float32)

    @torch.no_grad()
    def prefill(self, prompts) -> torch.Tensor:
        """prompts: a list of (input_ids, token_type_ids, caption_ids, imgs, auds) per sequence (1-D or [1, S] id
        tensors of any lengths; imgs / auds may be None).  Returns the next-token logits [B, V] (fp32)."""
        return self._prefill(prompts, 1)

    def _prefill(self, prompts, W: int) -> torch.Tensor:
        """The prefill of ``prompts`` into every W-th row: prompt g's cache rows, length and logits land in row g·W,
        its caption K | V and caption length in all W rows of its group, and the other rows get length 0 and zero
        logits.  W = 1 is ``prefill``; W > 1 is the state ``beam_prefill`` starts from."""
        self.m.refresh_bf16()
        B = len(prompts)
        R = B * W
        if not 1 <= R <= self.max_batch:
            raise ValueError(f"{B} prompts" + (f" of {W} beams" if W > 1 else "") + f" for max_batch {self.max_batch}")
        E, H, dev = self.E, self.H, self.dev
        ids_l = [p[0].reshape(-1) for p in prompts]
        cap_l = [p[2].reshape(-1) for p in prompts]
        lens = [int(t.numel()) for t in ids_l]
        clens = [int(t.numel()) for t in cap_l]
        if min(lens) < 1 or min(clens) < 1:
            raise ValueError("empty prompt or caption")
        S, Sc = max(lens), max(clens)
        if S >= self.max_len:
            raise ValueError("prompt longer than max_len")
        ids = torch.zeros(B, S, dtype=torch.long, device=dev)
        tt = torch.zeros(B, S, dtype=torch.long, device=dev)
        cap_ids = torch.zeros(B, Sc, dtype=torch.long, device=dev)
        for b, p in enumerate(prompts):
            ids[b, :lens[b]] = ids_l[b]
            tt[b, :lens[b]] = p[1].reshape(-1)
            cap_ids[b, :clens[b]] = cap_l[b]
        wte, wpe = self._f("__wte_pad"), self._f("transformer.wpe.weight")
        vis, aud, has = self._features(prompts)   # sequences without features add zeros
        if vis is not None and self.m.layout.Fd != E:   # config 5: nothing for the rows without features
            keep = torch.tensor(has, device=dev).unsqueeze(1)
            vis, aud = vis * keep, aud * keep
        h, _ = ops.embed_fwd(ids, tt, ids, wte, wpe, vis, aud)
        _, cap = ops.embed_fwd(cap_ids, None, cap_ids, wte, wpe)
        xkv = [self._gemm(cap, f"transformer.h.{l}.crossattention.c_attn", B * Sc, 2 * E, E,
                          out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS).view(B, Sc, 2 * E) for l in range(self.L)]
        self.xkv = xkv if W == 1 else [t.repeat_interleave(W, 0) for t in xkv]
        n = B * S

        def self_attn(l, qkv):
            self.kv[l][:R:W, :S].copy_(qkv[:, E:].view(B, S, 2 * E))
            return ops.attn_fwd(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], B, H, S, S, True)[0]

        def cross_attn(l, q):
            a = torch.empty(n, E, dtype=torch.bfloat16, device=dev)
            for b in range(B):   # each sequence over its own caption rows: padded caption rows are never attended
                kvb = xkv[l][b, :clens[b]]
                ops.attn_fwd(q[b * S:(b + 1) * S], kvb[:, :E], kvb[:, E:], 1, H, S, clens[b], False,
                             o=a[b * S:(b + 1) * S])
            return a

        for l in range(self.L):
            self._block(l, h, n, self_attn, cross_attn)
        self.B, self.n_max = R, S
        if W > 1:
            self.lens[:R] = 0
        self.lens[:R:W] = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.cap_lens[:R] = torch.tensor(clens, dtype=torch.int32, device=dev).repeat_interleave(W)
        self.finished.zero_()
        self._ws = ops.attn_decode_workspace(R, H, max(self.max_len, Sc), dev)
        last = torch.tensor([b * S + lens[b] - 1 for b in range(B)], device=dev)
        self._logits = self._head(h.index_select(0, last))
        if W > 1:
            rows = torch.zeros(R, self._logits.shape[1], dtype=torch.float32, device=dev)
            rows[::W] = self._logits
            self._logits = rows
        if self.engine != "python":
            self._bind_plan(Sc)
        return self._logits[:, :self.m.layout.vocab]

    @torch.no_grad()
    def step(self, tokens: torch.Tensor, token_types: torch.Tensor) -> torch.Tensor:
        """Append one token per sequence (ids [B], int64) at its own position lens[b]; returns the logits [B, V]
        for the next position.  The lengths of the sequences not yet finished advance by one."""
        if self.B == 0:
            raise ValueError("step before prefill")
        if self.n_max >= self.max_len:
            raise ValueError("KV cache full")
        B = self.B
        tokens, token_types = tokens.reshape(-1), token_types.reshape(-1)
        if tokens.numel() != B or token_types.numel() != B:
            raise ValueError(f"step takes one token and one token type per sequence ({B})")
        if self.engine != "python":   # the executor's step, into the logits buffer the prefill bound
            if tokens.dtype != torch.int64 or token_types.dtype != torch.int64 or not (tokens.is_cuda and token_types.is_cuda):
                raise ValueError("step takes int64 GPU tensors")
            tokens, token_types = tokens.contiguous(), token_types.contiguous()
            L.call("ergm_decode_step", self._plan, C.c_void_p(tokens.data_ptr()), C.c_void_p(token_types.data_ptr()),
                   self._stream())
            self.n_max += 1
            return self._logits[:, :self.m.layout.vocab]
        lens = self.lens[:B]
        self._logits = self._step_rows(tokens, token_types, lens, self.cap_lens[:B], [t[:B] for t in self.kv], self.xkv)
        lens.add_((self.finished[:B] == 0).to(torch.int32))
        self.n_max += 1
        return self._logits[:, :self.m.layout.vocab]

    @torch.no_grad()
    def generate(self, prompts, top_p: float, eos_id: int, sp2_id: int, seed: int = 0,
                 max_new_tokens: Optional[int] = None) -> List[List[int]]:
        """src/main.py:253-282 for the whole batch: sample every sequence until its eos or the bound, the responses
        typed as speaker 2.  Returns one token list per prompt, each ending at its first ``eos_id`` (included) or at
        ``max_new_tokens``.  The draw of step i for row b is ergm_topp_sample(seed, step=i): seeded runs repeat."""
        bound = self.max_len - max(int(p[0].numel()) for p in prompts)
        if max_new_tokens is None:
            max_new_tokens = bound
        if max_new_tokens < 1 or max_new_tokens > bound:
            raise ValueError(f"max_new_tokens {max_new_tokens} outside [1, {bound}] (max_len - the longest prompt)")
        self.prefill(prompts)
        B, V = self.B, self.m.layout.vocab
        out = torch.empty(max_new_tokens, B, dtype=torch.int64, device=self.dev)
        tt = torch.full((B,), sp2_id, dtype=torch.int64, device=self.dev)
        fin = self.finished[:B]
        done = 0
        if self.engine != "python":
            while True:   # the executor samples and steps 8 tokens per call; the host looks in between, as below
                n = min(8, max_new_tokens - done)
                L.call("ergm_decode_run", self._plan, done, n, float(top_p), seed & (2 ** 64 - 1), eos_id, sp2_id,
                       C.c_void_p(out.data_ptr()), self._stream())
                self.n_max += n - (1 if done == 0 else 0)
                done += n
                if done == max_new_tokens or bool(fin.all()):
                    break
            rows = out[:done].t().cpu().tolist()
            return [r[:r.index(eos_id) + 1] if eos_id in r else r for r in rows]
        for i in range(max_new_tokens):
            ops.topp_sample(self._logits, V, top_p, seed, i, eos_id, finished=fin, tokens=out[i])
            done = i + 1
            if done == max_new_tokens or (done % 8 == 0 and bool(fin.all())):  # the host looks once in 8 steps
                break
            self.step(out[i], tt)
        rows = out[:done].t().cpu().tolist()
        return [r[:r.index(eos_id) + 1] if eos_id in r else r for r in rows]

    # ---- beam search ---------------------------------------------------------------------------------------
    def _beam_check(self, n_prompts: int, num_beams: int) -> None:
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= 8:
            raise ValueError(f"num_beams {num_beams!r} outside [1, 8]")
        if num_beams > self.m.layout.vocab:
            raise ValueError(f"num_beams {num_beams} > the vocabulary")
        if not 1 <= n_prompts * num_beams <= self.max_batch:
            raise ValueError(f"{n_prompts} prompts of {num_beams} beams for max_batch {self.max_batch}")

    @torch.no_grad()
    def beam_prefill(self, prompts, num_beams: int, eos_id: Optional[int] = None, sp2_id: Optional[int] = None,
                     no_repeat_ngram_size: int = 0, no_repeat_scope: str = "sequence", bad_words_ids=()):
        """The state round 0 of a beam search starts from (ergm_hip.h, ergm_decode_run_beams): prompt g in row
        g·num_beams alone (cache rows, length, logits), its caption K | V in all rows of its group, ``beam_scores``
        [0, -inf, ...] per group, nothing finished.  ``eos_id`` / ``sp2_id`` are kept for ``beam_round``.  Returns the
        prompts' next-token logits [G, V].

        ``no_repeat_ngram_size`` / ``no_repeat_scope`` / ``bad_words_ids`` (``SamplingParams`` has their meaning; one
        setting for all prompts) make every round ban before it selects (ergm_hip.h, "Logit rules"): the prompt goes
        into the token history of row g·num_beams here, round 0's fan-out copies it to the group's other rows, and
        "turn" counts the generated part only.  A candidate's log-probability is then normalised over the tokens its
        beam may still take, where Hugging Face masks after the log-softmax."""
        self._beam_check(len(prompts), num_beams)
        bad = check_rules(no_repeat_ngram_size, no_repeat_scope, bad_words_ids)
        ruled = no_repeat_ngram_size > 0 or bool(bad)
        if ruled and self.max_len > 1024:
            raise ValueError(f"logit rules need max_len <= 1024 (it is {self.max_len})")
        W = num_beams
        self._prefill(prompts, W)
        R = self.B
        self._beam_rules = None
        if ruled:   # one copy to the device: the prompts' rows of the history, start | ngram | the pool row per row
            pool = pack_bad_words(bad, sum(len(w) + 1 for w in bad) + 1)
            rows = []
            for p in prompts:
                ids = [int(t) for t in p[0].reshape(-1).tolist()]
                vals = [len(ids) if no_repeat_scope == "turn" else 0, no_repeat_ngram_size, *pool]
                rows.append(vals + ids + [0] * (self.max_len - len(ids)))
                rows += [vals + [0] * self.max_len] * (W - 1)
            m = torch.tensor(rows, dtype=torch.int32).to(self.dev)
            k = 2 + len(pool)
            self._beam_hist = m[:, k:].contiguous()
            self._beam_rule_vals = (m[:, 0].contiguous(), m[:, 1].contiguous(), m[:, 2:k].contiguous())
            self._beam_rules = ops.rules_desc(self._beam_hist, *self._beam_rule_vals)
        if self.engine != "python":
            L.call("ergm_decode_set_rules", self._plan, None if self._beam_rules is None else C.byref(self._beam_rules))
        self.beam_W, self._beam_ids = W, (eos_id, sp2_id)
        self.beam_scores = torch.full((R,), -math.inf, dtype=torch.float32, device=self.dev)
        self.beam_scores[::W] = 0.0
        need = L.load().ergm_beam_select_workspace_size(R, W)
        self._beam_ws = torch.empty(max(need, 8), dtype=torch.uint8, device=self.dev)
        return self._logits[::W, :self.m.layout.vocab]

    @torch.no_grad()
    def beam_round(self, n: int, eos_id: Optional[int] = None, sp2_id: Optional[int] = None):
        """n rounds of select, gather, step over the rows ``beam_prefill`` left.  Returns ``(tokens, parents)``: n lists
        over the rows, read back once; the scores and flags stay on the device (``beam_scores``, ``finished``)."""
        W = getattr(self, "beam_W", None)
        if W is None or self.B == 0:
            raise ValueError("beam_round before beam_prefill")
        eos_id = self._beam_ids[0] if eos_id is None else eos_id
        sp2_id = self._beam_ids[1] if sp2_id is None else sp2_id
        if eos_id is None or sp2_id is None:
            raise ValueError("beam_round needs eos_id and sp2_id (here or at beam_prefill)")
        V = self.m.layout.vocab
        if not 0 <= eos_id < V:
            raise ValueError(f"eos_id {eos_id} outside the vocabulary")
        if n < 1 or self.n_max + n > self.max_len:
            raise ValueError(f"{n} round(s) behind {self.n_max} cache rows: outside [1, max_len {self.max_len} - rows]")
        self._beam_ids = (eos_id, sp2_id)
        R, dev = self.B, self.dev
        toks = torch.empty(n, R, dtype=torch.int64, device=dev)
        pars = torch.empty(n, R, dtype=torch.int32, device=dev)
        fin = self.finished[:R]
        rules = getattr(self, "_beam_rules", None)
        if self.engine != "python":
            p = lambda t: C.c_void_p(t.data_ptr())
            L.call("ergm_decode_run_beams", self._plan, n, W, eos_id, sp2_id, p(self.beam_scores), p(toks), p(pars),
                   p(self._beam_ws), self._beam_ws.numel(), self._stream())
            self.n_max += n
        else:
            tt = torch.full((R,), sp2_id, dtype=torch.int64, device=dev)
            lens = self.lens[:R]
            for i in range(n):
                if rules is not None:
                    ops.logit_rules(self._logits, V, rules, self.lens, eos_id, self.max_len, finished=fin)
                ops.beam_select(self._logits, V, W, self.beam_scores, fin, eos_id, parent=pars[i], token=toks[i],
                                ws=self._beam_ws)
                ops.beam_gather(self.kv, pars[i], self.lens, W, max_len=self.n_max)
                if rules is not None:
                    ops.hist_follow(self._beam_hist, pars[i], self.lens, W, self.max_len)
                    ops.hist_append(toks[i], self.lens, self._beam_hist, self.max_len, finished=fin)
                self._logits = self._step_rows(toks[i], tt, lens, self.cap_lens[:R], [t[:R] for t in self.kv], self.xkv)
                lens.add_((fin == 0).to(torch.int32))
                self.n_max += 1
        return toks.cpu().tolist(), pars.cpu().tolist()

    @torch.no_grad()
    def beam_search(self, prompts, num_beams: int, eos_id: int, sp2_id: int, max_new_tokens: Optional[int] = None,
                    length_penalty: float = 1.0, num_return: int = 1, no_repeat_ngram_size: int = 0,
                    no_repeat_scope: str = "sequence", bad_words_ids=()):
        """Beam search of ``num_beams`` beams per prompt, the responses typed as speaker 2: the prefill, then chunks of
        8 rounds with a look at ``finished`` in between, until every row is finished or ``max_new_tokens`` rounds ran.
        Returns, per prompt, ``num_return`` pairs ``(tokens, sum_logprob)``, best first by
        ``sum_logprob / len(tokens) ** length_penalty`` (ties by row); each hypothesis ends at its first ``eos_id``
        (included) or at ``max_new_tokens``.  The device ranks the beams by the raw sum of log-probabilities: the
        length penalty acts on this final ordering only, not during the search.  ``no_repeat_ngram_size`` /
        ``no_repeat_scope`` / ``bad_words_ids``: ``beam_prefill``'s, one setting for all prompts."""
        self._beam_check(len(prompts), num_beams)
        if isinstance(num_return, bool) or not isinstance(num_return, int) or not 1 <= num_return <= num_beams:
            raise ValueError(f"num_return {num_return!r} outside [1, num_beams {num_beams}]")
        if not 0 <= eos_id < self.m.layout.vocab:
            raise ValueError(f"eos_id {eos_id} outside the vocabulary")
        bound = self.max_len - max(int(p[0].numel()) for p in prompts)
        if max_new_tokens is None:
            max_new_tokens = bound
        if max_new_tokens < 1 or max_new_tokens > bound:
            raise ValueError(f"max_new_tokens {max_new_tokens} outside [1, {bound}] (max_len - the longest prompt)")
        self.beam_prefill(prompts, num_beams, eos_id, sp2_id, no_repeat_ngram_size, no_repeat_scope, bad_words_ids)
        tokens, parents, done = [], [], 0
        while True:
            n = min(8, max_new_tokens - done)
            t, p = self.beam_round(n)
            tokens += t
            parents += p
            done += n
            if done == max_new_tokens or bool(self.finished[:self.B].all()):
                break
        return beam_backtrack(tokens, parents, self.beam_scores.cpu().tolist(), num_beams, eos_id, length_penalty,
                              num_return)


def beam_backtrack(tokens, parents, scores, num_beams: int, eos_id: int, length_penalty: float = 1.0, num_return: int = 1):
    """The hypotheses of a finished beam search, on the host.  ``tokens`` / ``parents``: one list over the R rows per
    round (``BatchedGenerator.beam_round``), ``scores`` the rows' final sums of log-probabilities.  The hypothesis of
    row r is read backwards through ``parents`` and ends at its first ``eos_id`` (included); a row at -inf has none.
    Returns, per group of ``num_beams`` rows, up to ``num_return`` pairs ``(tokens, score)``, best first by
    ``score / len(tokens) ** length_penalty``, ties by row."""
    R = len(scores)
    if num_beams < 1 or R % num_beams or not 1 <= num_return <= num_beams:
        raise ValueError(f"{R} rows, num_beams {num_beams}, num_return {num_return}")
    out = []
    for g0 in range(0, R, num_beams):
        hyps = []
        for r in range(g0, g0 + num_beams):
            if not scores[r] > -math.inf:
                continue
            seq, row = [], r
            for i in range(len(tokens) - 1, -1, -1):
                seq.append(int(tokens[i][row]))
                row = int(parents[i][row])
            seq.reverse()
            if eos_id in seq:
                seq = seq[:seq.index(eos_id) + 1]
            hyps.append((-(scores[r] / len(seq) ** length_penalty) if seq else math.inf, r, seq, float(scores[r])))
        hyps.sort(key=lambda h: (h[0], h[1]))
        out.append([(h[2], h[3]) for h in hyps[:num_return]])
    return out


NO_REQUEST = -1
NGRAM_MAX = L.NGRAM_MAX          # the longest n-gram and the longest bad-word sequence (ERGM_NGRAM_MAX)
RULE_SCOPES = ("sequence", "turn")


def check_rules(no_repeat_ngram_size, no_repeat_scope, bad_words_ids) -> tuple:
    """Validate the arguments of the logit rules (ergm_hip.h, "Logit rules") and return ``bad_words_ids`` as a tuple of
    tuples: n an integer in [0, 8], the scope "sequence" or "turn", every sequence of 1 .. 8 ids >= 0."""
    n = no_repeat_ngram_size
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= NGRAM_MAX:
        raise ValueError(f"no_repeat_ngram_size {n!r} is not an integer in [0, {NGRAM_MAX}]")
    if no_repeat_scope not in RULE_SCOPES:
        raise ValueError(f"no_repeat_scope {no_repeat_scope!r} is not one of {RULE_SCOPES}")
    if isinstance(bad_words_ids, (str, bytes)) or not hasattr(bad_words_ids, "__iter__"):
        raise ValueError("bad_words_ids must be a sequence of token-id sequences")
    words = []
    for w in bad_words_ids:
        if isinstance(w, (str, bytes)) or not hasattr(w, "__iter__"):
            raise ValueError("bad_words_ids must be a sequence of token-id sequences")
        w = tuple(w)
        if not 1 <= len(w) <= NGRAM_MAX:
            raise ValueError(f"a bad-word sequence has {len(w)} tokens: outside [1, {NGRAM_MAX}]")
        for t in w:
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < 2 ** 31:
                raise ValueError(f"bad-word token {t!r} is not an integer in [0, 2^31)")
        words.append(w)
    return tuple(words)


def pack_bad_words(bad_words_ids, cap: int) -> List[int]:
    """The pool row of a bad-word list: each sequence as its length followed by its tokens, zeros to ``cap`` (a zero
    length ends the run; a list that fills the row exactly needs none).  ValueError when it does not fit."""
    row: List[int] = []
    for w in bad_words_ids:
        row += [len(w), *w]
    if len(row) > cap:
        raise ValueError(f"bad_words_ids take {len(row)} pool entries (one per token and one per sequence) > "
                         f"bad_words_cap {cap}")
    return row + [0] * (cap - len(row))


@dataclass(frozen=True)
class SamplingParams:
    """What one request asks of the sampler (ergm_sample_rows applies them in this order): ``repetition_penalty`` over
    the tokens its cache holds and the ones it drew, no eos before ``min_new_tokens`` tokens of the turn,
    ``temperature``, ``top_k`` (0: off; 1: greedy), then ``top_p`` over what top-k left (None: the run's).
    ``logprobs``: keep the log-probability of every returned token (``ContinuousGenerator.token_logprobs``).

    Two bans precede all of these (ergm_logit_rules_apply; a banned token holds no mass, eos is never banned):
    ``no_repeat_ngram_size`` = n in 1 .. 8: no n-gram may occur twice, Hugging Face's NoRepeatNGramLogitsProcessor, over
    the whole sequence, prompt included (``no_repeat_scope="sequence"``), or over the tokens generated in the current
    turn only (``"turn"``: the other speaker's words and earlier turns do not count); ``bad_words_ids``: sequences of
    1 .. 8 token ids none of which may be completed (lists are accepted and stored as tuples)."""
    top_p: Optional[float] = None
    temperature: float = 1.0
    top_k: int = 0
    repetition_penalty: float = 1.0
    min_new_tokens: int = 0
    logprobs: bool = False
    no_repeat_ngram_size: int = 0
    no_repeat_scope: str = "sequence"
    bad_words_ids: tuple = ()

    def __post_init__(self):
        object.__setattr__(self, "bad_words_ids",
                           check_rules(self.no_repeat_ngram_size, self.no_repeat_scope, self.bad_words_ids))
        for name in ("top_p", "temperature", "repetition_penalty"):
            v = getattr(self, name)
            if v is None and name == "top_p":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} {v!r} is not a finite number")
        if self.temperature <= 0 or self.repetition_penalty <= 0:
            raise ValueError("temperature and repetition_penalty must be positive")
        for name in ("top_k", "min_new_tokens"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 31:
                raise ValueError(f"{name} {v!r} is not an integer in [0, 2^31)")

    @property
    def has_rules(self) -> bool:
        return self.no_repeat_ngram_size > 0 or bool(self.bad_words_ids)

    def check_bound(self, max_new_tokens: int) -> None:
        if self.min_new_tokens > max_new_tokens:
            raise ValueError(f"min_new_tokens {self.min_new_tokens} > max_new_tokens {max_new_tokens}")


class _Request:
    __slots__ = ("id", "n", "c", "max_new", "payload", "tokens", "slot", "keep", "past", "sampling", "rounds", "cols", "share")

    def __init__(self, rid: int, n: int, c: int, max_new: int, payload, keep: bool = False, past: int = 0, sampling=None):
        self.id, self.n, self.c, self.max_new, self.payload = rid, n, c, max_new, payload
        self.tokens: List[int] = []
        self.rounds = 0            # beam mode: the rounds run since the admission
        self.cols: List[tuple] = []   # beam mode: per round, the group's (tokens, parents within the group)
        self.slot = NO_REQUEST
        self.share = None     # a continuation of a stored session: the byte count its blob is accounted under
        self.keep = keep      # park the slot when the request ends
        self.past = past      # a continuation: the rows its slot already holds (n counts the new ones)
        self.sampling = sampling   # a SamplingParams or None, for the backend


class SlotScheduler:
    """The host-side policy of continuous batching, with the device work behind ``backend``:

    * ``backend.admit_requests(slots, requests)`` prefills the requests (``.id``, ``.n``, ``.c``, ``.max_new``,
      ``.payload``) into the named free slots;
    * ``backend.run_chunk(n)`` runs n sample + step rounds over every slot and returns ``(tokens, finished)``:
      tokens as n lists of one token per slot, finished as one flag per slot, read back once;
    * ``backend.retire(slot, request)`` (optional) is told when a request leaves its slot or is parked in it;
    * ``backend.extend_requests(slots, requests)`` (optional; needed by ``extend``) appends the ``.n`` new tokens of
      each continuation (``.payload``) behind the ``.past`` rows its slot holds;
    * ``backend.check_sampling(sampling)`` (optional) raises ValueError at ``submit`` / ``extend`` for a
      ``SamplingParams`` the backend cannot serve, so that a refused request leaves nothing behind.

    Requests wait in arrival order (FIFO) and are admitted at a look, at most ``max_admit`` sequences and
    ``max_admit_tokens`` packed prompt rows per ``admit`` call, as many calls as fill the free slots; a request that does
    not fit the current call waits for the next one, and nothing overtakes it.  A free slot is chosen by least recent
    admission (ties by index), so the slots take turns.  The host looks once in ``look`` steps (8, the cadence of
    ``BatchedGenerator.generate``): it appends the chunk's tokens to the live requests, each list ending at its first
    eos (included) or at ``max_new_tokens``, and retires the requests that ended.

    Sessions: a request submitted with ``keep=True`` keeps its slot when it ends; it is *parked*, with the length its
    cache holds: ``n + len(tokens)``, less one when the last token is the eos, because an eos that was drawn is never
    stepped into the cache, while a request that ends at its bound has its last token there.  (A continuation that
    wants the eos as a separator begins with it.)  ``extend`` queues more tokens for a parked request; at a look the
    waiting continuations go first, grouped under the same ``max_admit`` / ``max_admit_tokens`` limits, one
    ``extend_requests`` call per group, and the admissions into free slots follow.  The new turn's tokens are returned
    under the same id.  ``release`` frees a parked slot.  A parked slot is stepped like any finished slot: the step's
    append lands in the row behind its length, which the next extension overwrites before it reads it.  A slot parked
    with its cache full (length ``max_len``) has no room and cannot be continued, only released.

    ``store=True``: the session store.  A parked session may leave its slot: it is then *stored* (``stored``: id ->
    (rows, caption rows)), which frees the slot, and returns into any free slot when its next turn arrives.  The backend
    adds ``save_sessions(slots, ids)`` (pack the parked sessions of these slots away under their ids; the ids are still
    in ``parked`` during the call), ``load_sessions(slots, ids)`` (unpack stored sessions into free slots, parked),
    ``drop_session(id)`` (forget a stored session), ``fork_session(id, new_id)`` (a second stored session with the same
    contents) and, optionally, ``session_bytes(slot, rows, c)`` (what a parked session costs, for ``store_bytes``).  At each look,
    before the continuations and the admissions:

    1. ``want`` = the waiting continuations of stored sessions + the queued requests; when that exceeds the free slots,
       ``min(want - free, evictable)`` parked sessions are evicted, the least recently parked first (ties by slot), in
       one ``save_sessions`` call.  A session whose continuation waits is not in ``parked`` and is never evicted; one
       that would take the stored bytes above ``store_bytes`` is passed over.
    2. The stored sessions with a waiting continuation take free slots in arrival order, the slot chosen as an
       admission's is, in one ``load_sessions`` call; those that find no slot keep their place and go first next time.
    3. The continuations and the admissions follow as without a store.

    ``extend`` and ``release`` take stored ids as they take parked ones; ``offload`` stores a parked session at once;
    ``fork`` gives a second id the same history (both share one stored copy, which is never written again).  Without a
    byte cap the all-parked deadlock cannot occur; with one that blocks the eviction it is raised as before.  With
    ``store=False`` nothing changes."""

    def __init__(self, backend, max_batch: int, max_len: int, cap_max: int, max_admit: Optional[int] = None,
                 max_admit_tokens: Optional[int] = None, look: int = 8, store: bool = False,
                 store_bytes: Optional[int] = None):
        if max_batch < 1 or max_len < 2 or cap_max < 1 or look < 1:
            raise ValueError("max_batch, cap_max, look must be at least 1 and max_len at least 2")
        if store_bytes is not None and (not store or isinstance(store_bytes, bool) or not isinstance(store_bytes, int)
                                        or store_bytes < 0):
            raise ValueError(f"store_bytes {store_bytes!r} needs store=True and a non-negative integer")
        self.store, self.store_bytes = bool(store), store_bytes
        self.stored: dict = {}                # id -> (rows in its blob, caption rows)
        self.stored_waiting: List[_Request] = []   # continuations of stored sessions waiting for a slot, arrival order
        self.stored_bytes = 0                 # what the stored sessions cost (a fork shares its origin's blob)
        self._share: dict = {}                # stored id -> [bytes, ids sharing the blob]
        self._parked_at: dict = {}            # parked id -> the look it was parked at
        self._looks = 0
        self.saves: List[List[tuple]] = []    # per save_sessions call: (session id, slot) pairs
        self.loads: List[List[tuple]] = []    # per load_sessions call: (session id, slot) pairs
        self.backend, self.max_batch, self.max_len, self.cap_max, self.look = backend, max_batch, max_len, cap_max, look
        self.max_admit = max_batch if max_admit is None else max_admit
        self.max_admit_tokens = max_batch * max_len if max_admit_tokens is None else max_admit_tokens
        if not 1 <= self.max_admit <= max_batch or self.max_admit_tokens < 1:
            raise ValueError("max_admit must lie in [1, max_batch] and max_admit_tokens be at least 1")
        self.queue: List[_Request] = []
        self.continuations: List[_Request] = []   # extensions waiting for the next look, in arrival order
        self.live: List[Optional[_Request]] = [None] * max_batch
        self.parked: dict = {}                # id -> (slot, rows in its cache, caption rows)
        self._held = set()                    # slots parked or waiting for their continuation: not free
        self._last_admit = [-1] * max_batch   # the admit call that last filled each slot
        self._calls = 0
        self._next_id = 0
        self._active = set()                  # ids queued, live or parked: a result is returned under its id
        self.steps = 0                        # decode steps run so far
        self.admissions: List[List[tuple]] = []   # per admit call: (request id, slot) pairs, for tests and tools
        self.extensions: List[List[tuple]] = []   # per extend_requests call: (request id, slot) pairs

    def submit(self, n: int, c: int, max_new_tokens: Optional[int] = None, request_id: Optional[int] = None,
               payload=None, keep: bool = False, sampling=None) -> int:
        """Queue a request with a prompt of n tokens and c caption tokens; returns its id (uint32, arrival order by
        default).  ``keep``: park the slot when the request ends, for ``extend``.  ``sampling``: a ``SamplingParams``
        the backend finds on the request (``.sampling``).  Raises ValueError when it can never be served: it would not
        fit a cache or one admission, or its minimum length is above its bound."""
        if n < 1 or c < 1:
            raise ValueError("empty prompt or caption")
        if n >= self.max_len:
            raise ValueError(f"prompt of {n} tokens leaves no room in a cache of max_len {self.max_len}")
        if c > self.cap_max:
            raise ValueError(f"caption of {c} tokens > cap_max {self.cap_max}")
        if n > self.max_admit_tokens:
            raise ValueError(f"prompt of {n} tokens > max_admit_tokens {self.max_admit_tokens}")
        if max_new_tokens is None:
            max_new_tokens = self.max_len - n
        if not 1 <= max_new_tokens <= self.max_len - n:
            raise ValueError(f"max_new_tokens {max_new_tokens} outside [1, {self.max_len - n}] (max_len - the prompt)")
        if sampling is not None:
            sampling.check_bound(max_new_tokens)
            self._backend_check(sampling)
        rid = self._next_id if request_id is None else request_id
        if not 0 <= rid < 2 ** 32:
            raise ValueError("request ids are uint32")
        if rid in self._active:
            raise ValueError(f"request id {rid} is already queued or running")
        self._active.add(rid)
        self._next_id = (rid + 1) % 2 ** 32 if request_id is None else self._next_id
        self.queue.append(_Request(rid, n, c, max_new_tokens, payload, keep, sampling=sampling))
        return rid

    def extend(self, request_id: int, n_new: int, max_new_tokens: Optional[int] = None, payload=None,
               keep: bool = True, sampling=None) -> int:
        """Queue n_new more tokens (``payload``) for a parked request and up to max_new_tokens new ones behind them
        (default: to the end of the cache); its slot stays held until the next look.  Raises ValueError when the id is
        not parked, n_new is outside [1, max_admit_tokens], or the cache has no room for the new rows and one new
        token; also when the slot holds fewer than 2 rows (a one-token prompt that drew eos at once: the first two
        positions belong to the admission)."""
        if request_id not in self.parked and request_id not in self.stored:
            raise ValueError(f"request id {request_id} is not parked" + (" or stored" if self.store else ""))
        if getattr(self.backend, "extend_requests", None) is None:
            raise ValueError("the backend cannot extend a request (no extend_requests)")
        is_stored = request_id in self.stored
        slot, length, c = (NO_REQUEST, *self.stored[request_id]) if is_stored else self.parked[request_id]
        if not 1 <= n_new <= self.max_admit_tokens:
            raise ValueError(f"{n_new} new tokens outside [1, max_admit_tokens {self.max_admit_tokens}]")
        room = self.max_len - length - n_new
        if room < 1:
            raise ValueError(f"{length} rows + {n_new} new tokens leave no room for one more in a cache of max_len "
                             f"{self.max_len}")
        if length < 2:
            raise ValueError(f"request id {request_id} holds {length} row: nothing to continue")
        if max_new_tokens is None:
            max_new_tokens = room
        if not 1 <= max_new_tokens <= room:
            raise ValueError(f"max_new_tokens {max_new_tokens} outside [1, {room}]")
        if sampling is not None:
            sampling.check_bound(max_new_tokens)
            self._backend_check(sampling)
        r = _Request(request_id, n_new, c, max_new_tokens, payload, keep, past=length, sampling=sampling)
        r.slot = slot
        if is_stored:   # it waits for a slot first: the next look loads it
            del self.stored[request_id]
            r.share = self._share.pop(request_id)
            self.stored_waiting.append(r)
            return request_id
        del self.parked[request_id]
        self._parked_at.pop(request_id, None)
        self.continuations.append(r)
        return request_id

    def _backend_check(self, sampling) -> None:
        """``backend.check_sampling(sampling)`` (optional) refuses, with ValueError, what the backend cannot serve."""
        check = getattr(self.backend, "check_sampling", None)
        if check is not None:
            check(sampling)

    def release(self, request_id: int) -> None:
        """Free the slot of a parked request, or forget a stored one."""
        if request_id in self.stored:
            del self.stored[request_id]
            self._unshare(request_id, self._share.pop(request_id))
            self.backend.drop_session(request_id)
            self._active.discard(request_id)
            return
        if request_id not in self.parked:
            raise ValueError(f"request id {request_id} is not parked" + (" or stored" if self.store else ""))
        slot, _, _ = self.parked.pop(request_id)
        self._parked_at.pop(request_id, None)
        self._held.discard(slot)
        self._active.discard(request_id)

    # ---- the session store ----------------------------------------------------------------------------------
    def _need_store(self, what: str) -> None:
        if not self.store:
            raise ValueError(f"{what} needs the session store (store=True)")

    def _session_bytes(self, slot: int, rows: int, c: int) -> int:
        size = getattr(self.backend, "session_bytes", None)
        return 0 if size is None else int(size(slot, rows, c))

    def _unshare(self, request_id: int, share: list) -> None:
        """``request_id`` no longer uses the blob ``share`` accounts for; the last user's leaving frees its bytes."""
        share[1].discard(request_id)
        if not share[1]:
            self.stored_bytes -= share[0]

    def _save(self, ids: List[int]) -> None:
        """The parked sessions ``ids`` leave their slots in one ``save_sessions`` call."""
        slots = [self.parked[i][0] for i in ids]
        nbytes = [self._session_bytes(*self.parked[i]) for i in ids]
        self.backend.save_sessions(slots, ids)
        for i, b in zip(ids, nbytes):
            slot, rows, c = self.parked.pop(i)
            self._parked_at.pop(i, None)
            self._held.discard(slot)
            self.stored[i] = (rows, c)
            self._share[i] = [b, {i}]
            self.stored_bytes += b
        self.saves.append(list(zip(ids, slots)))

    def _fits(self, nbytes: int) -> bool:
        return self.store_bytes is None or self.stored_bytes + nbytes <= self.store_bytes

    def offload(self, request_id: int) -> None:
        """Store a parked session at once, which frees its slot; a stored id is left as it is.  Raises ValueError for an
        id that is neither parked nor stored (a waiting continuation included) and when ``store_bytes`` has no room."""
        self._need_store("offload")
        if request_id in self.stored:
            return
        if request_id not in self.parked:
            raise ValueError(f"request id {request_id} is not parked or stored")
        if not self._fits(self._session_bytes(*self.parked[request_id])):
            raise ValueError(f"request id {request_id}: store_bytes {self.store_bytes} has no room for the session")
        self._save([request_id])

    def fork(self, request_id: int, new_id: Optional[int] = None) -> int:
        """A second session with the history of ``request_id`` under ``new_id`` (default: the next id), stored; a parked
        origin is offloaded first.  Both share one stored copy.  Raises ValueError for an id that is neither parked nor
        stored (a waiting continuation included) and for a ``new_id`` in use."""
        self._need_store("fork")
        if request_id not in self.stored and request_id not in self.parked:
            raise ValueError(f"request id {request_id} is not parked or stored")
        rid = self._next_id if new_id is None else new_id
        if not 0 <= rid < 2 ** 32:
            raise ValueError("request ids are uint32")
        if rid in self._active:
            raise ValueError(f"request id {rid} is already queued or running")
        self.offload(request_id)
        self.backend.fork_session(request_id, rid)
        self.stored[rid] = self.stored[request_id]
        share = self._share[rid] = self._share[request_id]
        share[1].add(rid)
        self._active.add(rid)
        self._next_id = (rid + 1) % 2 ** 32 if new_id is None else self._next_id
        return rid

    def _free_slots(self) -> List[int]:
        return sorted((s for s in range(self.max_batch) if self.live[s] is None and s not in self._held),
                      key=lambda s: (self._last_admit[s], s))

    def _restore(self) -> None:
        """The store's part of a look: evictions, then the stored sessions whose continuation waits."""
        self._looks += 1
        want, free = len(self.stored_waiting) + len(self.queue), len(self._free_slots())
        if want > free:
            evict, nbytes = [], 0
            for rid, (slot, rows, c) in sorted(self.parked.items(), key=lambda kv: (self._parked_at.get(kv[0], 0), kv[1][0])):
                if len(evict) == want - free:
                    break
                b = self._session_bytes(slot, rows, c)
                if self._fits(nbytes + b):
                    evict.append(rid)
                    nbytes += b
            if evict:
                self._save(evict)
        free = self._free_slots()
        batch = self.stored_waiting[:len(free)]
        if not batch:
            return
        del self.stored_waiting[:len(batch)]
        slots = free[:len(batch)]
        self.backend.load_sessions(slots, [r.id for r in batch])
        for s, r in zip(slots, batch):   # loaded: a parked slot whose continuation waits
            r.slot, self._last_admit[s] = s, self._calls
            self._held.add(s)
            self._unshare(r.id, r.share)
            r.share = None
            self.backend.drop_session(r.id)
            self.continuations.append(r)
        self._calls += 1
        self.loads.append([(r.id, s) for s, r in zip(slots, batch)])

    def _extend(self) -> None:
        while self.continuations:
            batch, rows = [], 0
            while (self.continuations and len(batch) < self.max_admit
                   and rows + self.continuations[0].n <= self.max_admit_tokens):
                r = self.continuations.pop(0)
                rows += r.n
                batch.append(r)
            slots = [r.slot for r in batch]
            self.backend.extend_requests(slots, batch)
            for r in batch:
                self._held.discard(r.slot)
                self.live[r.slot] = r
            self.extensions.append([(r.id, r.slot) for r in batch])

    def _admit(self) -> None:
        while self.queue:
            free = sorted((s for s in range(self.max_batch) if self.live[s] is None and s not in self._held),
                          key=lambda s: (self._last_admit[s], s))
            batch, rows = [], 0
            while (self.queue and len(batch) < min(self.max_admit, len(free))
                   and rows + self.queue[0].n <= self.max_admit_tokens):
                r = self.queue.pop(0)
                rows += r.n
                batch.append(r)
            if not batch:
                return
            slots = free[:len(batch)]
            self.backend.admit_requests(slots, batch)
            for s, r in zip(slots, batch):
                r.slot, self.live[s], self._last_admit[s] = s, r, self._calls
            self.admissions.append([(r.id, s) for s, r in zip(slots, batch)])
            self._calls += 1

    def drain(self, eos_id: int):
        """Run until nothing is queued and nothing is running, yielding (id, tokens) of each request as it retires or
        is parked; parked sessions do not keep it alive.  Raises RuntimeError when new requests wait, nothing runs and
        every slot is parked: nothing could ever change."""
        while self.queue or self.continuations or self.stored_waiting or any(r is not None for r in self.live):
            if self.store:
                self._restore()
            self._extend()
            self._admit()
            if all(r is None for r in self.live):
                n = len(self.queue) + len(self.stored_waiting)
                raise RuntimeError(f"{n} request(s) wait and every slot is parked: release a session"
                                   + (f" (store_bytes {self.store_bytes} leaves no room to store one)" if self.store else ""))
            tokens, finished = self.backend.run_chunk(self.look)
            self.steps += self.look
            for s, r in enumerate(self.live):
                if r is None:
                    continue
                done = False
                for row in tokens:
                    tok = int(row[s])
                    r.tokens.append(tok)
                    if tok == eos_id or len(r.tokens) == r.max_new:
                        done = True
                        break
                if done != bool(finished[s]):
                    raise RuntimeError(f"slot {s}: the device says finished = {int(finished[s])}, the tokens say {done}")
                if done:
                    self.live[s] = None
                    if r.keep:   # an eos that was drawn is never stepped into the cache
                        rows = r.past + r.n + len(r.tokens) - (1 if r.tokens[-1] == eos_id else 0)
                        self.parked[r.id] = (s, rows, r.c)
                        self._parked_at[r.id] = self._looks
                        self._held.add(s)
                    else:
                        self._active.discard(r.id)
                    retire = getattr(self.backend, "retire", None)
                    if retire is not None:
                        retire(s, r)
                    yield r.id, r.tokens

    def run(self, eos_id: int) -> dict:
        return dict(self.drain(eos_id))


class BeamScheduler(SlotScheduler):
    """``SlotScheduler``'s policy over groups of ``num_beams`` slots (queue, FIFO admission under ``max_admit`` /
    ``max_admit_tokens``, the least recently admitted free group first, a look every ``look`` rounds), for beam search
    in slot mode.  What the scheduler calls a slot is a group here: group g owns rows g·W .. g·W + W - 1.

    * ``backend.admit_requests(groups, requests)`` prefills each request into row g·W of its group and seeds the group;
    * ``backend.run_beam_chunk(n)`` runs n select + gather + step rounds over every row and returns ``(tokens, parents,
      finished, scores)``: n lists of one token / one parent row per row, one flag and one score per row, read back once;
    * ``backend.retire(group, request)`` (optional) is told when a request leaves its group.

    The host keeps a live group's (tokens, parents) columns from its admission round on.  A group retires at the first
    look at which all its rows are finished on the device (eos on every beam, or the bound of the admission); the host
    cross-checks that a group whose rounds reached ``max_new_tokens`` is finished.  A chunk runs on past a request's
    bound (finished rows offer eos at unchanged scores), so the hypotheses are read back over exactly
    ``min(rounds, max_new_tokens)`` rounds (``beam_backtrack``).  No sessions: ``keep`` and ``extend`` are refused."""

    def __init__(self, backend, n_groups: int, num_beams: int, max_len: int, cap_max: int, max_admit: Optional[int] = None,
                 max_admit_tokens: Optional[int] = None, look: int = 8):
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= 8:
            raise ValueError(f"num_beams {num_beams!r} outside [1, 8]")
        super().__init__(backend, n_groups, max_len, cap_max, max_admit, max_admit_tokens, look)
        self.num_beams = num_beams

    def submit(self, n: int, c: int, max_new_tokens: Optional[int] = None, request_id: Optional[int] = None,
               payload=None, keep: bool = False, sampling=None) -> int:
        if keep:
            raise ValueError("beam mode has no sessions (keep=True)")
        return super().submit(n, c, max_new_tokens, request_id, payload, False, sampling)

    def extend(self, *args, **kwargs) -> int:
        raise ValueError("beam mode has no sessions (extend)")

    def drain(self, eos_id: int, length_penalty: float = 1.0, num_return: int = 1):
        """Run until nothing is queued and nothing is running, yielding (id, [(tokens, sum_logprob), ...]) of each
        request as its group retires: ``beam_backtrack``'s result for the group."""
        W = self.num_beams
        if isinstance(num_return, bool) or not isinstance(num_return, int) or not 1 <= num_return <= W:
            raise ValueError(f"num_return {num_return!r} outside [1, num_beams {W}]")
        while self.queue or any(r is not None for r in self.live):
            self._admit()
            tokens, parents, finished, scores = self.backend.run_beam_chunk(self.look)
            self.steps += self.look
            for g, r in enumerate(self.live):
                if r is None:
                    continue
                r0 = g * W
                for trow, prow in zip(tokens, parents):
                    par = [int(p) - r0 for p in prow[r0:r0 + W]]
                    if min(par) < 0 or max(par) >= W:
                        raise RuntimeError(f"group {g}: a parent row outside the group ({prow[r0:r0 + W]})")
                    r.cols.append(([int(t) for t in trow[r0:r0 + W]], par))
                r.rounds += self.look
                done = all(bool(f) for f in finished[r0:r0 + W])
                if r.rounds >= r.max_new and not done:
                    raise RuntimeError(f"group {g}: {r.rounds} rounds ran for a bound of {r.max_new} and the device says "
                                       f"finished = {[int(f) for f in finished[r0:r0 + W]]}")
                if not done:
                    continue
                k = min(r.rounds, r.max_new)   # the chunk ran on past the bound: those rounds are not the request's
                hyps = beam_backtrack([c[0] for c in r.cols[:k]], [c[1] for c in r.cols[:k]],
                                      [float(s) for s in scores[r0:r0 + W]], W, eos_id, length_penalty, num_return)[0]
                self.live[g] = None
                self._active.discard(r.id)
                r.cols = []
                retire = getattr(self.backend, "retire", None)
                if retire is not None:
                    retire(g, r)
                yield r.id, hyps

    def run(self, eos_id: int, length_penalty: float = 1.0, num_return: int = 1) -> dict:
        return dict(self.drain(eos_id, length_penalty, num_return))


def _u32_as_i32(x: int) -> int:
    return x - 2 ** 32 if x >= 2 ** 31 else x


@dataclass
class SequenceScore:
    """What ``ContinuousGenerator.score`` returns for one sequence: ``logprobs[i]`` = log p(token first + i | the tokens
    before it, captions, features) and ``top1[i]`` = the token the model ranks first at that position."""
    logprobs: List[float]
    top1: List[int]

    @property
    def sum(self) -> float:
        return float(sum(self.logprobs))

    @property
    def ppl(self) -> float:
        return math.exp(-self.sum / len(self.logprobs))


def score_targets(ids: List[List[int]], first: List[int]) -> List[int]:
    """The packed targets of a scoring group: packed row s of sequence b holds ids[b][s + 1] when s + 1 >= first[b], else
    -100; a sequence's last row holds -100."""
    out: List[int] = []
    for seq, f in zip(ids, first):
        out += [seq[s + 1] if s + 1 >= f else -100 for s in range(len(seq) - 1)] + [-100]
    return out


def score_groups(lens: List[int], max_admit: int, max_admit_tokens: int) -> List[tuple]:
    """[lo, hi) index ranges that cut the sequences, in order, into groups of at most max_admit sequences and
    max_admit_tokens packed rows: the scheduler's admission rule.  A sequence longer than max_admit_tokens fits none."""
    groups, lo, rows = [], 0, 0
    for i, n in enumerate(lens):
        if n > max_admit_tokens:
            raise ValueError(f"sequence {i} has {n} tokens > max_admit_tokens {max_admit_tokens}: it fits no group")
        if i > lo and (i - lo >= max_admit or rows + n > max_admit_tokens):
            groups.append((lo, i))
            lo, rows = i, 0
        rows += n
    if len(lens) > lo:
        groups.append((lo, len(lens)))
    return groups


@dataclass
class _StoredSession:
    """A session in the store: its blob in HBM, the host's copy of the blob's header, and the host records that travel
    with it (``ContinuousGenerator.save_sessions``)."""
    blob: torch.Tensor
    hdr: "L.SessionHdr"
    rid: int                 # the id it draws under
    cap: int                 # the caption rows of its admission (_cap_host)
    sp: Optional[SamplingParams] = None
    hist_host: Optional[list] = None
    ruled: bool = False
    fork: bool = False       # loaded under ``rid`` in place of the id in the blob


class ContinuousGenerator:
    """In-flight batching over ``max_batch`` cache slots: requests are prefilled into free slots while the others keep
    decoding, every step runs over all slots, and a request's result does not depend on what it ran beside (bitwise
    with ``max_admit=1`` on engine "fused", whose rows are independent of their neighbours).

    A prompt is (input_ids, token_type_ids, caption_ids, imgs, auds) as in ``BatchedGenerator.prefill``.  The draw of a
    request's i-th token is ergm_topp_sample_rows' counter {request id, 0, 0xE5A3, i}: seeded runs repeat whatever the
    slot and the neighbours.

    ``engine``: "python" (default, the yardstick) admits with the kernels the static prefill uses, sequence by sequence
    for the embedding and the attention, and drives every kernel of a step from Python; "native" / "fused" hand the
    admission (ergm_decode_admit: packed embedding, ragged attention, rows to slots) and the sample + step chunks
    (ergm_decode_run_slots) to the library's executor.

    ``controls=True``: requests carry a ``SamplingParams`` each (``submit(..., sampling=...)``).  The generator then
    owns one value of every control per slot and the bitmap of the tokens each slot has seen, sets them behind every
    admission and extension (ergm_sample_mark), and samples with ergm_sample_rows (ergm_decode_run_slots_sampled on the
    executor engines): still nothing is read back inside a chunk.  With ``controls=False`` every launch is the one
    described above.

    Logit rules (``SamplingParams.no_repeat_ngram_size`` / ``bad_words_ids``, ``controls=True``): the generator keeps
    the ordered tokens of every slot on the device (``hist`` int32 [max_batch, max_len]) beside one ``start`` / ``ngram``
    value per slot and a pool row of ``bad_words_cap`` entries for its bad words (one per token and one per sequence).
    They are written behind every admission and extension that carries a rule (ergm_hist_write), a new tenant inherits
    nothing, a parked slot keeps its history, and while a ruled request is live every round bans before it samples and
    records what it drew (ergm_logit_rules_apply, ergm_hist_append: two launches more; ergm_decode_set_rules on the
    executor engines).  While none is live the rounds launch what they always did.

    ``num_beams=W`` (1 .. 8, ``max_batch % W == 0``, not with ``controls``): beam mode.  The slots are ``max_batch // W``
    groups, group g rows g·W .. g·W + W - 1, and a request is a beam search of W beams in one group: the admission
    prefills its prompt into row g·W alone, ergm_beam_seed copies the caption K | V to the group's other rows and
    leaves the scores [0, -inf, ...], and every round is ergm_beam_select, ergm_beam_gather and the slot step over all
    rows (ergm_decode_run_slot_beams on the executor engines), so a group ends on the device at eos on every beam or at
    its bound and is served again at the next look (``BeamScheduler``).  ``submit`` takes the logit rules per request,
    ``run_beams`` / ``drain_beams`` / ``beam_search`` serve the queue, and the sampled entry points are refused.

    ``session_store=True`` (not with ``num_beams``): more open conversations than slots.  A parked session's state (its
    cache rows, caption rows, draw counters, controls, seen row, rule state and history) is packed into one blob in HBM
    (ergm_slots_save; a ``torch.uint8`` tensor allocated on the generator's stream), which frees the slot, and unpacked
    into any free slot when its next turn arrives (ergm_slots_load), all enqueued on the generator's stream between
    chunks.  The scheduler evicts the least recently parked sessions when requests wait for slots
    (``SlotScheduler(store=True)``); ``offload`` does it at once, ``fork_request`` gives a second id the same history,
    ``extend_request`` and ``release`` take stored ids, and ``session_store_bytes`` caps what the store may hold.
    ``save_calls`` / ``load_calls`` / ``stored_bytes`` count.  With ``session_store=False`` nothing changes."""

    ENGINES = BatchedGenerator.ENGINES
    num_beams: Optional[int] = None   # beam mode: the beams per request, fixed for the generator's life

    def __init__(self, model, max_batch: int, max_len: int, cap_max: int, engine: str = "python",
                 max_admit: Optional[int] = None, max_admit_tokens: Optional[int] = None, keep_logits: bool = False,
                 controls: bool = False, bad_words_cap: int = 64, num_beams: Optional[int] = None,
                 session_store: bool = False, session_store_bytes: Optional[int] = None):
        if engine not in self.ENGINES:
            raise ValueError(f"engine {engine!r} is not one of {sorted(self.ENGINES)}")
        if session_store and num_beams is not None:
            raise ValueError("session_store and num_beams do not go together: beam mode has no sessions")
        if session_store_bytes is not None and not session_store:
            raise ValueError("session_store_bytes needs session_store=True")
        if num_beams is not None:
            if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= 8:
                raise ValueError(f"num_beams {num_beams!r} outside [1, 8]")
            if max_batch < 1 or max_batch % num_beams:
                raise ValueError(f"max_batch {max_batch} is no positive multiple of num_beams {num_beams}")
            if num_beams > model.layout.vocab:
                raise ValueError(f"num_beams {num_beams} > the vocabulary")
            if controls:
                raise ValueError("num_beams and controls=True do not go together: beam search draws nothing")
        self.num_beams = num_beams
        if isinstance(bad_words_cap, bool) or not isinstance(bad_words_cap, int) or bad_words_cap < 1:
            raise ValueError(f"bad_words_cap {bad_words_cap!r} is not a positive integer")
        self.bad_words_cap = bad_words_cap
        cfg = model.config
        if max_len > cfg.n_positions:
            raise ValueError(f"max_len {max_len} > n_positions {cfg.n_positions}")
        self.engine, self.m, self.cfg = engine, model, cfg
        self.E, self.H, self.L, self.F = cfg.n_embd, cfg.n_head, cfg.n_layer, cfg.inner
        self.max_batch, self.max_len, self.cap_max = max_batch, max_len, cap_max
        if max_admit_tokens is None:
            max_admit_tokens = min(2048, max_batch * max_len)
        if num_beams is None:
            self.sched = SlotScheduler(self, max_batch, max_len, cap_max, max_admit, max_admit_tokens,
                                       store=bool(session_store), store_bytes=session_store_bytes)
        else:   # the same policy over groups of num_beams slots
            self.n_groups = max_batch // num_beams
            self.sched = BeamScheduler(self, self.n_groups, num_beams, max_len, cap_max, max_admit, max_admit_tokens)
        self.keep_logits = keep_logits
        self.final_logits: dict = {}   # keep_logits: id -> the slot's logits row [V] when the request retired
        dev = self.dev = model.flat.device
        E, mb, lay = self.E, max_batch, model.layout
        self.kv = [torch.empty(mb, max_len, 2 * E, dtype=torch.bfloat16, device=dev) for _ in range(self.L)]
        self.xkv = [torch.empty(mb, cap_max, 2 * E, dtype=torch.bfloat16, device=dev) for _ in range(self.L)]
        self._logits = torch.zeros(mb, lay.vocab_pad, dtype=torch.float32, device=dev)
        self.lens = torch.zeros(mb, dtype=torch.int32, device=dev)
        self.cap_lens = torch.zeros(mb, dtype=torch.int32, device=dev)
        self.stop_lens = torch.zeros(mb, dtype=torch.int32, device=dev)
        self.finished = torch.ones(mb, dtype=torch.uint8, device=dev)      # every slot idle
        self.row_ids = torch.zeros(mb, dtype=torch.int32, device=dev)      # uint32 bits
        self.row_steps = torch.zeros(mb, dtype=torch.int32, device=dev)
        self._ws = ops.attn_decode_workspace(mb, self.H, max(max_len, cap_max), dev)
        self._plan = self._plan_ws = self._plan_params = self._admit_ws = None
        self._score_ws = self._plan_dims = None
        self._sampling = None   # (top_p, eos_id, sp2_id, seed) of the run in progress
        self.admit_calls = 0
        self.extend_calls = 0
        self._cap_host = [0] * mb   # the caption rows each slot was admitted with (extend's host check)
        self.controls = controls
        self.token_logprobs: dict = {}   # controls, logprobs=True: id -> one log-probability per token of the turn
        if num_beams is not None:
            self.beam_scores = torch.full((mb,), -math.inf, dtype=torch.float32, device=dev)
            need = L.load().ergm_beam_select_workspace_size(mb, num_beams)
            self._beam_ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
            self._beam_ids = (None, None)              # (eos_id, sp2_id) of the search in progress
            self._grp_rows = [0] * self.n_groups       # host bound on the live lengths of each group (0: idle)
            self.seed_calls = 0
        if controls or num_beams is not None:
            # logit rules: the slots' token histories, start | ngram per slot, and the bad-word pool
            self.hist = torch.zeros(mb, max_len, dtype=torch.int32, device=dev)
            self._rule_vals = torch.zeros(2, mb, dtype=torch.int32, device=dev)
            self._bad_pool = torch.zeros(mb, bad_words_cap, dtype=torch.int32, device=dev)
            self._rules = ops.rules_desc(self.hist, start=self._rule_vals[0], ngram=self._rule_vals[1], bad=self._bad_pool)
            self._slot_ruled = [False] * mb    # the slot's device values hold a rule and its history is kept
            self._rule_live = [False] * mb     # ... and a request is running in it
            self._rules_bound = False          # the executor plan holds the rules (ergm_decode_set_rules)
        if controls:
            # rows: top_p, temperature, repetition penalty (f32 bits) and top_k, one column per slot
            self._ctl_vals = torch.zeros(4, mb, dtype=torch.int32, device=dev)
            self._ctl_vals[:3].view(torch.float32).fill_(1.0)
            self.min_step = torch.zeros(mb, dtype=torch.int32, device=dev)                        # uint32 bits
            self.seen = torch.zeros(mb, (lay.vocab + 31) // 32, dtype=torch.int32, device=dev)    # uint32 bits
            f = lambda i: self._ctl_vals[i].view(torch.float32)
            self._ctl = ops.sample_ctl(top_p=f(0), temperature=f(1), rep_penalty=f(2), top_k=self._ctl_vals[3],
                                       min_step=self.min_step, seen=self.seen)
            self._slot_sp: List[Optional[SamplingParams]] = [None] * mb   # what each slot was last given
            self._lp_acc: List[Optional[list]] = [None] * mb              # the log-probabilities of the turn so far
            self._hist_host: List[list] = [[] for _ in range(mb)]   # what each slot's cache holds, as segments
        self.session_store = bool(session_store)
        self._rid_host = [0] * mb   # the id each slot draws under (a stored session takes it along)
        self._store: dict = {}      # session id -> _StoredSession
        self.save_calls = 0
        self.load_calls = 0
        self._session_state = None
        if engine != "python":
            self._create_plan()

    _f, _b, _ln = KVCacheGenerator._f, KVCacheGenerator._b, KVCacheGenerator._ln
    _gemm, _mlp, _head, _stream = (BatchedGenerator._gemm, BatchedGenerator._mlp, BatchedGenerator._head,
                                   BatchedGenerator._stream)
    _block, _step_rows, _features = BatchedGenerator._block, BatchedGenerator._step_rows, BatchedGenerator._features
    _new_plan, _drop_plan, __del__ = BatchedGenerator._new_plan, BatchedGenerator._drop_plan, BatchedGenerator.__del__

    @property
    def logits(self) -> torch.Tensor:
        """The next-token logits of every slot, [max_batch, V] (fp32)."""
        return self._logits[:, :self.m.layout.vocab]

    def _create_plan(self) -> None:
        self.m.refresh_bf16()
        dims = self._plan_dims = self._new_plan(self.cap_max, capkv=True)
        plan = self._plan
        rows = min(self.sched.max_admit_tokens, self.max_batch * self.max_len)
        need_admit = L.load().ergm_decode_admit_workspace_size(C.byref(dims), rows, self.sched.max_admit * self.cap_max)
        if need_admit == 0:
            raise ValueError("the decode executor does not support this model's dimensions")
        self._admit_ws = torch.empty(need_admit, dtype=torch.uint8, device=self.dev)
        ptrs = C.c_void_p * self.L
        p = lambda t: C.c_void_p(t.data_ptr())
        L.call("ergm_decode_bind_slots", plan, ptrs(*[t.data_ptr() for t in self.kv]),
               ptrs(*[t.data_ptr() for t in self.xkv]), p(self._logits), p(self.lens), p(self.cap_lens), p(self.finished),
               p(self.stop_lens), p(self.row_ids), p(self.row_steps))

    def admit_launches(self, n_seq: int, rows: int, cap_rows: int) -> int:
        """Kernel launches of one native admission of these sizes (ergm_decode_admit_launches)."""
        if self._plan is None:
            raise ValueError("the python engine has no executor plan")
        n = L.load().ergm_decode_admit_launches(self._plan, n_seq, rows, cap_rows)
        if n < 0:
            L.check(n, "ergm_decode_admit_launches")
        return n

    def extend_launches(self, n_seq: int, rows: int) -> int:
        """Kernel launches of one native extension of these sizes (ergm_decode_extend_launches)."""
        if self._plan is None:
            raise ValueError("the python engine has no executor plan")
        n = L.load().ergm_decode_extend_launches(self._plan, n_seq, rows)
        if n < 0:
            L.check(n, "ergm_decode_extend_launches")
        return n

    # ---- admission --------------------------------------------------------------------------------------
    def _resolve(self, sampling, n_seq: int, max_new, slots=None) -> Optional[List[SamplingParams]]:
        """The SamplingParams each of n_seq sequences runs with, checked against its bound, or None without controls.
        An admission's None is the defaults; an extension's (``slots`` given) keeps what the slot has, with no minimum
        length for the new turn."""
        sampling = [None] * n_seq if sampling is None else list(sampling)
        if len(sampling) != n_seq:
            raise ValueError("one sampling value per sequence")
        if not self.controls:
            if any(s is not None for s in sampling):
                raise ValueError("sampling parameters need ContinuousGenerator(controls=True)")
            return None
        for b, s in enumerate(sampling):
            if s is None:
                old = None if slots is None else self._slot_sp[slots[b]]
                sampling[b] = SamplingParams() if old is None else replace(old, min_new_tokens=0)
            sampling[b].check_bound(max_new[b])
            self.check_sampling(sampling[b])
            if sampling[b].top_p is None and self._sampling is None:
                raise ValueError("top_p=None takes the run's top_p: outside run / drain give the request its own")
        return sampling

    def _set_rules(self, slots, sps, ids, q0, lens, past) -> None:
        """The slots' rule values (start, ngram, the bad-word pool row) and their token histories, behind the admission
        or extension that filled them: one copy to the device, two scatters, one ergm_hist_write of the new ids at
        ``past``.  A slot that carried no rule so far has no history on the device: its earlier tokens are written
        from the host's record (a second ergm_hist_write)."""
        rows, late = [], []
        for b, (s, sp) in enumerate(zip(slots, sps)):
            direct = past[b] == 0 or self._slot_ruled[s] or not sp.has_rules
            if not direct:
                late.append(b)
            start = past[b] + lens[b] if sp.no_repeat_scope == "turn" else 0
            rows.append([s, q0[b], lens[b] if direct else 0, past[b], start, sp.no_repeat_ngram_size,
                         *pack_bad_words(sp.bad_words_ids, self.bad_words_cap)])
        m = torch.tensor(rows, dtype=torch.int32).to(self.dev)
        sl = m[:, 0].long()
        self._rule_vals[:, sl] = m[:, 4:6].t()
        self._bad_pool[sl] = m[:, 6:]
        w = m[:, :4].t().contiguous()
        ops.hist_write(ids, w[0], w[1], w[2], self.hist, self.max_len, pos0=w[3])
        if late:
            full = []
            for b in late:
                seq = [int(t) for seg in self._hist_host[slots[b]] for t in (seg.tolist() if torch.is_tensor(seg) else seg)]
                if len(seq) != past[b] + lens[b]:
                    raise ValueError(f"slot {slots[b]}: a rule that starts in a later turn needs the slot's earlier tokens, "
                                     "which are known for requests served by run / drain only: give the rule at admission")
                full.append(seq)
            q = [sum(len(x) for x in full[:i]) for i in range(len(full))]
            w = torch.tensor([[slots[b] for b in late], q, [len(x) for x in full]], dtype=torch.int32).to(self.dev)
            flat = torch.tensor([t for x in full for t in x], dtype=torch.int64).to(self.dev)
            ops.hist_write(flat, w[0], w[1], w[2], self.hist, self.max_len)
        for s, sp in zip(slots, sps):
            self._slot_ruled[s] = self._rule_live[s] = sp.has_rules

    def _set_controls(self, slots, sps, ids, q0, lens, reset: bool, past=None, segs=None) -> None:
        """The slots' control values, their bitmap rows (cleared first at an admission) and their minimum length, behind
        the admission or extension that filled them: one copy to the device, one scatter, one ergm_sample_mark; then the
        logit rules of the slots that carry one or carried one (``_set_rules``)."""
        n_seq = len(slots)
        past = [0] * n_seq if past is None else past
        for b, s in enumerate(slots):   # the host's record of what the slot's cache holds
            if reset:
                self._hist_host[s] = []
            self._hist_host[s].append(segs[b])
        if any(sp.has_rules for sp in sps) or any(self._slot_ruled[s] for s in slots):
            self._set_rules(slots, sps, ids, q0, lens, past)
        top_p = [self._sampling[0] if sp.top_p is None else sp.top_p for sp in sps]
        f = torch.tensor([top_p, [sp.temperature for sp in sps], [sp.repetition_penalty for sp in sps]], dtype=torch.float32)
        i = torch.tensor([[sp.top_k for sp in sps], slots, q0, lens, [int(reset)] * n_seq,
                          [sp.min_new_tokens for sp in sps]], dtype=torch.int32)
        m = torch.cat([f.view(torch.int32), i]).to(self.dev)
        self._ctl_vals[:, m[4].long()] = m[:4]
        ops.sample_mark(ids, m[4], m[5], m[6], self.m.layout.vocab, seen=self.seen, reset=m[7], min_new=m[8],
                        row_steps=self.row_steps, min_step=self.min_step)
        for s, sp in zip(slots, sps):
            self._slot_sp[s] = sp
            self._lp_acc[s] = [] if sp.logprobs else None

    @torch.no_grad()
    def admit(self, slots, prompts, max_new_tokens=None, request_ids=None, sampling=None) -> None:
        """Prefill ``prompts`` into the free ``slots`` (low level; ``submit`` / ``run`` do this through the scheduler).
        max_new_tokens: one bound per prompt (default: to the end of the cache); request_ids: the uint32 ids the
        draws are keyed by (default 0 .. n-1); sampling (``controls=True``): one ``SamplingParams`` or None per prompt."""
        self.m.refresh_bf16()
        n_seq = len(prompts)
        slots = [int(s) for s in slots]
        ids_l = [p[0].reshape(-1) for p in prompts]
        tt_l = [p[1].reshape(-1) for p in prompts]
        cap_l = [p[2].reshape(-1) for p in prompts]
        lens = [int(t.numel()) for t in ids_l]
        clens = [int(t.numel()) for t in cap_l]
        max_new = [self.max_len - n for n in lens] if max_new_tokens is None else [int(x) for x in max_new_tokens]
        rids = list(range(n_seq)) if request_ids is None else [int(x) for x in request_ids]
        if not (n_seq == len(slots) == len(max_new) == len(rids)) or n_seq < 1:
            raise ValueError("admit takes one slot, one bound and one id per prompt")
        if len(set(slots)) != n_seq or min(slots) < 0 or max(slots) >= self.max_batch:
            raise ValueError(f"slots {slots}: outside [0, {self.max_batch}) or named twice")
        for n, c, k in zip(lens, clens, max_new):
            if n < 1 or c < 1 or c > self.cap_max or k < 1 or n + k > self.max_len:
                raise ValueError(f"a prompt of {n} tokens, {c} caption tokens and {k} new tokens does not fit "
                                 f"max_len {self.max_len} / cap_max {self.cap_max}")
        if sum(lens) > self.sched.max_admit_tokens or n_seq > self.sched.max_admit:
            raise ValueError("more sequences or packed rows than one admission takes (max_admit, max_admit_tokens)")
        sps = self._resolve(sampling, n_seq, max_new)
        vis, aud, has = self._features(prompts)
        q0 = [sum(lens[:b]) for b in range(n_seq)]
        c0 = [sum(clens[:b]) for b in range(n_seq)]
        self.admit_calls += 1
        for sl, c, rid in zip(slots, clens, rids):
            self._cap_host[sl], self._rid_host[sl] = c, rid
        if self.engine == "python":
            self._admit_python(slots, ids_l, tt_l, cap_l, lens, clens, q0, c0, max_new, rids, vis, aud, has)
        else:
            self._admit_native(slots, ids_l, tt_l, cap_l, lens, clens, q0, c0, max_new, rids, vis, aud, has)
        if sps is not None:   # behind the admission: it set row_steps, which the minimum length counts from
            self._set_controls(slots, sps, torch.cat(ids_l).to(device=self.dev, dtype=torch.int64), q0, lens, reset=True,
                               segs=ids_l)

    def _packed_python(self, ids_l, tt_l, cap_l, lens, clens, q0, c0, vis, aud, has, keep_kv=None, keep_ckv=None):
        """The packed rows of n_seq sequences through the embedding and every block with the per-sequence kernels of the
        static prefill: what the "python" admission and the "python" scoring share.  ``keep_kv(l, b, kv_rows)`` /
        ``keep_ckv(l, b, ckv_rows)`` are called right behind sequence b's self-attention / before its cross-attention
        with its K | V rows of layer l (the admission copies them to the slot).  Returns h [R, E] f32."""
        E, H, dev, n_seq = self.E, self.H, self.dev, len(lens)
        R, Rc = sum(lens), sum(clens)
        wte, wpe = self._f("__wte_pad"), self._f("transformer.wpe.weight")
        h = torch.empty(R, E, dtype=torch.float32, device=dev)
        cap = torch.empty(Rc, E, dtype=torch.bfloat16, device=dev)
        rows = [slice(q0[b], q0[b] + lens[b]) for b in range(n_seq)]
        crows = [slice(c0[b], c0[b] + clens[b]) for b in range(n_seq)]
        for b in range(n_seq):
            ids, cids = ids_l[b].view(1, -1), cap_l[b].view(1, -1)
            v, a = (vis[b:b + 1], aud[b:b + 1]) if has[b] else (None, None)
            h[rows[b]], _ = ops.embed_fwd(ids, tt_l[b].view(1, -1), ids, wte, wpe, v, a)
            _, cap[crows[b]] = ops.embed_fwd(cids, None, cids, wte, wpe)
        def self_attn(l, qkv):
            a = torch.empty(R, E, dtype=torch.bfloat16, device=dev)
            for b, r in enumerate(rows):
                ops.attn_fwd(qkv[r, :E], qkv[r, E:2 * E], qkv[r, 2 * E:], 1, H, lens[b], lens[b], True, o=a[r])
                if keep_kv is not None:
                    keep_kv(l, b, qkv[r, E:])
            return a

        def cross_attn(l, q):   # the captions' K | V of this layer, to the slots and under the queries
            ckv = self._gemm(cap, f"transformer.h.{l}.crossattention.c_attn", Rc, 2 * E, E, out_dtype=torch.bfloat16,
                             epilogue=L.EPI_BIAS)
            a = torch.empty(R, E, dtype=torch.bfloat16, device=dev)
            for b, (r, cr) in enumerate(zip(rows, crows)):
                if keep_ckv is not None:
                    keep_ckv(l, b, ckv[cr])
                ops.attn_fwd(q[r], ckv[cr, :E], ckv[cr, E:], 1, H, lens[b], clens[b], False, o=a[r])
            return a

        for l in range(self.L):
            self._block(l, h, R, self_attn, cross_attn)
        return h

    def _admit_python(self, slots, ids_l, tt_l, cap_l, lens, clens, q0, c0, max_new, rids, vis, aud, has) -> None:
        dev, n_seq = self.dev, len(slots)

        def keep_kv(l, b, kv_rows):
            self.kv[l][slots[b], :lens[b]].copy_(kv_rows)

        def keep_ckv(l, b, ckv_rows):
            self.xkv[l][slots[b], :clens[b]].copy_(ckv_rows)

        h = self._packed_python(ids_l, tt_l, cap_l, lens, clens, q0, c0, vis, aud, has, keep_kv, keep_ckv)
        last = torch.tensor([q0[b] + lens[b] - 1 for b in range(n_seq)], device=dev)
        sl = torch.tensor(slots, device=dev)
        self._logits[sl] = self._head(h.index_select(0, last))
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        self.lens[sl] = i32(lens)
        self.cap_lens[sl] = i32(clens)
        self.stop_lens[sl] = i32([n + k for n, k in zip(lens, max_new)])
        self.row_ids[sl] = i32([_u32_as_i32(r) for r in rids])
        self.row_steps[sl] = 0
        self.finished[sl] = 0

    def _admit_native(self, slots, ids_l, tt_l, cap_l, lens, clens, q0, c0, max_new, rids, vis, aud, has) -> None:
        dev, n_seq = self.dev, len(slots)
        meta = torch.tensor([slots, q0, lens, c0, clens, max_new, [_u32_as_i32(r) for r in rids],
                             [a + n - 1 for a, n in zip(q0, lens)], [1] * n_seq, list(range(n_seq))],
                            dtype=torch.int32).to(dev)
        ids = torch.cat(ids_l).to(device=dev, dtype=torch.int64)
        tt = torch.cat(tt_l).to(device=dev, dtype=torch.int64)
        cids = torch.cat(cap_l).to(device=dev, dtype=torch.int64)
        flags = None if vis is None else torch.tensor(has, dtype=torch.uint8).to(dev)
        arr = lambda v: (C.c_int * n_seq)(*v)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        L.call("ergm_decode_admit", self._plan, n_seq, arr(slots), arr(lens), arr(clens), arr(max_new), p(meta), p(ids), p(tt),
               p(cids), p(vis), p(aud), p(flags), p(self._admit_ws), self._admit_ws.numel(), self._stream())

    # ---- scoring: what the model thinks of tokens it is handed ---------------------------------------------------
    def score_launches(self, n_seq: int, rows: int, cap_rows: int) -> int:
        """Kernel launches of one native scoring call of these sizes (ergm_decode_score_launches)."""
        if self._plan is None:
            raise ValueError("the python engine has no executor plan")
        n = L.load().ergm_decode_score_launches(self._plan, n_seq, rows, cap_rows)
        if n < 0:
            L.check(n, "ergm_decode_score_launches")
        return n

    @torch.no_grad()
    def score(self, sequences, first=None) -> List["SequenceScore"]:
        """Teacher-forced scoring: for every sequence (a prompt tuple whose ``input_ids`` already hold the response) the
        log-probability the model gives token s, s = first[b] .. n_b - 1, after the tokens before it, and the token it
        would have preferred there.  ``first[b]`` in [1, n_b) defaults to 1.  The sequences are grouped in order under
        ``max_admit`` / ``max_admit_tokens`` as the scheduler groups admissions; a group is one call and one read-back.
        No slot, cache or length is touched: live and parked requests go on as if the call had not been made.
        "native" / "fused": ergm_decode_score (no logits are written); "python": the per-sequence kernels of the
        python admission, f32 logits for the group's rows, torch.log_softmax."""
        self.m.refresh_bf16()
        n_all = len(sequences)
        first = [1] * n_all if first is None else [int(f) for f in first]
        if len(first) != n_all:
            raise ValueError("one first index per sequence")
        lens = [int(p[0].numel()) for p in sequences]
        clens = [int(p[2].numel()) for p in sequences]
        for b, (n, c, f) in enumerate(zip(lens, clens, first)):
            if c < 1:
                raise ValueError(f"sequence {b} has an empty caption")
            if n < 2 or n > self.cfg.n_positions or n > self.sched.max_admit_tokens or c > self.cap_max:
                raise ValueError(f"sequence {b} ({n} tokens, {c} caption tokens) fits no scoring group (2 <= tokens <= "
                                 f"min(n_positions {self.cfg.n_positions}, max_admit_tokens {self.sched.max_admit_tokens}), "
                                 f"cap_max {self.cap_max})")
            if not 1 <= f < n:
                raise ValueError(f"first[{b}] = {f} outside [1, {n})")
        out: List[SequenceScore] = []
        for lo, hi in score_groups(lens, self.sched.max_admit, self.sched.max_admit_tokens):
            grp, g_lens, g_first = sequences[lo:hi], lens[lo:hi], first[lo:hi]
            targets = score_targets([p[0].reshape(-1).tolist() for p in grp], g_first)
            run = self._score_python if self.engine == "python" else self._score_native
            lp, t1 = run(grp, g_lens, clens[lo:hi], torch.tensor(targets, dtype=torch.int64).to(self.dev))
            lp, t1 = lp.tolist(), t1.tolist()
            q = 0
            for n, f in zip(g_lens, g_first):
                out.append(SequenceScore(lp[q + f - 1:q + n - 1], t1[q + f - 1:q + n - 1]))
                q += n
        return out

    def _score_python(self, grp, lens, clens, targets):
        """(logprob, top1) of the group's R packed rows on the CPU, unscored rows 0: the yardstick."""
        n_seq, V = len(grp), self.m.layout.vocab
        q0 = [sum(lens[:b]) for b in range(n_seq)]
        c0 = [sum(clens[:b]) for b in range(n_seq)]
        vis, aud, has = self._features(grp)
        h = self._packed_python([p[0].reshape(-1) for p in grp], [p[1].reshape(-1) for p in grp],
                                [p[2].reshape(-1) for p in grp], lens, clens, q0, c0, vis, aud, has)
        logits = self._head(h)[:, :V]
        lsm = torch.log_softmax(logits, dim=-1)
        valid = (targets >= 0) & (targets < V)
        lp = lsm.gather(1, targets.clamp(0, V - 1)[:, None])[:, 0]
        lp = torch.where(valid, lp, torch.zeros_like(lp))
        return lp.cpu(), logits.argmax(-1).cpu()

    def _score_native(self, grp, lens, clens, targets):
        dev, n_seq, R = self.dev, len(grp), sum(lens)
        if self._score_ws is None:
            rows = min(self.sched.max_admit_tokens, self.max_batch * self.cfg.n_positions)
            need = L.load().ergm_decode_score_workspace_size(C.byref(self._plan_dims), rows, self.sched.max_admit * self.cap_max)
            if need == 0:
                raise ValueError("the decode executor cannot score with this model's dimensions")
            self._score_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        q0 = [sum(lens[:b]) for b in range(n_seq)]
        c0 = [sum(clens[:b]) for b in range(n_seq)]
        zero = [0] * n_seq
        meta = torch.tensor([zero, q0, lens, c0, clens, zero, zero, [a + n - 1 for a, n in zip(q0, lens)], [1] * n_seq,
                             list(range(n_seq))], dtype=torch.int32).to(dev)
        cat = lambda i: torch.cat([p[i].reshape(-1) for p in grp]).to(device=dev, dtype=torch.int64)
        ids, tt, cids = cat(0), cat(1), cat(2)
        vis, aud, has = self._features(grp)
        flags = None if vis is None else torch.tensor(has, dtype=torch.uint8).to(dev)
        out = torch.empty(2, R, dtype=torch.int32, device=dev)   # logprob (f32 bits) | top1: one read-back
        arr = lambda v: (C.c_int * n_seq)(*v)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        L.call("ergm_decode_score", self._plan, n_seq, arr(lens), arr(clens), p(meta), p(ids), p(tt), p(cids), p(vis), p(aud),
               p(flags), p(targets), p(out[0]), p(out[1]), p(self._score_ws), self._score_ws.numel(), self._stream())
        host = out.cpu()
        return host[0].view(torch.float32), host[1]

    # ---- extension: more than one token behind a cache that holds a past -------------------------------------
    @torch.no_grad()
    def extend(self, slots, turns, max_new_tokens=None, past=None, sampling=None) -> None:
        """Append the tokens of ``turns`` (one (input_ids, token_type_ids) per slot) behind what the occupied ``slots``
        hold, and leave the logits after each turn's last token in the slot (low level; ``extend_request`` / ``run``
        do this through the scheduler).  The captions, the request ids and the draw counters stay those of the
        admission.  max_new_tokens: one bound per turn (default: to the end of the cache).  past: the rows each slot
        holds; None reads them from ``lens`` (one sync).  A slot's first two positions belong to its admission (they
        may carry the visual / audio vectors), so every past is at least 2.  sampling (``controls=True``): one
        ``SamplingParams`` or None per turn; None keeps the slot's, without a minimum length.  The turn's ids join the
        slot's bitmap: the penalty covers everything the cache holds."""
        self.m.refresh_bf16()
        n_seq = len(turns)
        slots = [int(s) for s in slots]
        if len(slots) != n_seq or n_seq < 1:
            raise ValueError("extend takes one slot per turn")
        if len(set(slots)) != n_seq or min(slots) < 0 or max(slots) >= self.max_batch:
            raise ValueError(f"slots {slots}: outside [0, {self.max_batch}) or named twice")
        ids_l = [t[0].reshape(-1) for t in turns]
        tt_l = [t[1].reshape(-1) for t in turns]
        lens = [int(t.numel()) for t in ids_l]
        if past is None:
            host = self.lens.cpu().tolist()
            past = [host[s] for s in slots]
        past = [int(x) for x in past]
        max_new = ([self.max_len - p - n for p, n in zip(past, lens)] if max_new_tokens is None
                   else [int(x) for x in max_new_tokens])
        clens = [self._cap_host[s] for s in slots]
        if not (n_seq == len(past) == len(max_new)):
            raise ValueError("extend takes one past and one bound per turn")
        for tt, n, p, c, k in zip(tt_l, lens, past, clens, max_new):
            if n < 1 or tt.numel() != n or p < 2 or c < 1 or k < 1 or p + n + k > self.max_len:
                raise ValueError(f"a turn of {n} tokens ({tt.numel()} token types) behind {p} rows with {k} new tokens "
                                 f"does not fit max_len {self.max_len}, or its slot was never admitted")
        if sum(lens) > self.sched.max_admit_tokens or n_seq > self.sched.max_admit:
            raise ValueError("more sequences or packed rows than one extension takes (max_admit, max_admit_tokens)")
        sps = self._resolve(sampling, n_seq, max_new, slots)
        q0 = [sum(lens[:b]) for b in range(n_seq)]
        dev = self.dev
        ids = torch.cat(ids_l).to(device=dev, dtype=torch.int64)
        tt = torch.cat(tt_l).to(device=dev, dtype=torch.int64)
        pos = torch.tensor([p + s for p, n in zip(past, lens) for s in range(n)], dtype=torch.int32).to(dev)
        self.extend_calls += 1
        if self.engine == "python":
            self._extend_python(slots, ids, tt, pos, lens, past, clens, q0, max_new)
        else:
            self._extend_native(slots, ids, tt, pos, lens, past, clens, q0, max_new)
        if sps is not None:
            self._set_controls(slots, sps, ids, q0, lens, reset=False, past=past, segs=ids_l)

    def _extend_python(self, slots, ids, tt, pos, lens, past, clens, q0, max_new) -> None:
        """The yardstick: the row-wise kernels over the packed rows, the K | V rows copied by torch, and the attention
        sequence by sequence through ergm_attn_fwd over the whole sequence (queries zero below ``past``, only the rows
        from ``past`` kept), so that nothing here runs the extension's own kernels."""
        E, H, dev, n_seq = self.E, self.H, self.dev, len(slots)
        R = sum(lens)
        h = ops.embed_rows(ids, tt, pos, self._f("__wte_pad"), self._f("transformer.wpe.weight"))
        rows = [slice(q0[b], q0[b] + lens[b]) for b in range(n_seq)]
        def self_attn(l, qkv):
            a = torch.empty(R, E, dtype=torch.bfloat16, device=dev)
            for b, r in enumerate(rows):
                n_all = past[b] + lens[b]
                self.kv[l][slots[b], past[b]:n_all].copy_(qkv[r, E:])
                qf = torch.zeros(n_all, E, dtype=torch.bfloat16, device=dev)
                qf[past[b]:] = qkv[r, :E]
                kvb = self.kv[l][slots[b], :n_all]
                ob, _ = ops.attn_fwd(qf, kvb[:, :E], kvb[:, E:], 1, H, n_all, n_all, True)
                a[r] = ob[past[b]:]
            return a

        def cross_attn(l, q):
            a = torch.empty(R, E, dtype=torch.bfloat16, device=dev)
            for b, r in enumerate(rows):
                kvb = self.xkv[l][slots[b], :clens[b]]
                ops.attn_fwd(q[r], kvb[:, :E], kvb[:, E:], 1, H, lens[b], clens[b], False, o=a[r])
            return a

        for l in range(self.L):
            self._block(l, h, R, self_attn, cross_attn)
        last = torch.tensor([q0[b] + lens[b] - 1 for b in range(n_seq)], device=dev)
        sl = torch.tensor(slots, device=dev)
        self._logits[sl] = self._head(h.index_select(0, last))
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        self.lens[sl] = i32([p_ + n for p_, n in zip(past, lens)])
        self.stop_lens[sl] = i32([p_ + n + k for p_, n, k in zip(past, lens, max_new)])
        self.finished[sl] = 0

    def _extend_native(self, slots, ids, tt, pos, lens, past, clens, q0, max_new) -> None:
        n_seq = len(slots)
        meta = torch.tensor([slots, q0, lens, past, [s * self.max_len for s in slots], [p + n for p, n in zip(past, lens)],
                             [s * self.cap_max for s in slots], clens, max_new, [a + n - 1 for a, n in zip(q0, lens)],
                             [1] * n_seq, list(range(n_seq))], dtype=torch.int32).to(self.dev)
        assert meta.shape[0] == L.EXTEND_META_ROWS
        arr = lambda v: (C.c_int * n_seq)(*v)
        p = lambda t: C.c_void_p(t.data_ptr())
        L.call("ergm_decode_extend", self._plan, n_seq, arr(slots), arr(past), arr(lens), arr(clens), arr(max_new), p(meta),
               p(ids), p(tt), p(pos), p(self._admit_ws), self._admit_ws.numel(), self._stream())

    # ---- decode -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, tokens: torch.Tensor, token_types: torch.Tensor) -> torch.Tensor:
        """Append one token per slot (int64 [max_batch] on the device; what an idle or finished slot gets does not
        matter) and return the logits [max_batch, V].  A live row's length and draw counter advance by one, and it
        finishes when it reaches the bound of its admission."""
        B = self.max_batch
        tokens, token_types = tokens.reshape(-1), token_types.reshape(-1)
        if tokens.numel() != B or token_types.numel() != B:
            raise ValueError(f"step takes one token and one token type per slot ({B})")
        if tokens.dtype != torch.int64 or token_types.dtype != torch.int64 or not (tokens.is_cuda and token_types.is_cuda):
            raise ValueError("step takes int64 GPU tensors")
        if self.engine != "python":
            tokens, token_types = tokens.contiguous(), token_types.contiguous()
            L.call("ergm_decode_step_slots", self._plan, C.c_void_p(tokens.data_ptr()),
                   C.c_void_p(token_types.data_ptr()), self._stream())
            return self.logits
        lens = self.lens
        self._logits.copy_(self._step_rows(tokens, token_types, lens, self.cap_lens, self.kv, self.xkv))
        live = self.finished == 0
        lens.add_(live.to(torch.int32))
        self.row_steps.add_(live.to(torch.int32))
        self.finished.logical_or_(live & (lens >= self.stop_lens))
        return self.logits

    @torch.no_grad()
    def run_chunk(self, n: int):
        """n rounds of ergm_topp_sample_rows (``controls``: ergm_sample_rows) + one step over every slot; one read of
        the tokens and flags, and of the log-probabilities when a slot keeps them."""
        self._no_beams("run_chunk")
        top_p, eos_id, sp2_id, seed = self._sampling
        B = self.max_batch
        out = torch.empty(n, B, dtype=torch.int64, device=self.dev)
        lp = None
        if self.controls and any(a is not None for a in self._lp_acc):
            lp = torch.zeros(n, B, dtype=torch.float32, device=self.dev)
        ruled = self.controls and any(self._rule_live)   # some live request carries a logit rule
        if self.engine != "python":
            if self.controls and ruled != self._rules_bound:
                L.call("ergm_decode_set_rules", self._plan, C.byref(self._rules) if ruled else None)
                self._rules_bound = ruled
            if self.controls:
                L.call("ergm_decode_run_slots_sampled", self._plan, n, float(top_p), C.byref(self._ctl), seed & (2 ** 64 - 1),
                       eos_id, sp2_id, C.c_void_p(out.data_ptr()), None if lp is None else C.c_void_p(lp.data_ptr()),
                       self._stream())
            else:
                L.call("ergm_decode_run_slots", self._plan, n, float(top_p), seed & (2 ** 64 - 1), eos_id, sp2_id,
                       C.c_void_p(out.data_ptr()), self._stream())
        else:
            tt = torch.full((B,), sp2_id, dtype=torch.int64, device=self.dev)
            V = self.m.layout.vocab
            for i in range(n):
                if self.controls:
                    if ruled:
                        ops.logit_rules(self._logits, V, self._rules, self.lens, eos_id, self.max_len, finished=self.finished)
                    ops.sample_rows(self._logits, V, top_p, seed, self.row_ids, self.row_steps, eos_id, ctl=self._ctl,
                                    finished=self.finished, tokens=out[i], logprob=None if lp is None else lp[i])
                    if ruled:
                        ops.hist_append(out[i], self.lens, self.hist, self.max_len, finished=self.finished)
                else:
                    ops.topp_sample_rows(self._logits, V, top_p, seed, self.row_ids, self.row_steps, eos_id,
                                         finished=self.finished, tokens=out[i])
                self.step(out[i], tt)
        parts = [out.reshape(-1), self.finished.to(torch.int64)]
        if lp is not None:   # the f32 bits ride along in the one copy
            parts.append(lp.view(torch.int32).reshape(-1).to(torch.int64))
        both = torch.cat(parts).cpu()
        if lp is not None:
            rows = both[n * B + B:].to(torch.int32).view(torch.float32).view(n, B).tolist()
            for s, acc in enumerate(self._lp_acc):
                if acc is not None:
                    acc.extend(row[s] for row in rows)
        return both[:n * B].view(n, B).tolist(), both[n * B:n * B + B].tolist()

    def admit_requests(self, slots, requests) -> None:
        if self.num_beams is not None:   # the scheduler's slots are groups
            self.admit_beams(slots, [r.payload for r in requests], [r.max_new for r in requests], [r.id for r in requests],
                             [r.sampling for r in requests])
            return
        self.admit(slots, [r.payload for r in requests], [r.max_new for r in requests], [r.id for r in requests],
                   [r.sampling for r in requests] if self.controls else None)

    def extend_requests(self, slots, requests) -> None:
        self.extend(slots, [r.payload for r in requests], [r.max_new for r in requests], [r.past for r in requests],
                    [r.sampling for r in requests] if self.controls else None)

    def retire(self, slot: int, request) -> None:
        if self.num_beams is not None:   # slot is the group: its rows hold no live length and no live rule any more
            self._grp_rows[slot] = 0
            for r in range(slot * self.num_beams, (slot + 1) * self.num_beams):
                self._rule_live[r] = False
            return
        if self.keep_logits:
            self.final_logits[request.id] = self.logits[slot].clone()
        if self.controls and self._lp_acc[slot] is not None:   # the chunk ran on past the request's last token
            self.token_logprobs[request.id] = self._lp_acc[slot][:len(request.tokens)]
            self._lp_acc[slot] = None
        if self.controls:   # an eos that was drawn is never stepped into the cache, nor into the history
            toks = request.tokens
            self._hist_host[slot].append(toks[:-1] if toks and toks[-1] == self._sampling[1] else list(toks))
            self._rule_live[slot] = False

    # ---- requests -----------------------------------------------------------------------------------------
    def check_sampling(self, sampling) -> None:
        """ValueError for what this generator cannot serve: any ``sampling`` without ``controls=True``, bad words that do
        not fit a pool row of ``bad_words_cap`` entries, a rule with a cache longer than the 1,024 positions the rule
        kernel stages.  The scheduler calls it at ``submit`` / ``extend``, the low-level ``admit`` / ``extend`` too."""
        if sampling is not None and not self.controls and getattr(self, "num_beams", None) is None:
            raise ValueError("sampling parameters need ContinuousGenerator(controls=True)")
        if sampling is not None and not isinstance(sampling, SamplingParams):
            raise ValueError("sampling must be a SamplingParams")
        if sampling is not None and sampling.has_rules:
            pack_bad_words(sampling.bad_words_ids, self.bad_words_cap)
            if self.max_len > 1024:
                raise ValueError(f"logit rules need max_len <= 1024 (it is {self.max_len})")

    def submit(self, prompt, max_new_tokens: Optional[int] = None, request_id: Optional[int] = None,
               keep: bool = False, sampling: Optional[SamplingParams] = None, no_repeat_ngram_size: int = 0,
               no_repeat_scope: str = "sequence", bad_words_ids=()) -> int:
        """Queue a prompt; returns its id (uint32; arrival order unless given).  ``keep``: the request keeps its slot
        and its cache when it ends (it is parked), so that ``extend_request`` can continue the conversation; a kept
        prompt that carries visual / audio features has at least 2 tokens (the positions the features sit at).

        Beam mode (``num_beams``): the request is served by ``run_beams`` / ``drain_beams`` in a group of ``num_beams``
        slots; ``no_repeat_ngram_size`` / ``no_repeat_scope`` / ``bad_words_ids`` (``SamplingParams`` has their meaning)
        are its logit rules, the same in all rows of its group.  ``keep`` and ``sampling`` are refused there, and the
        three rule arguments outside it (a sampled request carries its rules in ``sampling``)."""
        if self.num_beams is not None:
            if keep or sampling is not None:
                raise ValueError("beam mode has no sessions and draws nothing: keep / sampling are refused")
            bad = check_rules(no_repeat_ngram_size, no_repeat_scope, bad_words_ids)
            rules = None
            if no_repeat_ngram_size > 0 or bad:
                rules = SamplingParams(no_repeat_ngram_size=no_repeat_ngram_size, no_repeat_scope=no_repeat_scope,
                                       bad_words_ids=bad)
                self.check_sampling(rules)
            return self.sched.submit(int(prompt[0].numel()), int(prompt[2].numel()), max_new_tokens, request_id, prompt,
                                     False, sampling=rules)
        if no_repeat_ngram_size or bad_words_ids or no_repeat_scope != "sequence":
            raise ValueError("a sampled request carries its logit rules in sampling=SamplingParams(...)")
        if keep and prompt[3] is not None and int(prompt[0].numel()) < 2:
            raise ValueError("a kept prompt with visual / audio features needs at least 2 tokens")
        self.check_sampling(sampling)
        return self.sched.submit(int(prompt[0].numel()), int(prompt[2].numel()), max_new_tokens, request_id, prompt, keep,
                                 sampling=sampling)

    def extend_request(self, request_id: int, ids, token_types, max_new_tokens: Optional[int] = None,
                       keep: bool = True, sampling: Optional[SamplingParams] = None) -> int:
        """Queue the next turn of a parked request: ``ids`` / ``token_types`` are appended behind what its cache holds
        (the tokens of the earlier turns; an eos the model drew is not among them, so a turn that wants it as a
        separator begins with it), and up to max_new_tokens are generated behind them at the next ``run`` / ``drain``,
        returned under the same id.  Raises ValueError when the id is not parked, the turn is empty or longer than
        max_admit_tokens, or the cache has no room for it and one new token.  ``sampling`` (``controls=True``): None
        keeps the session's values, except that the new turn has no minimum length."""
        self._no_beams("extend_request")
        ids, token_types = ids.reshape(-1), token_types.reshape(-1)
        if ids.numel() != token_types.numel():
            raise ValueError("one token type per token")
        self.check_sampling(sampling)
        return self.sched.extend(request_id, int(ids.numel()), max_new_tokens, (ids, token_types), keep, sampling=sampling)

    def release(self, request_id: int) -> None:
        """Free the slot of a parked request, or forget a stored one."""
        self.sched.release(request_id)

    # ---- the session store: parked conversations leave their slots (session_store=True) --------------------------
    def _need_store(self, what: str) -> None:
        if not self.session_store:
            raise ValueError(f"{what} needs ContinuousGenerator(session_store=True)")

    def _sessions(self) -> "ops.SessionState":
        """The bound buffers as ergm_session_state, built once."""
        if self._session_state is None:
            self._session_state = ops.SessionState(
                self.kv, self.xkv, self.lens, self.cap_lens, self.stop_lens, self.finished, self.row_ids, self.row_steps,
                ctl=self._ctl if self.controls else None, rules=self._rules if self.controls else None,
                max_len=self.max_len, cap_max=self.cap_max)
        return self._session_state

    def _slot_flags(self, slot: int) -> int:
        """The sections the session in ``slot`` takes along: its controls, and its rule state when it carries a rule."""
        if not self.controls:
            return 0
        return L.SESSION_CTL | (L.SESSION_RULES if self._slot_ruled[slot] else 0)

    def session_bytes(self, slot: int, rows: int, c: int) -> int:
        """The size of the blob the session parked in ``slot`` with ``rows`` cache rows and ``c`` caption rows packs into."""
        return self._sessions().bytes(rows, c, self._slot_flags(slot))

    @property
    def stored_bytes(self) -> int:
        """The bytes of HBM the stored sessions hold; a fork shares its origin's blob."""
        return sum(b.numel() for b in {id(r.blob): r.blob for r in self._store.values()}.values())

    def _check_slots(self, slots, what: str) -> List[int]:
        slots = [int(s) for s in slots]
        if not slots or len(set(slots)) != len(slots) or min(slots) < 0 or max(slots) >= self.max_batch:
            raise ValueError(f"{what}: slots {slots}: none, outside [0, {self.max_batch}) or named twice")
        return slots

    @torch.no_grad()
    def save_sessions(self, slots, ids, rows=None, cap_rows=None) -> None:
        """Pack the sessions parked in ``slots`` away under ``ids``, one blob in HBM each (the layout: ergm_hip.h,
        "Session store"), and leave the slots idle and their host records as a new tenant finds them.  ``rows`` /
        ``cap_rows``: the rows each slot holds (default: the scheduler's record of the parked ids).  "native" /
        "fused": ergm_slots_save, 3 launches whatever the number of sessions; "python": the same bytes by torch slicing."""
        self._need_store("save_sessions")
        slots, ids = self._check_slots(slots, "save_sessions"), [int(i) for i in ids]
        if rows is None or cap_rows is None:
            for s, i in zip(slots, ids):
                if i not in self.sched.parked or self.sched.parked[i][0] != s:
                    raise ValueError(f"save_sessions: request id {i} is not parked in slot {s}")
            rows, cap_rows = [self.sched.parked[i][1] for i in ids], [self.sched.parked[i][2] for i in ids]
        rows, cap_rows = [int(n) for n in rows], [int(c) for c in cap_rows]
        if not (len(slots) == len(ids) == len(rows) == len(cap_rows)) or len(set(ids)) != len(ids):
            raise ValueError("save_sessions takes one distinct id, one row count and one caption row count per slot")
        for i, n, c in zip(ids, rows, cap_rows):
            if i in self._store:
                raise ValueError(f"save_sessions: session id {i} is stored already")
            if not (1 <= n <= self.max_len and 1 <= c <= self.cap_max):
                raise ValueError(f"save_sessions: {n} rows / {c} caption rows outside [1, max_len {self.max_len}] / "
                                 f"[1, cap_max {self.cap_max}]")
        st = self._sessions()
        flags = [self._slot_flags(s) for s in slots]
        if self.engine == "python":
            blobs = [self._pack_python(s, n, c, f) for s, n, c, f in zip(slots, rows, cap_rows, flags)]
        else:
            blobs = ops.slots_save(st, slots, rows, cap_rows, flags)
        self.save_calls += 1
        for s, i, n, c, f, blob in zip(slots, ids, rows, cap_rows, flags, blobs):
            rec = _StoredSession(blob, st.header(n, c, f), self._rid_host[s], self._cap_host[s])
            self._cap_host[s] = 0
            if self.controls:
                rec.sp, rec.hist_host, rec.ruled = self._slot_sp[s], self._hist_host[s], self._slot_ruled[s]
                self._slot_sp[s], self._hist_host[s], self._lp_acc[s] = None, [], None
                self._slot_ruled[s] = self._rule_live[s] = False
            self._store[i] = rec

    @torch.no_grad()
    def load_sessions(self, slots, ids) -> None:
        """Unpack the stored sessions ``ids`` into the free ``slots`` and leave them parked there (lens = stop_lens = the
        rows, finished), with their host records; the stored copies stay until ``drop_session``.  A fork is loaded under
        its own id, so its draws differ from its origin's."""
        self._need_store("load_sessions")
        slots, ids = self._check_slots(slots, "load_sessions"), [int(i) for i in ids]
        if len(ids) != len(slots) or any(i not in self._store for i in ids):
            raise ValueError(f"load_sessions: one stored id per slot (ids {ids}, stored {sorted(self._store)})")
        recs = [self._store[i] for i in ids]
        if self.engine == "python":
            for s, rec in zip(slots, recs):
                self._unpack_python(s, rec)
        else:
            row_ids = None
            if any(rec.fork for rec in recs):
                row_ids = torch.tensor([_u32_as_i32(rec.rid) for rec in recs], dtype=torch.int32).to(self.dev)
            ops.slots_load(self._sessions(), slots, [rec.hdr for rec in recs], [rec.blob for rec in recs], row_ids)
        self.load_calls += 1
        for s, rec in zip(slots, recs):
            self._cap_host[s], self._rid_host[s] = rec.cap, rec.rid
            if self.controls:
                self._slot_sp[s], self._hist_host[s], self._slot_ruled[s] = rec.sp, list(rec.hist_host), rec.ruled
                self._rule_live[s], self._lp_acc[s] = False, None

    def drop_session(self, session_id: int) -> None:
        """Forget a stored session; its blob is freed with its last user."""
        if self._store.pop(session_id, None) is None:
            raise ValueError(f"session id {session_id} is not stored")

    def fork_session(self, session_id: int, new_id: int) -> None:
        """A second stored session ``new_id`` with the contents of ``session_id``: blobs are never written after the
        save, so both ids share one tensor; the fork draws under ``new_id``."""
        if session_id not in self._store or new_id in self._store:
            raise ValueError(f"fork_session: id {session_id} is not stored, or id {new_id} is")
        self._store[new_id] = replace(self._store[session_id], rid=int(new_id), fork=True)

    def _pack_python(self, slot: int, n: int, c: int, flags: int) -> torch.Tensor:
        """The yardstick of ergm_slots_save for one slot: the same blob, byte for byte, by torch slicing."""
        st, nl, dev = self._sessions(), self.L, self.dev
        rb, i32 = st.row_bytes, torch.int32
        up16 = lambda x: (x + 15) & ~15
        nbytes = st.bytes(n, c, flags)
        blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        words = [L.SESSION_MAGIC, 1, flags, nl, rb, n, c, 0, 0, st.ld_seen if flags & L.SESSION_CTL else 0,
                 st.bad_cap if flags & L.SESSION_RULES else 0, 0, nbytes & 0xFFFFFFFF, nbytes >> 32, 0, 0]
        hdr = blob[:64].view(i32)
        hdr.copy_(torch.tensor([_u32_as_i32(w) for w in words], dtype=i32))
        hdr[7:8].copy_(self.row_ids[slot:slot + 1])
        hdr[8:9].copy_(self.row_steps[slot:slot + 1])
        o = 64
        for caches, rows in ((self.kv, n), (self.xkv, c)):
            sec = blob[o:o + nl * rows * rb].view(caches[0].dtype).view(nl, rows, -1)
            for l in range(nl):
                sec[l].copy_(caches[l][slot, :rows])
            o += nl * rows * rb
        if flags & L.SESSION_CTL:
            w = blob[o:o + 32].view(i32)
            w[:4].copy_(self._ctl_vals[:, slot])
            w[4:5].copy_(self.min_step[slot:slot + 1])
            o += 32
            blob[o:o + 4 * st.ld_seen].view(i32).copy_(self.seen[slot])
            o += up16(4 * st.ld_seen)
        if flags & L.SESSION_RULES:
            blob[o:o + 8].view(i32).copy_(self._rule_vals[:, slot])
            o += 16
            blob[o:o + 4 * st.bad_cap].view(i32).copy_(self._bad_pool[slot])
            o += up16(4 * st.bad_cap)
            blob[o:o + 4 * n].view(i32).copy_(self.hist[slot, :n])
            o += up16(4 * n)
            self._rule_vals[:, slot] = 0   # the next tenant inherits no rule
            self._bad_pool[slot] = 0
        assert o == nbytes
        self.finished[slot] = 1
        self.lens[slot] = 0
        self.cap_lens[slot] = 0
        return blob

    def _unpack_python(self, slot: int, rec: "_StoredSession") -> None:
        """The yardstick of ergm_slots_load for one slot, by torch slicing."""
        st, nl, blob, h = self._sessions(), self.L, rec.blob, rec.hdr
        rb, i32 = st.row_bytes, torch.int32
        up16 = lambda x: (x + 15) & ~15
        n, c, flags = h.rows, h.cap_rows, h.flags
        if (h.magic, h.version, h.n_layer, h.row_bytes) != (L.SESSION_MAGIC, 1, nl, rb) or blob.numel() < st.bytes(n, c, flags):
            raise ValueError("load_sessions: the blob's header disagrees with this generator")
        hdr = blob[:64].view(i32)
        o = 64
        for caches, rows in ((self.kv, n), (self.xkv, c)):
            sec = blob[o:o + nl * rows * rb].view(caches[0].dtype).view(nl, rows, -1)
            for l in range(nl):
                caches[l][slot, :rows].copy_(sec[l])
            o += nl * rows * rb
        self.lens[slot] = n
        self.cap_lens[slot] = c
        self.stop_lens[slot] = n
        self.finished[slot] = 1
        self.row_steps[slot:slot + 1].copy_(hdr[8:9])
        if rec.fork:
            self.row_ids[slot] = _u32_as_i32(rec.rid)
        else:
            self.row_ids[slot:slot + 1].copy_(hdr[7:8])
        if flags & L.SESSION_CTL:
            w = blob[o:o + 32].view(i32)
            self._ctl_vals[:, slot] = w[:4]
            self.min_step[slot:slot + 1].copy_(w[4:5])
            o += 32
            self.seen[slot].copy_(blob[o:o + 4 * st.ld_seen].view(i32))
            o += up16(4 * st.ld_seen)
        if flags & L.SESSION_RULES:
            self._rule_vals[:, slot] = blob[o:o + 8].view(i32)
            o += 16
            self._bad_pool[slot].copy_(blob[o:o + 4 * st.bad_cap].view(i32))
            o += up16(4 * st.bad_cap)
            self.hist[slot, :n].copy_(blob[o:o + 4 * n].view(i32))
        elif self.controls:   # a session without a rule turns off what the slot's last tenant left
            self._rule_vals[:, slot] = 0
            self._bad_pool[slot] = 0

    def offload(self, request_id: int) -> None:
        """Move a parked session out of its slot into the store at once (a stored id is left as it is); the slot is
        free for the next admission.  ValueError for an id that is neither parked nor stored."""
        self._need_store("offload")
        self.sched.offload(request_id)

    def fork_request(self, request_id: int, new_id: Optional[int] = None) -> int:
        """A second session with the history of ``request_id`` (parked: it is offloaded first), returned under ``new_id``
        (default: the next id).  ``extend_request`` continues either; the fork draws under its own id."""
        self._need_store("fork_request")
        return self.sched.fork(request_id, new_id)

    def drain(self, top_p: float, eos_id: int, sp2_id: int, seed: int = 0):
        """Serve the queue, yielding (id, tokens) as each request retires."""
        self._no_beams("drain")
        self._sampling = (top_p, eos_id, sp2_id, seed)
        try:
            yield from self.sched.drain(eos_id)
        finally:
            self._sampling = None

    def run(self, top_p: float, eos_id: int, sp2_id: int, seed: int = 0) -> dict:
        """Serve the queue; returns {id: tokens}, each list ending at its first eos (included) or at its bound."""
        self._no_beams("run")
        return dict(self.drain(top_p, eos_id, sp2_id, seed))

    def generate(self, prompts, top_p: float, eos_id: int, sp2_id: int, seed: int = 0, max_new_tokens=None,
                 sampling=None) -> List[List[int]]:
        """One token list per prompt, in submission order.  max_new_tokens: None, one bound for all, or one per prompt;
        sampling (``controls=True``): None, one ``SamplingParams`` for all, or one per prompt."""
        self._no_beams("generate")
        if max_new_tokens is None or isinstance(max_new_tokens, int):
            max_new_tokens = [max_new_tokens] * len(prompts)
        if sampling is None or isinstance(sampling, SamplingParams):
            sampling = [sampling] * len(prompts)
        ids = [self.submit(p, k, sampling=sp) for p, k, sp in zip(prompts, max_new_tokens, sampling)]
        out = self.run(top_p, eos_id, sp2_id, seed)
        return [out[i] for i in ids]

    # ---- beam mode: beam search on the slots (num_beams) -----------------------------------------------------
    def _no_beams(self, what: str) -> None:
        if self.num_beams is not None:
            raise ValueError(f"{what} samples: a generator in beam mode (num_beams={self.num_beams}) serves run_beams / "
                             "drain_beams / beam_search")

    def _need_beams(self, what: str) -> int:
        if self.num_beams is None:
            raise ValueError(f"{what} needs ContinuousGenerator(num_beams=W)")
        return self.num_beams

    def _set_beam_rules(self, groups, rules, ids_l, lens) -> None:
        """The rule values of every row of the admitted groups (start, ngram, the bad-word pool row: one copy to the
        device, two scatters) and the prompts of the ruled ones in the history of row g·W (one ergm_hist_write); round
        0's ergm_hist_follow fans the history out.  An unruled group takes the values that ban nothing, so a new tenant
        inherits no rule."""
        W = self.num_beams
        rows = []
        for g, sp, n in zip(groups, rules, lens):
            if sp is None:
                vals = [0, 0] + [0] * self.bad_words_cap
            else:
                vals = [n if sp.no_repeat_scope == "turn" else 0, sp.no_repeat_ngram_size,
                        *pack_bad_words(sp.bad_words_ids, self.bad_words_cap)]
            rows += [[g * W + w] + vals for w in range(W)]
        m = torch.tensor(rows, dtype=torch.int32).to(self.dev)
        sl = m[:, 0].long()
        self._rule_vals[:, sl] = m[:, 1:3].t()
        self._bad_pool[sl] = m[:, 3:]
        ruled = [b for b, sp in enumerate(rules) if sp is not None]
        if ruled:
            q0 = [sum(lens[i] for i in ruled[:j]) for j in range(len(ruled))]
            w = torch.tensor([[groups[b] * W for b in ruled], q0, [lens[b] for b in ruled]], dtype=torch.int32).to(self.dev)
            ids = torch.cat([ids_l[b] for b in ruled]).to(device=self.dev, dtype=torch.int64)
            ops.hist_write(ids, w[0], w[1], w[2], self.hist, self.max_len)
        for g, sp in zip(groups, rules):
            for r in range(g * W, (g + 1) * W):
                self._slot_ruled[r] = self._rule_live[r] = sp is not None

    @torch.no_grad()
    def admit_beams(self, groups, prompts, max_new_tokens=None, request_ids=None, rules=None) -> None:
        """Prefill ``prompts`` into the free ``groups`` (low level; ``submit`` / ``run_beams`` do this through the
        scheduler): the admission of prompt b into slot groups[b]·W alone, then ergm_beam_seed, which copies its caption
        K | V to the group's other slots and leaves the scores [0, -inf, ...], the state round 0 starts from.
        max_new_tokens: one bound per prompt (default: to the end of the cache); rules: one ``SamplingParams`` (its
        three rule fields count) or None per prompt."""
        W = self._need_beams("admit_beams")
        groups = [int(g) for g in groups]
        n_seq = len(prompts)
        if len(groups) != n_seq or n_seq < 1:
            raise ValueError("admit_beams takes one group per prompt")
        if len(set(groups)) != n_seq or min(groups) < 0 or max(groups) >= self.n_groups:
            raise ValueError(f"groups {groups}: outside [0, {self.n_groups}) or named twice")
        rules = [None] * n_seq if rules is None else [sp if sp is not None and sp.has_rules else None for sp in rules]
        if len(rules) != n_seq:
            raise ValueError("one rules value per prompt")
        for sp in rules:
            self.check_sampling(sp)
        ids_l = [p[0].reshape(-1) for p in prompts]
        lens = [int(t.numel()) for t in ids_l]
        self.admit([g * W for g in groups], prompts, max_new_tokens, request_ids)
        if any(sp is not None for sp in rules) or any(self._slot_ruled[g * W] for g in groups):
            self._set_beam_rules(groups, rules, ids_l, lens)
        ops.beam_seed(self.xkv, groups, W, self.cap_max, self.lens, self.cap_lens, self.stop_lens, self.finished,
                      self.beam_scores)
        self.seed_calls += 1
        for g, n in zip(groups, lens):
            self._grp_rows[g] = n

    def _beam_chunk(self, n: int, eos_id: Optional[int], sp2_id: Optional[int]):
        """n rounds on the device; the tokens and parents [n, max_batch] stay there."""
        W = self._need_beams("beam_round")
        eos_id = self._beam_ids[0] if eos_id is None else eos_id
        sp2_id = self._beam_ids[1] if sp2_id is None else sp2_id
        if eos_id is None or sp2_id is None:
            raise ValueError("beam_round needs eos_id and sp2_id")
        V = self.m.layout.vocab
        if not 0 <= eos_id < V:
            raise ValueError(f"eos_id {eos_id} outside the vocabulary")
        if n < 1:
            raise ValueError(f"{n} round(s)")
        self._beam_ids = (eos_id, sp2_id)
        B, dev = self.max_batch, self.dev
        toks = torch.empty(n, B, dtype=torch.int64, device=dev)
        pars = torch.empty(n, B, dtype=torch.int32, device=dev)
        ruled = any(self._rule_live)
        bound = max(self._grp_rows)   # the host's bound on the live lengths
        if self.engine != "python":
            if ruled != self._rules_bound:
                L.call("ergm_decode_set_rules", self._plan, C.byref(self._rules) if ruled else None)
                self._rules_bound = ruled
            p = lambda t: C.c_void_p(t.data_ptr())
            L.call("ergm_decode_run_slot_beams", self._plan, n, W, bound, eos_id, sp2_id, p(self.beam_scores), p(toks), p(pars),
                   p(self._beam_ws), self._beam_ws.numel(), self._stream())
        else:
            tt = torch.full((B,), sp2_id, dtype=torch.int64, device=dev)
            for i in range(n):
                if ruled:
                    ops.logit_rules(self._logits, V, self._rules, self.lens, eos_id, self.max_len, finished=self.finished)
                ops.beam_select(self._logits, V, W, self.beam_scores, self.finished, eos_id, parent=pars[i], token=toks[i],
                                ws=self._beam_ws)
                ops.beam_gather(self.kv, pars[i], self.lens, W, max_len=max(1, min(bound + i, self.max_len)))
                if ruled:
                    ops.hist_follow(self.hist, pars[i], self.lens, W, self.max_len)
                    ops.hist_append(toks[i], self.lens, self.hist, self.max_len, finished=self.finished)
                self.step(toks[i], tt)
        self._grp_rows = [min(r + n, self.max_len) if r else 0 for r in self._grp_rows]
        return toks, pars

    @torch.no_grad()
    def beam_round(self, n: int, eos_id: Optional[int] = None, sp2_id: Optional[int] = None):
        """n rounds of select, gather, step over every slot (low level).  Returns ``(tokens, parents)``: n lists over
        the max_batch rows, read back once; the scores and flags stay on the device (``beam_scores``, ``finished``)."""
        toks, pars = self._beam_chunk(n, eos_id, sp2_id)
        return toks.cpu().tolist(), pars.cpu().tolist()

    @torch.no_grad()
    def run_beam_chunk(self, n: int):
        """The scheduler's chunk: n rounds, then one read of the tokens, parents, flags and scores."""
        toks, pars = self._beam_chunk(n, None, None)
        B = self.max_batch
        both = torch.cat([toks.reshape(-1), pars.reshape(-1).to(torch.int64), self.finished.to(torch.int64),
                          self.beam_scores.view(torch.int32).to(torch.int64)]).cpu()
        scores = both[2 * n * B + B:].to(torch.int32).view(torch.float32).tolist()
        return (both[:n * B].view(n, B).tolist(), both[n * B:2 * n * B].view(n, B).tolist(),
                both[2 * n * B:2 * n * B + B].tolist(), scores)

    def drain_beams(self, eos_id: int, sp2_id: int, length_penalty: float = 1.0, num_return: int = 1):
        """Serve the queue by beam search, yielding (id, [(tokens, sum_logprob), ...]) as each group retires."""
        self._need_beams("drain_beams")
        if not 0 <= eos_id < self.m.layout.vocab:
            raise ValueError(f"eos_id {eos_id} outside the vocabulary")
        self._beam_ids = (eos_id, sp2_id)
        return self.sched.drain(eos_id, length_penalty, num_return)

    def run_beams(self, eos_id: int, sp2_id: int, length_penalty: float = 1.0, num_return: int = 1) -> dict:
        """Serve the queue by beam search; returns {id: [(tokens, sum_logprob), ...]}: ``num_return`` hypotheses per
        request, best first by ``sum_logprob / len(tokens) ** length_penalty`` (``beam_backtrack``), each ending at its
        first eos (included) or at the request's ``max_new_tokens``.  The device ranks by the raw sum."""
        return dict(self.drain_beams(eos_id, sp2_id, length_penalty, num_return))

    def beam_search(self, prompts, eos_id: int, sp2_id: int, max_new_tokens=None, length_penalty: float = 1.0,
                    num_return: int = 1, no_repeat_ngram_size: int = 0, no_repeat_scope: str = "sequence",
                    bad_words_ids=()) -> list:
        """One hypothesis list per prompt, in submission order.  max_new_tokens: None, one bound for all, or one per
        prompt; the rule arguments hold for every prompt."""
        self._need_beams("beam_search")
        if max_new_tokens is None or isinstance(max_new_tokens, int):
            max_new_tokens = [max_new_tokens] * len(prompts)
        ids = [self.submit(p, k, no_repeat_ngram_size=no_repeat_ngram_size, no_repeat_scope=no_repeat_scope,
                           bad_words_ids=bad_words_ids) for p, k in zip(prompts, max_new_tokens)]
        out = self.run_beams(eos_id, sp2_id, length_penalty, num_return)
        return [out[i] for i in ids]
