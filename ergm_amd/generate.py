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
"""
from __future__ import annotations

import ctypes as C
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
    reads them); ``step`` appends one token per sequence; ``generate`` is nucleus sampling of the whole batch.

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

    def _bind_plan(self, Sc: int) -> None:
        """(Re)create the executor plan when the captions outgrow it, then bind the state the prefill left."""
        lib, lay = L.load(), self.m.layout
        if self._plan is None or Sc > self._cap_max:
            self._drop_plan()
            self._cap_max = max(Sc, self.max_len)
            dims = L.DecodeDims(vocab=lay.vocab, vocab_pad=lay.vocab_pad, n_embd=self.E, n_layer=self.L, n_head=self.H,
                                n_inner=self.F, n_positions=self.cfg.n_positions, max_batch=self.max_batch,
                                max_len=self.max_len, cap_max=self._cap_max, eps=self.cfg.layer_norm_epsilon)
            prm = L.ModelParams()
            prm.wte, prm.wte_b = self._f("__wte_pad").data_ptr(), self._b("__wte_pad").data_ptr()
            prm.wpe = self._f("transformer.wpe.weight").data_ptr()
            prm.ln_f_w = self._f("transformer.ln_f.weight").data_ptr()
            prm.ln_f_b = self._f("transformer.ln_f.bias").data_ptr()
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
            L.call("ergm_decode_set_engine", self._plan, self.ENGINES[self.engine])
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

    def _head(self, h_last: torch.Tensor) -> torch.Tensor:
        """Rows [B, E] -> logits [B, vocab_pad] f32 (the first ``vocab`` columns count)."""
        x = self._ln(h_last, "transformer.ln_f")
        lay = self.m.layout
        return ops.gemm(x, self._b("__wte_pad"), x.shape[0], lay.vocab_pad, self.E, L.MK, L.NK, out_dtype=torch.float32)

    @torch.no_grad()
    def prefill(self, prompts) -> torch.Tensor:
        """prompts: a list of (input_ids, token_type_ids, caption_ids, imgs, auds) per sequence (1-D or [1, S] id
        tensors of any lengths; imgs / auds may be None).  Returns the next-token logits [B, V] (fp32)."""
        self.m.refresh_bf16()
        B = len(prompts)
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"{B} prompts for max_batch {self.max_batch}")
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
        Fd = self.m.layout.Fd
        has = [p[3] is not None for p in prompts]
        vis = aud = None
        if any(has):   # sequences without features add zeros
            vis = torch.zeros(B, Fd, dtype=torch.float32, device=dev)
            aud = torch.zeros(B, Fd, dtype=torch.float32, device=dev)
            for b, p in enumerate(prompts):
                if has[b]:
                    vis[b] = p[3].float().reshape(-1, Fd)[0]
                    aud[b] = p[4].float().reshape(Fd)
            if Fd != E:  # config 5: the build-side projections (Conv1D), then nothing for the rows without features
                keep = torch.tensor(has, device=dev).unsqueeze(1)
                vis, aud = (self._gemm(x.to(torch.bfloat16), f"transformer.{m}", B, E, Fd, out_dtype=torch.float32,
                                       epilogue=L.EPI_BIAS) * keep for x, m in ((vis, "visual_proj"), (aud, "audio_proj")))
        h, _ = ops.embed_fwd(ids, tt, ids, wte, wpe, vis, aud)
        _, cap = ops.embed_fwd(cap_ids, None, cap_ids, wte, wpe)
        self.xkv = [self._gemm(cap, f"transformer.h.{l}.crossattention.c_attn", B * Sc, 2 * E, E,
                               out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS).view(B, Sc, 2 * E) for l in range(self.L)]
        n = B * S
        for l in range(self.L):
            p = f"transformer.h.{l}."
            x = self._ln(h, p + "ln_1")
            qkv = self._gemm(x, p + "attn.c_attn", n, 3 * E, E, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS)
            self.kv[l][:B, :S].copy_(qkv[:, E:].view(B, S, 2 * E))
            a, _ = ops.attn_fwd(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], B, H, S, S, True)
            self._gemm(a, p + "attn.c_proj", n, E, E, out=h, epilogue=L.EPI_BIAS_RESID, aux=h)
            x = self._ln(h, p + "ln_cross_attn")
            q = self._gemm(x, p + "crossattention.q_attn", n, E, E, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS)
            a = torch.empty(n, E, dtype=torch.bfloat16, device=dev)
            for b in range(B):   # each sequence over its own caption rows: padded caption rows are never attended
                kvb = self.xkv[l][b, :clens[b]]
                ops.attn_fwd(q[b * S:(b + 1) * S], kvb[:, :E], kvb[:, E:], 1, H, S, clens[b], False,
                             o=a[b * S:(b + 1) * S])
            self._gemm(a, p + "crossattention.c_proj", n, E, E, out=h, epilogue=L.EPI_BIAS_RESID, aux=h)
            self._mlp(p, h, n)
        self.B, self.n_max = B, S
        self.lens[:B] = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.cap_lens[:B] = torch.tensor(clens, dtype=torch.int32, device=dev)
        self.finished.zero_()
        self._ws = ops.attn_decode_workspace(B, H, max(self.max_len, Sc), dev)
        last = torch.tensor([b * S + lens[b] - 1 for b in range(B)], device=dev)
        self._logits = self._head(h.index_select(0, last))
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
        B, E, dev = self.B, self.E, self.dev
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
        lens, cap_lens = self.lens[:B], self.cap_lens[:B]
        h = ops.embed_rows(tokens, token_types, lens, self._f("__wte_pad"), self._f("transformer.wpe.weight"))
        for l in range(self.L):
            p = f"transformer.h.{l}."
            x = self._ln(h, p + "ln_1")
            qkv = self._gemm(x, p + "attn.c_attn", B, 3 * E, E, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS)
            cache = self.kv[l][:B]
            a = ops.attn_decode(qkv, cache[:, :, :E], cache[:, :, E:], lens, True, ws=self._ws)
            self._gemm(a, p + "attn.c_proj", B, E, E, out=h, epilogue=L.EPI_BIAS_RESID, aux=h)
            x = self._ln(h, p + "ln_cross_attn")
            q = self._gemm(x, p + "crossattention.q_attn", B, E, E, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS)
            xkv = self.xkv[l]
            a = ops.attn_decode(q, xkv[:, :, :E], xkv[:, :, E:], cap_lens, False, ws=self._ws)
            self._gemm(a, p + "crossattention.c_proj", B, E, E, out=h, epilogue=L.EPI_BIAS_RESID, aux=h)
            self._mlp(p, h, B)
        self._logits = self._head(h)
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
