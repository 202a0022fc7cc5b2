"""Tensor-level wrappers over the C-ABI kernels (one HIP launch sequence per call).

Every function takes torch tensors that already live on the GPU, checks shapes/dtypes on the host,
and calls the corresponding ``ergm_*`` entry point on the current HIP stream.  No function falls back
to PyTorch or CPU: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib as L


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev: torch.device):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("ergm_amd ops need GPU tensors (the HIP path has no CPU fallback)")


def gemm(A: torch.Tensor, B: torch.Tensor, M: int, N: int, K: int, a_layout: int = L.MK, b_layout: int = L.NK,
         out: Optional[torch.Tensor] = None, out_dtype=torch.float32, epilogue: int = L.EPI_NONE,
         bias: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None,
         aux_out: Optional[torch.Tensor] = None, alpha: float = 1.0, split_k: int = 0,
         alpha_dev: Optional[torch.Tensor] = None, bias_grad: Optional[torch.Tensor] = None,
         m_count: Optional[torch.Tensor] = None, k_count: Optional[torch.Tensor] = None,
         row_map: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C[M,N] = epilogue(alpha · A·B); A/B bf16 row-major with layouts as in ergm_hip.h.  ``bias_grad`` (f32 [N],
    KM x KN weight gradients only) also receives alpha·Σ_k B[k][n].  ``m_count`` / ``k_count`` (device int32
    scalars) and ``row_map`` (device int32 [M]) are the device-side extents and the store's row map of
    ergm_gemm_desc: M and K are then capacities, and rows of ``out`` no computed row maps to are left as they are."""
    _need_gpu(A, B)
    assert A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16
    lda = A.stride(0) if A.dim() == 2 else (K if a_layout == L.MK else M)
    ldb = B.stride(0) if B.dim() == 2 else (K if b_layout == L.NK else N)
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=A.device)
    d = L.GemmDesc(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=out.stride(0), a_layout=a_layout, b_layout=b_layout,
                   c_dtype=L.BF16 if out.dtype == torch.bfloat16 else L.F32, epilogue=epilogue, alpha=alpha,
                   bias=_ptr(bias), aux=_ptr(aux), ld_aux=aux.stride(0) if aux is not None else 0,
                   aux_out=_ptr(aux_out), ld_aux_out=aux_out.stride(0) if aux_out is not None else 0,
                   split_k=split_k, alpha_dev=_ptr(alpha_dev), bias_grad=_ptr(bias_grad), m_count_dev=_ptr(m_count),
                   k_count_dev=_ptr(k_count), row_map=_ptr(row_map))
    for t in (m_count, k_count, row_map):
        assert t is None or (t.is_cuda and t.dtype == torch.int32)
    lib = L.load()
    wsb = lib.ergm_gemm_workspace_size(C.byref(d))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=A.device)
    L.check(lib.ergm_gemm(C.byref(d), _ptr(A), _ptr(B), _ptr(out), _ptr(ws), wsb, _stream(A.device)), "ergm_gemm")
    return out


def linear_rows(A: torch.Tensor, W: torch.Tensor, M: int, N: int, K: int, w_layout: int = L.KN,
                out: Optional[torch.Tensor] = None, epilogue: int = L.EPI_NONE, bias: Optional[torch.Tensor] = None,
                aux: Optional[torch.Tensor] = None, ln_gamma: Optional[torch.Tensor] = None,
                ln_beta: Optional[torch.Tensor] = None, ln_eps: float = 1e-5) -> torch.Tensor:
    """C[M,N] = epilogue(A'·W + bias) for a handful of rows (ergm_linear_rows): A bf16 [>= M, >= K], or f32 rows
    that the kernel LayerNorms itself when ``ln_gamma`` / ``ln_beta`` are given; W bf16 [K, N] (KN) or [N, K] (NK).
    The output dtype follows the epilogue: f32 for NONE and BIAS_RESID (``aux`` f32, may be ``out``), bf16 otherwise."""
    _need_gpu(A, W)
    ln = ln_gamma is not None or ln_beta is not None
    if A.dtype != (torch.float32 if ln else torch.bfloat16) or W.dtype != torch.bfloat16:
        raise ValueError("linear_rows: A is bf16 (f32 with the LayerNorm prologue), W bf16")
    f32_out = epilogue in (L.EPI_NONE, L.EPI_BIAS_RESID)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32 if f32_out else torch.bfloat16, device=A.device)
    elif out.dtype != (torch.float32 if f32_out else torch.bfloat16):
        raise ValueError("linear_rows: the output dtype does not match the epilogue")
    for t in (bias, aux, ln_gamma, ln_beta):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise ValueError("linear_rows: bias, aux, ln_gamma and ln_beta are f32 GPU tensors")
    d = L.LinearRowsDesc(M=M, N=N, K=K, lda=A.stride(0) if A.dim() == 2 else K,
                         ldw=W.stride(0) if W.dim() == 2 else (N if w_layout == L.KN else K), ldc=out.stride(0),
                         w_layout=w_layout, epilogue=epilogue, bias=_ptr(bias), aux=_ptr(aux),
                         ld_aux=aux.stride(0) if aux is not None else 0, ln_gamma=_ptr(ln_gamma), ln_beta=_ptr(ln_beta),
                         ln_eps=ln_eps)
    L.check(L.load().ergm_linear_rows(C.byref(d), _ptr(A), _ptr(W), _ptr(out), _stream(A.device)), "ergm_linear_rows")
    return out


def lm_score(x: torch.Tensor, w: torch.Tensor, targets: torch.Tensor, V: int, R: Optional[int] = None,
             want=("logprob", "lse", "top1_logit", "top1"), ws: Optional[torch.Tensor] = None):
    """The tied head and the log-softmax of every row without the logits (ergm_lm_score): x bf16 [>= R, K], w bf16
    [>= V, K], targets int64 [R] (outside [0, V): the row is not scored and its logprob is exactly 0).  Returns the
    tuple ``(logprob, lse, top1_logit, top1)`` (f32, f32, f32, int32, [R] each) with None for a name not in ``want``.
    ``ws``: a uint8 workspace to reuse."""
    _need_gpu(x, w, targets)
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or targets.dtype != torch.int64:
        raise ValueError("lm_score: x and w are bf16, targets int64")
    if x.dim() != 2 or w.dim() != 2 or x.stride(1) != 1 or w.stride(1) != 1 or not targets.is_contiguous():
        raise ValueError("lm_score: x and w are 2-d with unit column stride, targets contiguous")
    R = x.shape[0] if R is None else R
    K = x.shape[1]
    if w.shape[1] != K or w.shape[0] < V or x.shape[0] < R or targets.numel() < R:
        raise ValueError("lm_score: w is [>= V, K], x [>= R, K], targets [>= R]")
    dev = x.device
    out = [torch.empty(R, dtype=torch.int32 if n == "top1" else torch.float32, device=dev) if n in want else None
           for n in ("logprob", "lse", "top1_logit", "top1")]
    need = L.load().ergm_lm_score_workspace_size(R, V, K)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    L.call("ergm_lm_score", _ptr(x), x.stride(0), _ptr(w), w.stride(0), _ptr(targets), R, V, K, *[_ptr(o) for o in out],
           _ptr(ws), ws.numel(), _stream(dev))
    return tuple(out)


def gemm_f8(A8: torch.Tensor, a_scale: torch.Tensor, B8t: torch.Tensor, b_scale: torch.Tensor,
            out: Optional[torch.Tensor] = None, out_dtype=torch.float32, epilogue: int = L.EPI_NONE,
            bias: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None,
            aux_out: Optional[torch.Tensor] = None, alpha: float = 1.0) -> torch.Tensor:
    """C[M,N] = epilogue(alpha · a_scale[m] · b_scale[n] · A8[m]·B8t[n]); A8 [M,K], B8t [N,K] e4m3 bytes
    (uint8 or torch.float8_e4m3fn), a_scale [M], b_scale [N] f32."""
    _need_gpu(A8, B8t, a_scale, b_scale)
    M, K = A8.shape
    N = B8t.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=A8.device)
    d = L.GemmDesc(M=M, N=N, K=K, lda=A8.stride(0), ldb=B8t.stride(0), ldc=out.stride(0), a_layout=L.MK,
                   b_layout=L.NK, c_dtype=L.BF16 if out.dtype == torch.bfloat16 else L.F32, epilogue=epilogue,
                   alpha=alpha, bias=_ptr(bias), aux=_ptr(aux), ld_aux=aux.stride(0) if aux is not None else 0,
                   aux_out=_ptr(aux_out), ld_aux_out=aux_out.stride(0) if aux_out is not None else 0)
    L.check(L.load().ergm_gemm_f8(C.byref(d), _ptr(A8), _ptr(a_scale), _ptr(B8t), _ptr(b_scale), _ptr(out),
                                  _stream(A8.device)), "ergm_gemm_f8")
    return out


def quant_rows_fp8(X: torch.Tensor, cols: Optional[int] = None):
    """Row-wise e4m3 quantisation: returns (Q [rows, cols] uint8, scale [rows] f32)."""
    _need_gpu(X)
    rows = X.shape[0]
    cols = X.shape[1] if cols is None else cols
    Q = torch.empty(rows, cols, dtype=torch.uint8, device=X.device)
    sc = torch.empty(rows, dtype=torch.float32, device=X.device)
    dt = L.BF16 if X.dtype == torch.bfloat16 else L.F32
    L.call("ergm_quant_rows_fp8", _ptr(X), dt, X.stride(0), rows, cols, _ptr(Q), cols, _ptr(sc), _stream(X.device))
    return Q, sc


def quant_weight_fp8(W: torch.Tensor):
    """Conv1D weight W [K, N] (f32 or bf16) → (Wt [N, K] e4m3 bytes, scale [N] f32), column-wise scales."""
    _need_gpu(W)
    K, N = W.shape
    Wt = torch.empty(N, K, dtype=torch.uint8, device=W.device)
    sc = torch.empty(N, dtype=torch.float32, device=W.device)
    ws = torch.empty(N, dtype=torch.int32, device=W.device)
    dt = L.BF16 if W.dtype == torch.bfloat16 else L.F32
    L.call("ergm_quant_weight_fp8", _ptr(W), dt, W.stride(0), K, N, _ptr(Wt), K, _ptr(sc), _ptr(ws), _stream(W.device))
    return Wt, sc


def gemm_mx(A8: torch.Tensor, a_sc: torch.Tensor, B8t: torch.Tensor, b_sc: torch.Tensor,
            out: Optional[torch.Tensor] = None, out_dtype=torch.float32, epilogue: int = L.EPI_NONE,
            bias: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None,
            aux_out: Optional[torch.Tensor] = None, alpha: float = 1.0, q_out: Optional[torch.Tensor] = None,
            q_sc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MX-fp8 GEMM: C[M,N] = epilogue(alpha · Σ_k dequant(A8)[m,k]·dequant(B8t)[n,k]) with A8 [M,K], B8t [N,K]
    e4m3 bytes and their e8m0 block scales (uint8, 2^(byte-127) per 32-element K block) in the library's
    K-step-major layout: a_sc [K/128, pitch >= M, 4], b_sc [K/128, pitch >= N, 4] (``mx_tile`` converts a
    [rows, K/32] array).  q_out / q_sc (BIAS_GELU / GELU_BWD): the MX copy of the bf16 output ([M,N] uint8 and
    [N/128, pitch >= M, 4])."""
    _need_gpu(A8, B8t, a_sc, b_sc)
    M, K = A8.shape
    N = B8t.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=A8.device)
    d = L.GemmDesc(M=M, N=N, K=K, lda=A8.stride(0), ldb=B8t.stride(0), ldc=out.stride(0), a_layout=L.MK,
                   b_layout=L.NK, c_dtype=L.BF16 if out.dtype == torch.bfloat16 else L.F32, epilogue=epilogue,
                   alpha=alpha, bias=_ptr(bias), aux=_ptr(aux), ld_aux=aux.stride(0) if aux is not None else 0,
                   aux_out=_ptr(aux_out), ld_aux_out=aux_out.stride(0) if aux_out is not None else 0)
    L.check(L.load().ergm_gemm_mx(C.byref(d), _ptr(A8), _ptr(a_sc), _pitch(a_sc), _ptr(B8t), _ptr(b_sc),
                                  _pitch(b_sc), _ptr(out), _ptr(q_out), _ptr(q_sc),
                                  q_out.stride(0) if q_out is not None else 0,
                                  _pitch(q_sc) if q_sc is not None else 0, _stream(A8.device)), "ergm_gemm_mx")
    return out


def _pitch(s: torch.Tensor) -> int:
    """Row pitch of an MX scale array [K/128, pitch, 4] (a 2-D [rows, 4] array: one 128-deep K step)."""
    assert s.dtype == torch.uint8 and s.is_contiguous() and s.shape[-1] == 4 and s.dim() in (2, 3)
    return s.shape[-2]


def mx_tile(S: torch.Tensor, pitch: Optional[int] = None) -> torch.Tensor:
    """[rows, nb] e8m0 block scales (block b = elements 32b..32b+31 of a row) → the library layout
    [ceil(nb/4), pitch, 4] (padding bytes 127)."""
    rows, nb = S.shape
    pitch = rows if pitch is None else pitch
    out = torch.full(((nb + 3) // 4, pitch, 4), 127, dtype=torch.uint8, device=S.device)
    Sp = torch.full((rows, out.shape[0] * 4), 127, dtype=torch.uint8, device=S.device)
    Sp[:, :nb] = S
    out[:, :rows] = Sp.reshape(rows, -1, 4).permute(1, 0, 2)
    return out


def mx_untile(T: torch.Tensor, rows: int, nb: int) -> torch.Tensor:
    """Inverse of mx_tile: [K/128, pitch, 4] → [rows, nb]."""
    return T[:, :rows].permute(1, 0, 2).reshape(rows, -1)[:, :nb].contiguous()


def quant_rows_mx(X: torch.Tensor, cols: Optional[int] = None):
    """MX-fp8 quantisation of rows: returns (Q [rows, cols] uint8 e4m3, S [ceil(cols/128), rows, 4] uint8 e8m0 in
    the library layout, ``mx_untile`` gives [rows, cols/32])."""
    _need_gpu(X)
    rows = X.shape[0]
    cols = X.shape[1] if cols is None else cols
    Q = torch.empty(rows, cols, dtype=torch.uint8, device=X.device)
    S = torch.empty((cols + 127) // 128, rows, 4, dtype=torch.uint8, device=X.device)
    dt = L.BF16 if X.dtype == torch.bfloat16 else L.F32
    L.call("ergm_quant_rows_mx", _ptr(X), dt, X.stride(0), rows, cols, _ptr(Q), cols, _ptr(S), rows,
           _stream(X.device))
    return Q, S


def quant_weight_mx(W: torch.Tensor, row_form: bool = False):
    """Conv1D weight W [K, N] (bf16) → (Wt [N, K] e4m3 bytes, S [K/128, N, 4] e8m0 block scales); with
    ``row_form`` also (Wr [K, N], Sr [N/128, K, 4]): W's rows quantised along N (the dX GEMM's B operand)."""
    _need_gpu(W)
    K, N = W.shape
    Wt = torch.empty(N, K, dtype=torch.uint8, device=W.device)
    S = torch.empty((K + 127) // 128, N, 4, dtype=torch.uint8, device=W.device)
    Wr = torch.empty(K, N, dtype=torch.uint8, device=W.device) if row_form else None
    Sr = torch.empty((N + 127) // 128, K, 4, dtype=torch.uint8, device=W.device) if row_form else None
    L.call("ergm_quant_weight_mx", _ptr(W), W.stride(0), K, N, _ptr(Wt), K, _ptr(S), N, _ptr(Wr), N, _ptr(Sr), K,
           _stream(W.device))
    return (Wt, S, Wr, Sr) if row_form else (Wt, S)


def dropout_desc(p: float, seed: int, offset: int, site: int, row0: int = 0) -> L.Dropout:
    """ergm_dropout for one site of one forward (include/ergm_hip.h)."""
    return L.Dropout(seed=seed & (2 ** 64 - 1), offset=offset & 0xFFFFFFFF, site=site, p=p, row0=row0)


def _dp(d: Optional[L.Dropout]):
    return None if d is None else C.byref(d)


def dropout_mask(d: L.Dropout, rows: int, cols: int, device) -> torch.Tensor:
    """The keep mask of dropout site ``d`` over [rows, cols] as bool (ergm_dropout_mask's bits)."""
    wpr = (cols + 31) // 32
    bits = torch.empty(rows * wpr, dtype=torch.int32, device=device)
    L.call("ergm_dropout_mask", C.byref(d), rows, cols, _ptr(bits), _stream(torch.device(device)))
    return unpack_bits(bits.view(rows, wpr), cols, 32)


def unpack_bits(words: torch.Tensor, cols: int, width: int) -> torch.Tensor:
    """[rows, n] little-endian words of `width` (32 / 64) bits -> bool [rows, cols] (bit j of word w =
    column width·w + j)."""
    rows = words.shape[0]
    b = words.contiguous().view(torch.uint8).view(rows, -1)            # little-endian bytes
    shifts = torch.arange(8, device=b.device, dtype=torch.uint8)
    bits = (b.unsqueeze(-1) >> shifts) & 1                               # [rows, bytes, 8]
    return bits.view(rows, -1)[:, :cols].bool()


def dropout_apply(x: torch.Tensor, d: L.Dropout) -> torch.Tensor:
    """In place: x = keep ? x/(1-p) : 0 (f32 [rows, cols])."""
    _need_gpu(x)
    rows, cols = x.shape
    L.call("ergm_dropout_apply", C.byref(d), _ptr(x), rows, cols, x.stride(0), _stream(x.device))
    return x


def attn_fwd(q, k, v, B, H, Sq, Sk, causal, o=None, lse=None, dropout: Optional[L.Dropout] = None):
    """q/k/v: 2-D token-major views [B*S, ld] whose first column is head 0, dim 0.  With ``dropout``
    also returns the keep bits the backward needs (u64 [B*H*Sq, ceil(Sk/64)])."""
    _need_gpu(q, k, v)
    dev = q.device
    if o is None:
        o = torch.empty(B * Sq, H * 64, dtype=torch.bfloat16, device=dev)
    if lse is None:
        lse = torch.empty(B, H, Sq, dtype=torch.float32, device=dev)
    bits = torch.zeros(B * H * Sq, (Sk + 63) // 64, dtype=torch.int64, device=dev) if dropout is not None else None
    L.call("ergm_attn_fwd", _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), B, H, Sq, Sk, q.stride(0), k.stride(0),
           v.stride(0), o.stride(0), int(bool(causal)), _dp(dropout), _ptr(bits), _stream(dev))
    return (o, lse) if dropout is None else (o, lse, bits)


def attn_bwd(q, k, v, o, dout, lse, B, H, Sq, Sk, causal, dq=None, dk=None, dv=None,
             dropout: Optional[L.Dropout] = None, keep_bits: Optional[torch.Tensor] = None,
             delta: Optional[torch.Tensor] = None):
    """``delta`` (f32, B*H*Sq elements): where the tiled kernels leave rowsum(dO∘O) (the short kernel keeps it in LDS);
    a scratch buffer by default."""
    _need_gpu(q, k, v, o, dout, lse)
    dev = q.device
    dq = torch.empty(B * Sq, H * 64, dtype=torch.bfloat16, device=dev) if dq is None else dq
    dk = torch.empty(B * Sk, H * 64, dtype=torch.bfloat16, device=dev) if dk is None else dk
    dv = torch.empty(B * Sk, H * 64, dtype=torch.bfloat16, device=dev) if dv is None else dv
    if delta is None:
        delta = torch.empty(B, H, Sq, dtype=torch.float32, device=dev)
    elif not delta.is_cuda or delta.dtype != torch.float32 or delta.numel() < B * H * Sq or not delta.is_contiguous():
        raise ValueError("attn_bwd: delta is a contiguous f32 GPU tensor of at least B*H*Sq elements")
    L.call("ergm_attn_bwd", _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(dout), _ptr(lse), _ptr(delta), _ptr(dq), _ptr(dk),
           _ptr(dv), B, H, Sq, Sk, q.stride(0), k.stride(0), v.stride(0), o.stride(0), dout.stride(0), dq.stride(0),
           dk.stride(0), dv.stride(0), int(bool(causal)), _dp(dropout), _ptr(keep_bits), _stream(dev))
    return dq, dk, dv


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    _need_gpu(x, gamma, beta)
    rows, E = x.shape
    y = torch.empty(rows, E, dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    L.call("ergm_layernorm_fwd", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), rows, E, eps,
           _stream(x.device))
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, dres, dropout: Optional[L.Dropout] = None):
    """dres += LN_bwd(dy) in place; returns (dres, dres_bf16, dgamma, dbeta) (dres_bf16 through the
    residual-branch ``dropout`` when given)."""
    _need_gpu(dy, x, mean, rstd, gamma, dres)
    rows, E = x.shape
    lib = L.load()
    wsb = lib.ergm_layernorm_bwd_workspace_size(rows, E)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    db = torch.empty(rows, E, dtype=torch.bfloat16, device=x.device)
    dg = torch.empty(E, dtype=torch.float32, device=x.device)
    dbe = torch.empty_like(dg)
    L.call("ergm_layernorm_bwd", _ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dres), _ptr(db), _ptr(dg),
           _ptr(dbe), _ptr(ws), wsb, rows, E, _dp(dropout), _stream(x.device))
    return dres, db, dg, dbe


def layernorm_fwd_ld(x, gamma, beta, y, eps=1e-5, mean=None, rstd=None):
    """ergm_layernorm_fwd_ld: ``y`` is a bf16 [rows, E] view whose row stride may exceed E (the pad columns are not
    written).  Returns (y, mean, rstd)."""
    _need_gpu(x, gamma, beta, y)
    rows, E = x.shape
    if y.dtype != torch.bfloat16 or y.shape != (rows, E) or y.stride(1) != 1:
        raise ValueError("layernorm_fwd_ld: y is a bf16 [rows, E] view with unit column stride")
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if mean is None else mean
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if rstd is None else rstd
    L.call("ergm_layernorm_fwd_ld", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), y.stride(0), _ptr(mean), _ptr(rstd), rows,
           E, eps, _stream(x.device))
    return y, mean, rstd


def layernorm_bwd_ex(dy, x, mean, rstd, gamma, dres, dres_bf16=None, dgamma=None, dbeta=None,
                     dropout: Optional[L.Dropout] = None, drop_res: bool = False):
    """ergm_layernorm_bwd_ex: ``dy`` f32 or bf16 [rows, E]; dres += LN_bwd(dy) in place, with ``drop_res`` the sum
    itself through ``dropout`` (then ``dres_bf16`` is None); ``dres_bf16`` (bf16 [rows, E] or None) as
    layernorm_bwd's.  Returns (dres, dres_bf16, dgamma, dbeta)."""
    _need_gpu(dy, x, mean, rstd, gamma, dres)
    rows, E = x.shape
    if dy.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("layernorm_bwd_ex: dy is f32 or bf16")
    lib = L.load()
    wsb = lib.ergm_layernorm_bwd_workspace_size(rows, E)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=x.device)
    dgamma = torch.empty(E, dtype=torch.float32, device=x.device) if dgamma is None else dgamma
    dbeta = torch.empty(E, dtype=torch.float32, device=x.device) if dbeta is None else dbeta
    L.call("ergm_layernorm_bwd_ex", _ptr(dy), L.BF16 if dy.dtype == torch.bfloat16 else L.F32, _ptr(x), _ptr(mean),
           _ptr(rstd), _ptr(gamma), _ptr(dres), _ptr(dres_bf16), _ptr(dgamma), _ptr(dbeta), _ptr(ws), wsb, rows, E,
           _dp(dropout), int(bool(drop_res)), _stream(x.device))
    return dres, dres_bf16, dgamma, dbeta


def colsum(X, out=None, accumulate=False):
    _need_gpu(X)
    rows, cols = X.shape
    out = torch.zeros(cols, dtype=torch.float32, device=X.device) if out is None else out
    lib = L.load()
    wsb = lib.ergm_colsum_workspace_size(rows, cols)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=X.device)
    L.call("ergm_colsum", _ptr(X), L.BF16 if X.dtype == torch.bfloat16 else L.F32, rows, cols, X.stride(0), _ptr(out),
           int(accumulate), _ptr(ws), wsb, _stream(X.device))
    return out


def embed_fwd(ids, tt, cap_ids, wte, wpe, vis=None, aud=None, dropout: Optional[L.Dropout] = None):
    _need_gpu(ids, cap_ids, wte, wpe)
    B, S = ids.shape
    V, E = wte.shape
    h0 = torch.empty(B * S, E, dtype=torch.float32, device=ids.device)
    cap = torch.empty(B * S, E, dtype=torch.bfloat16, device=ids.device)
    ld_vis = 0
    if vis is not None:
        vis = vis.contiguous()
        ld_vis = vis[0].numel() if vis.dim() == 3 else vis.shape[1]
    L.call("ergm_embed_fwd", _ptr(ids), _ptr(tt), _ptr(cap_ids), _ptr(wte), _ptr(wpe), _ptr(vis), ld_vis,
           _ptr(aud), _ptr(h0), _ptr(cap), B, S, E, V, _dp(dropout), _stream(ids.device))
    return h0, cap


def attn_decode_workspace(B: int, H: int, max_len: int, device, splits: int = 0) -> torch.Tensor:
    """The fp32 workspace ergm_attn_decode needs for the automatic split count (or for a forced ``splits``)."""
    n = max(L.load().ergm_attn_decode_workspace_size(B, H, max_len), B * H * max(splits, 1) * 66 * 4, 16)
    return torch.empty(n, dtype=torch.uint8, device=device)


def attn_decode(qkv, kcache, vcache, lens, append: bool, splits: int = 0, out=None, ws=None):
    """One query per sequence over a ragged cache (ergm_attn_decode).  qkv [B, >= E (3E with ``append``)] bf16;
    kcache / vcache: [B, max_len, E] bf16 views (any sequence and row strides) of the per-sequence K and V rows;
    lens int32 [B] on the device.  With ``append`` the new K/V row is stored at row lens[b] and attended too."""
    _need_gpu(qkv, kcache, vcache, lens)
    assert qkv.dtype == kcache.dtype == vcache.dtype == torch.bfloat16 and lens.dtype == torch.int32
    B, max_len, E = kcache.shape
    if vcache.shape != kcache.shape or vcache.stride() != kcache.stride() or kcache.stride(2) != 1 or E % 64:
        raise ValueError("attn_decode: kcache / vcache must be [B, max_len, 64·H] views with the same strides")
    if qkv.shape[0] != B or lens.numel() != B or qkv.stride(1) != 1:
        raise ValueError("attn_decode: qkv and lens must have one row per sequence")
    H = E // 64
    dev = qkv.device
    if out is None:
        out = torch.empty(B, E, dtype=torch.bfloat16, device=dev)
    if ws is None and splits != 1:
        ws = attn_decode_workspace(B, H, max_len, dev, splits)
    L.call("ergm_attn_decode", _ptr(qkv), qkv.stride(0), _ptr(kcache), _ptr(vcache), kcache.stride(0), kcache.stride(1),
           _ptr(lens), B, H, max_len, int(bool(append)), splits, _ptr(out), out.stride(0), _ptr(ws),
           0 if ws is None else ws.numel() * ws.element_size(), _stream(dev))
    return out


def embed_rows(ids, tt, pos, wte, wpe, out=None):
    """h[b] = wte[ids[b]] + wpe[pos[b]] + wte[tt[b]] (ergm_embed_rows): ids / tt int64 [B], pos int32 [B]."""
    _need_gpu(ids, pos, wte, wpe)
    assert ids.dtype == torch.int64 and pos.dtype == torch.int32 and (tt is None or tt.dtype == torch.int64)
    B = ids.numel()
    V, E = wte.shape
    if out is None:
        out = torch.empty(B, E, dtype=torch.float32, device=ids.device)
    L.call("ergm_embed_rows", _ptr(ids), _ptr(tt), _ptr(pos), _ptr(wte), _ptr(wpe), _ptr(out), B, E, V, wpe.shape[0],
           _stream(ids.device))
    return out


def _sampler_args(logits, finished, tokens, row_ids=None, row_steps=None):
    """The samplers' shared checks; returns B and ``tokens`` (allocated if None)."""
    rows = () if row_ids is None else (row_ids, row_steps)
    _need_gpu(logits, *rows)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    assert finished is None or finished.dtype == torch.uint8
    B = logits.shape[0]
    for t in rows:
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == B
    if tokens is None:
        tokens = torch.empty(B, dtype=torch.int64, device=logits.device)
    return B, tokens


def topp_sample(logits, V: int, top_p: float, seed: int, step: int, eos_id: int, finished=None, tokens=None,
                kept=None, kept_mass=None):
    """Nucleus sampling of the rows of logits [B, >= V] f32 on the device (ergm_topp_sample); returns ``tokens``
    (int64 [B]).  ``finished`` (uint8 [B]) is read and updated; ``kept`` (int32 [B]) / ``kept_mass`` (f32 [B]) are
    optional diagnostics."""
    B, tokens = _sampler_args(logits, finished, tokens)
    L.call("ergm_topp_sample", _ptr(logits), logits.stride(0), B, V, float(top_p), seed & (2 ** 64 - 1),
           step & 0xFFFFFFFF, _ptr(finished), eos_id, _ptr(tokens), _ptr(kept), _ptr(kept_mass), _stream(logits.device))
    return tokens


def attn_fwd_ragged(q, k, v, q_start, q_len, k_start, k_len, H: int, max_q: int, max_k: int, causal: bool, o=None,
                    lse=None):
    """Inference attention over packed sequences of different lengths in one launch (ergm_attn_fwd_ragged).  q / o:
    [total_q, ld] bf16 rows, k / v: [total_k, ld]; q_start / q_len / k_start / k_len: int32 [n_seq] on the device;
    max_q / max_k: the host's bounds on the lengths.  ``lse`` (optional, f32 [H·total_q]) holds sequence b's
    [H, q_len[b]] block at H·q_start[b].  Returns ``o``."""
    _need_gpu(q, k, v, q_start, q_len, k_start, k_len)
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16
    for t in (q_start, q_len, k_start, k_len):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == q_start.numel()
    dev = q.device
    if o is None:
        o = torch.empty(q.shape[0], H * 64, dtype=torch.bfloat16, device=dev)
    L.call("ergm_attn_fwd_ragged", _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(lse), _ptr(q_start), _ptr(q_len), _ptr(k_start),
           _ptr(k_len), q_start.numel(), H, q.shape[0], k.shape[0], max_q, max_k, q.stride(0), k.stride(0), v.stride(0),
           o.stride(0), int(bool(causal)), _stream(dev))
    return o


def rows_to_slots(src, start, length, slot, max_rows: int, dst, n_slots: Optional[int] = None,
                  slot_rows: Optional[int] = None):
    """Row t < length[b] of sequence b (row start[b] + t of ``src`` [rows, width]) -> dst[slot[b], t] (ergm_rows_to_slots).
    ``dst``: [n_slots, slot_rows, width] (or [n_slots, width] with one row per slot), the same dtype as ``src``, rows
    of a multiple of 16 bytes; start / length / slot int32 [n_seq] on the device; max_rows the host's bound on length."""
    _need_gpu(src, start, length, slot, dst)
    assert src.dtype == dst.dtype and src.dim() == 2 and src.stride(1) == 1 and dst.stride(-1) == 1
    for t in (start, length, slot):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == start.numel()
    es = src.element_size()
    if dst.dim() == 2:
        ld_slot, ld_row, rows = dst.stride(0), dst.stride(0), 1
    else:
        ld_slot, ld_row, rows = dst.stride(0), dst.stride(1), dst.shape[1]
    if src.shape[1] != dst.shape[-1]:
        raise ValueError("rows_to_slots: src and dst rows differ in width")
    L.call("ergm_rows_to_slots", _ptr(src), src.stride(0) * es, _ptr(start), _ptr(length), _ptr(slot), start.numel(),
           src.shape[0], max_rows, _ptr(dst), ld_slot * es, ld_row * es, src.shape[1] * es,
           dst.shape[0] if n_slots is None else n_slots, rows if slot_rows is None else slot_rows, _stream(src.device))
    return dst


def attn_fwd_extend(q, k, v, q_start, q_len, k_start, k_len, H: int, max_q: int, max_k: int, o=None):
    """Causal attention of packed new query rows over caches that already hold a past, in one launch
    (ergm_attn_fwd_extend).  ``attn_fwd_ragged``'s arguments; k_len[b] >= q_len[b], query row s of sequence b sits at
    position k_len[b] - q_len[b] + s and sees the keys up to it, and the new rows' own K / V are already among the key
    rows.  Row s is bitwise row past + s of ``attn_fwd(B=1, Sq=Sk=k_len[b], causal)``.  Returns ``o``."""
    _need_gpu(q, k, v, q_start, q_len, k_start, k_len)
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16
    for t in (q_start, q_len, k_start, k_len):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == q_start.numel()
    dev = q.device
    if o is None:
        o = torch.empty(q.shape[0], H * 64, dtype=torch.bfloat16, device=dev)
    L.call("ergm_attn_fwd_extend", _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(q_start), _ptr(q_len), _ptr(k_start),
           _ptr(k_len), q_start.numel(), H, q.shape[0], k.shape[0], max_q, max_k, q.stride(0), k.stride(0), v.stride(0),
           o.stride(0), _stream(dev))
    return o


def rows_to_slots_at(src, start, length, slot, dst_row0, max_rows: int, dst, n_slots: Optional[int] = None,
                     slot_rows: Optional[int] = None):
    """``rows_to_slots`` with a first destination row per sequence: row t < length[b] of sequence b -> dst[slot[b],
    dst_row0[b] + t] (ergm_rows_to_slots_at); a sequence stops at the slot's last row."""
    _need_gpu(src, start, length, slot, dst_row0, dst)
    assert src.dtype == dst.dtype and src.dim() == 2 and src.stride(1) == 1 and dst.stride(-1) == 1
    for t in (start, length, slot, dst_row0):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == start.numel()
    es = src.element_size()
    if dst.dim() == 2:
        ld_slot, ld_row, rows = dst.stride(0), dst.stride(0), 1
    else:
        ld_slot, ld_row, rows = dst.stride(0), dst.stride(1), dst.shape[1]
    if src.shape[1] != dst.shape[-1]:
        raise ValueError("rows_to_slots_at: src and dst rows differ in width")
    L.call("ergm_rows_to_slots_at", _ptr(src), src.stride(0) * es, _ptr(start), _ptr(length), _ptr(slot), _ptr(dst_row0),
           start.numel(), src.shape[0], max_rows, _ptr(dst), ld_slot * es, ld_row * es, src.shape[1] * es,
           dst.shape[0] if n_slots is None else n_slots, rows if slot_rows is None else slot_rows, _stream(src.device))
    return dst


def embed_packed(ids, tt, cap_ids, wte, wpe, q_start, q_len, c_start, c_len, max_rows: int, max_cap: int, vis=None,
                 aud=None, has_feat=None):
    """ergm_embed_fwd for packed rows (ergm_embed_packed): ids / tt int64 [Σ n_b], cap_ids int64 [Σ c_b], the starts
    and lengths int32 [n_seq] on the device, vis / aud f32 [n_seq, E] (projected) or None, has_feat uint8 [n_seq] or
    None.  Returns (h0 f32 [Σ n_b, E], cap bf16 [Σ c_b, E])."""
    _need_gpu(ids, cap_ids, wte, wpe, q_start, q_len, c_start, c_len)
    assert ids.dtype == torch.int64 and cap_ids.dtype == torch.int64 and (tt is None or tt.dtype == torch.int64)
    assert has_feat is None or has_feat.dtype == torch.uint8
    V, E = wte.shape
    n_seq = q_start.numel()
    if vis is not None:
        vis, aud = vis.contiguous(), aud.contiguous()
        assert vis.shape == aud.shape == (n_seq, E) and vis.dtype == aud.dtype == torch.float32
    R, Rc = ids.numel(), cap_ids.numel()
    h0 = torch.empty(R, E, dtype=torch.float32, device=ids.device)
    cap = torch.empty(Rc, E, dtype=torch.bfloat16, device=ids.device)
    L.call("ergm_embed_packed", _ptr(ids), _ptr(tt), _ptr(cap_ids), _ptr(wte), _ptr(wpe), _ptr(vis), _ptr(aud),
           _ptr(has_feat), _ptr(q_start), _ptr(q_len), _ptr(c_start), _ptr(c_len), n_seq, R, Rc, max_rows, max_cap,
           _ptr(h0), _ptr(cap), E, E, V, wpe.shape[0], _stream(ids.device))
    return h0, cap


def topp_sample_rows(logits, V: int, top_p: float, seed: int, row_ids, row_steps, eos_id: int, finished=None,
                     tokens=None, kept=None, kept_mass=None):
    """ergm_topp_sample with the Philox counter {row_ids[b], 0, 0xE5A3, row_steps[b]} per row (ergm_topp_sample_rows):
    row_ids / row_steps uint32 [B] on the device, passed as int32 tensors holding the same bits."""
    B, tokens = _sampler_args(logits, finished, tokens, row_ids, row_steps)
    L.call("ergm_topp_sample_rows", _ptr(logits), logits.stride(0), B, V, float(top_p), seed & (2 ** 64 - 1), _ptr(row_ids),
           _ptr(row_steps), _ptr(finished), eos_id, _ptr(tokens), _ptr(kept), _ptr(kept_mass), _stream(logits.device))
    return tokens


def sample_ctl(top_p=None, temperature=None, rep_penalty=None, top_k=None, min_step=None, seen=None) -> L.SampleCtl:
    """ergm_sample_ctl over per-row device tensors: top_p / temperature / rep_penalty f32 [B], top_k int32 [B],
    min_step int32 [B] (uint32 bits), seen int32 [B, >= ceil(V / 32)] (uint32 bits); None is the default of every
    row.  The struct holds addresses only: the caller keeps the tensors alive."""
    for t, dt in ((top_p, torch.float32), (temperature, torch.float32), (rep_penalty, torch.float32), (top_k, torch.int32),
                  (min_step, torch.int32), (seen, torch.int32)):
        if t is not None:
            _need_gpu(t)
            assert t.dtype == dt and t.is_contiguous()
    assert seen is None or seen.dim() == 2
    p = lambda t: None if t is None else t.data_ptr()
    return L.SampleCtl(p(top_p), p(temperature), p(rep_penalty), p(top_k), p(min_step), p(seen),
                       0 if seen is None else seen.stride(0))


def sample_rows(logits, V: int, top_p: float, seed: int, row_ids, row_steps, eos_id: int, ctl: Optional[L.SampleCtl] = None,
                finished=None, tokens=None, kept=None, kept_mass=None, logprob=None):
    """``topp_sample_rows`` with per-row sampling controls (ergm_sample_rows): ``ctl`` from ``sample_ctl`` (None: every
    default, the old sampler's outputs); ``logprob`` (f32 [B], optional) receives the drawn tokens' log-probabilities."""
    B, tokens = _sampler_args(logits, finished, tokens, row_ids, row_steps)
    assert logprob is None or (logprob.dtype == torch.float32 and logprob.is_contiguous())
    L.call("ergm_sample_rows", _ptr(logits), logits.stride(0), B, V, float(top_p), None if ctl is None else C.byref(ctl),
           seed & (2 ** 64 - 1), _ptr(row_ids), _ptr(row_steps), _ptr(finished), eos_id, _ptr(tokens), _ptr(kept),
           _ptr(kept_mass), _ptr(logprob), _stream(logits.device))
    return tokens


def sample_mark(ids, slot, start, length, V: int, seen=None, reset=None, min_new=None, row_steps=None, min_step=None,
                n_slots: Optional[int] = None):
    """Record the packed ``ids`` (int64 [total]) of n_seq sequences in the bitmap rows of their slots and set the slots'
    minimum length (ergm_sample_mark): slot / start / length (and reset / min_new, optional) int32 [n_seq] on the device;
    seen int32 [n_slots, >= ceil(V / 32)]; min_step[slot] = row_steps[slot] + min_new (int32 [n_slots], uint32 bits)."""
    _need_gpu(ids, slot, start, length)
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    for t in (slot, start, length, reset, min_new):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() == slot.numel())
    for t in (seen, row_steps, min_step):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous())
    if n_slots is None:
        n_slots = seen.shape[0] if seen is not None else min_step.numel()
    L.call("ergm_sample_mark", _ptr(ids), ids.numel(), _ptr(slot), _ptr(start), _ptr(length), _ptr(reset), _ptr(min_new),
           slot.numel(), V, n_slots, _ptr(seen), 0 if seen is None else seen.stride(0), _ptr(row_steps), _ptr(min_step),
           _stream(ids.device))


def beam_select(logits, V: int, W: int, scores, finished, eos_id: int, parent=None, token=None, ws=None):
    """One select of beam search over the rows of logits [R, >= V] f32, W consecutive rows per prompt (ergm_beam_select):
    ``scores`` (f32 [R]) and ``finished`` (uint8 [R]) are read and updated in place; returns ``(parent, token)``, int32 /
    int64 [R]: the row each row continues and the token it takes.  ``ws``: a uint8 workspace to reuse."""
    _need_gpu(logits, scores, finished)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    R = logits.shape[0]
    assert scores.dtype == torch.float32 and finished.dtype == torch.uint8
    assert scores.is_contiguous() and finished.is_contiguous() and scores.numel() == R and finished.numel() == R
    dev = logits.device
    if parent is None:
        parent = torch.empty(R, dtype=torch.int32, device=dev)
    if token is None:
        token = torch.empty(R, dtype=torch.int64, device=dev)
    assert parent.dtype == torch.int32 and token.dtype == torch.int64 and parent.is_contiguous() and token.is_contiguous()
    need = L.load().ergm_beam_select_workspace_size(R, W)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    L.call("ergm_beam_select", _ptr(logits), logits.stride(0), R, W, V, _ptr(scores), _ptr(finished), eos_id, _ptr(parent),
           _ptr(token), _ptr(ws), ws.numel(), _stream(dev))
    return parent, token


def beam_gather(caches, parent, lens, W: int, max_len: Optional[int] = None):
    """The caches follow the beams (ergm_beam_gather): ``caches`` is a list of per-layer tensors [R, rows, width] with
    the same strides; for every row with parent[r] != r the cache rows [0, lens[parent[r]]) of every layer go from slot
    parent[r] to slot r, and lens[r] = lens[parent[r]].  ``max_len``: the host's bound on the lengths (default: rows)."""
    _need_gpu(parent, lens, *caches)
    c0 = caches[0]
    assert parent.dtype == torch.int32 and lens.dtype == torch.int32 and parent.is_contiguous() and lens.is_contiguous()
    R = parent.numel()
    for c in caches:
        assert c.dim() == 3 and c.dtype == c0.dtype and c.shape == c0.shape and c.stride() == c0.stride() and c.stride(2) == 1
    if c0.shape[0] < R or lens.numel() < R:
        raise ValueError("beam_gather: fewer cache slots or lengths than rows")
    es = c0.element_size()
    rows = c0.shape[1] if max_len is None else max_len
    if not 1 <= rows <= c0.shape[1]:
        raise ValueError(f"beam_gather: max_len {rows} outside [1, {c0.shape[1]}]")
    ptrs = (C.c_void_p * len(caches))(*[c.data_ptr() for c in caches])
    L.call("ergm_beam_gather", ptrs, len(caches), c0.stride(0) * es, c0.stride(1) * es, c0.shape[2] * es, _ptr(parent),
           _ptr(lens), R, W, rows, _stream(c0.device))


def beam_seed(xkv, groups, W: int, cap_max: int, lens, cap_lens, stop_lens, finished, scores, groups_dev=None):
    """Seed groups of W slots behind an admission that filled row g·W of each (ergm_beam_seed): ``xkv`` is a list of
    per-layer caption caches [max_batch, rows >= cap_max, width] with the same strides; for every g in ``groups`` (host
    ints) the caption rows [0, clamp(cap_lens[g·W], 0, cap_max)) of every layer go from slot g·W to the group's other
    slots, those rows get that caption length, stop_lens[g·W], lens 0, finished 0 and score -inf, and scores[g·W] = 0.
    ``groups_dev``: the same ids as int32 on the device (default: copied from ``groups``)."""
    _need_gpu(lens, cap_lens, stop_lens, finished, scores, *xkv)
    c0 = xkv[0]
    for c in xkv:
        assert c.dim() == 3 and c.dtype == c0.dtype and c.shape == c0.shape and c.stride() == c0.stride() and c.stride(2) == 1
    for t in (lens, cap_lens, stop_lens):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert finished.dtype == torch.uint8 and scores.dtype == torch.float32 and finished.is_contiguous() and scores.is_contiguous()
    mb = c0.shape[0]
    if min(t.numel() for t in (lens, cap_lens, stop_lens, finished, scores)) < mb:
        raise ValueError("beam_seed: fewer state rows than cache slots")
    if not 1 <= cap_max <= c0.shape[1]:
        raise ValueError(f"beam_seed: cap_max {cap_max} outside [1, {c0.shape[1]}]")
    groups = [int(g) for g in groups]
    if groups_dev is None:
        groups_dev = torch.tensor(groups, dtype=torch.int32).to(c0.device)
    assert groups_dev.dtype == torch.int32 and groups_dev.is_contiguous() and groups_dev.numel() == len(groups)
    _need_gpu(groups_dev)
    es = c0.element_size()
    ptrs = (C.c_void_p * len(xkv))(*[c.data_ptr() for c in xkv])
    L.call("ergm_beam_seed", ptrs, len(xkv), c0.stride(0) * es, c0.stride(1) * es, c0.shape[2] * es, _ptr(groups_dev),
           (C.c_int * len(groups))(*groups), len(groups), W, mb, cap_max, _ptr(lens), _ptr(cap_lens), _ptr(stop_lens),
           _ptr(finished), _ptr(scores), _stream(c0.device))


def rules_desc(hist, start=None, ngram=None, bad=None) -> L.LogitRules:
    """ergm_logit_rules over device tensors: hist int32 [R, >= max_len] (rows ld_hist apart), start / ngram int32 [R],
    bad int32 [R, ld_bad] (length-prefixed sequences); None turns a rule off.  The struct holds addresses only: the
    caller keeps the tensors alive."""
    _need_gpu(hist)
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.stride(1) == 1
    for t in (start, ngram):
        if t is not None:
            _need_gpu(t)
            assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= hist.shape[0]
    if bad is not None:
        _need_gpu(bad)
        assert bad.dtype == torch.int32 and bad.dim() == 2 and bad.stride(1) == 1 and bad.shape[0] >= hist.shape[0]
    p = lambda t: None if t is None else t.data_ptr()
    return L.LogitRules(p(hist), hist.stride(0), p(start), p(ngram), p(bad), 0 if bad is None else bad.stride(0))


def logit_rules(logits, V: int, rules: L.LogitRules, lens, eos_id: int, max_len: int, finished=None):
    """Ban the tokens the rows' rules forbid next, in place (ergm_logit_rules_apply): logits f32 [R, >= V], ``rules``
    from ``rules_desc``, lens int32 [R], finished uint8 [R] or None.  A banned token's logit becomes -inf; eos_id never."""
    _need_gpu(logits, lens)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
    assert lens.dtype == torch.int32 and lens.is_contiguous() and lens.numel() >= logits.shape[0]
    assert finished is None or (finished.dtype == torch.uint8 and finished.is_contiguous())
    L.call("ergm_logit_rules_apply", _ptr(logits), logits.stride(0), logits.shape[0], V, C.byref(rules), _ptr(lens),
           _ptr(finished), eos_id, max_len, _stream(logits.device))
    return logits


def hist_write(ids, slot, start, length, hist, max_len: int, pos0=None, n_slots: Optional[int] = None):
    """The packed ``ids`` (int64 [total]) of n_seq sequences into the history rows of their slots (ergm_hist_write):
    slot / start / length (and pos0, the first position written; None: 0) int32 [n_seq] on the device, hist int32
    [n_slots, >= max_len]."""
    _need_gpu(ids, slot, start, length, hist)
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    for t in (slot, start, length, pos0):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.numel() == slot.numel())
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.stride(1) == 1
    L.call("ergm_hist_write", _ptr(ids), ids.numel(), _ptr(slot), _ptr(start), _ptr(length), _ptr(pos0), slot.numel(),
           hist.shape[0] if n_slots is None else n_slots, _ptr(hist), hist.stride(0), max_len, _stream(ids.device))


def hist_append(tokens, lens, hist, max_len: int, finished=None):
    """hist[r, lens[r]] = tokens[r] for every row that is not finished (ergm_hist_append): tokens int64 [R], lens int32
    [R], finished uint8 [R] or None; behind the sampler or the select, before the step."""
    _need_gpu(tokens, lens, hist)
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and lens.dtype == torch.int32 and lens.is_contiguous()
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.stride(1) == 1 and hist.shape[0] >= tokens.numel()
    assert finished is None or (finished.dtype == torch.uint8 and finished.is_contiguous())
    L.call("ergm_hist_append", _ptr(tokens), _ptr(lens), _ptr(finished), tokens.numel(), _ptr(hist), hist.stride(0), max_len,
           _stream(tokens.device))


def hist_follow(hist, parent, lens, W: int, max_len: int):
    """The histories follow the beams (ergm_hist_follow): the rows ``beam_gather`` moves for ``parent`` take positions
    [0, lens[parent[r]]) of their parent's row.  lens is not written."""
    _need_gpu(hist, parent, lens)
    assert parent.dtype == torch.int32 and lens.dtype == torch.int32 and parent.is_contiguous() and lens.is_contiguous()
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.stride(1) == 1 and hist.shape[0] >= parent.numel()
    L.call("ergm_hist_follow", _ptr(hist), hist.stride(0), _ptr(parent), _ptr(lens), parent.numel(), W, max_len,
           _stream(hist.device))


def session_bytes(n_layer: int, row_bytes: int, rows: int, cap_rows: int, ld_seen: int = 0, bad_cap: int = 0, flags: int = 0) -> int:
    """The size of a session blob (ergm_session_bytes; host only).  ValueError for arguments it rejects."""
    n = L.load().ergm_session_bytes(n_layer, row_bytes, rows, cap_rows, ld_seen, bad_cap, flags)
    if n == 0:
        raise ValueError(f"session_bytes: bad shape n_layer {n_layer} row_bytes {row_bytes} rows {rows} cap_rows {cap_rows} "
                         f"ld_seen {ld_seen} bad_cap {bad_cap} flags {flags}")
    return n


def session_header(n_layer: int, row_bytes: int, rows: int, cap_rows: int, ld_seen: int = 0, bad_cap: int = 0,
                   flags: int = 0) -> L.SessionHdr:
    """The host's copy of a blob's header (ergm_session_header): everything but the draw counters."""
    h = L.SessionHdr()
    L.call("ergm_session_header", n_layer, row_bytes, rows, cap_rows, ld_seen, bad_cap, flags, C.byref(h))
    return h


class SessionState:
    """ergm_session_state over a generator's buffers: ``kv`` / ``xkv`` lists of per-layer caches [max_batch, rows, width]
    with the same strides per list, the slot-state arrays (int32 [max_batch]; finished uint8), and optionally the
    ``sample_ctl`` / ``rules_desc`` structs of the per-slot controls and rules.  Holds addresses only: the caller keeps
    the tensors alive.  ``max_len`` / ``cap_max`` default to the caches' row counts."""

    def __init__(self, kv, xkv, lens, cap_lens, stop_lens, finished, row_ids, row_steps, ctl: Optional[L.SampleCtl] = None,
                 rules: Optional[L.LogitRules] = None, max_len: Optional[int] = None, cap_max: Optional[int] = None):
        _need_gpu(lens, cap_lens, stop_lens, finished, row_ids, row_steps, *kv, *xkv)
        k0, x0 = kv[0], xkv[0]
        if len(kv) != len(xkv):
            raise ValueError("session state: one caption cache per self-attention cache")
        for group, c0 in ((kv, k0), (xkv, x0)):
            for c in group:
                assert c.dim() == 3 and c.dtype == k0.dtype and c.shape == c0.shape and c.stride() == c0.stride() and c.stride(2) == 1
        assert k0.shape[0] == x0.shape[0] and k0.shape[2] == x0.shape[2]
        mb = k0.shape[0]
        for t in (lens, cap_lens, stop_lens, row_ids, row_steps):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= mb
        assert finished.dtype == torch.uint8 and finished.is_contiguous() and finished.numel() >= mb
        es = k0.element_size()
        self.device, self.n_layer, self.row_bytes, self.max_batch = k0.device, len(kv), k0.shape[2] * es, mb
        self.max_len = k0.shape[1] if max_len is None else max_len
        self.cap_max = x0.shape[1] if cap_max is None else cap_max
        if not (1 <= self.max_len <= k0.shape[1] and 1 <= self.cap_max <= x0.shape[1]):
            raise ValueError("session state: max_len / cap_max outside the caches")
        self._keep = (kv, xkv, lens, cap_lens, stop_lens, finished, row_ids, row_steps, ctl, rules,
                      (C.c_void_p * len(kv))(*[c.data_ptr() for c in kv]), (C.c_void_p * len(xkv))(*[c.data_ptr() for c in xkv]))
        self.ld_seen = 0 if ctl is None else ctl.ld_seen
        self.bad_cap = 0 if rules is None else rules.ld_bad
        self.flags = (L.SESSION_CTL if ctl is not None else 0) | (L.SESSION_RULES if rules is not None else 0)
        self.c = L.SessionState(self._keep[10], self._keep[11], len(kv), self.row_bytes, k0.stride(0) * es, k0.stride(1) * es,
                                x0.stride(0) * es, x0.stride(1) * es, mb, self.max_len, self.cap_max, lens.data_ptr(),
                                cap_lens.data_ptr(), stop_lens.data_ptr(), finished.data_ptr(), row_ids.data_ptr(),
                                row_steps.data_ptr(), None if ctl is None else C.pointer(ctl),
                                None if rules is None else C.pointer(rules))

    def bytes(self, rows: int, cap_rows: int, flags: int) -> int:
        return session_bytes(self.n_layer, self.row_bytes, rows, cap_rows, self.ld_seen, self.bad_cap, flags)

    def header(self, rows: int, cap_rows: int, flags: int) -> L.SessionHdr:
        return session_header(self.n_layer, self.row_bytes, rows, cap_rows, self.ld_seen, self.bad_cap, flags)


def session_meta(slots, rows, cap_rows, blobs, flags, device) -> torch.Tensor:
    """The device meta of a save or a load: int64 [ERGM_SESSION_META_ROWS, n_seq], slot | rows | cap_rows | blob address
    | flags | blob bytes; one copy to the device."""
    return torch.tensor([list(slots), list(rows), list(cap_rows), [b.data_ptr() for b in blobs], list(flags),
                         [b.numel() for b in blobs]], dtype=torch.int64).to(device)


def _session_blobs(blobs):
    for b in blobs:
        _need_gpu(b)
        assert b.dtype == torch.uint8 and b.is_contiguous()
    n = len(blobs)
    return (C.c_void_p * n)(*[b.data_ptr() for b in blobs]), (C.c_size_t * n)(*[b.numel() for b in blobs])


def slots_save(state: SessionState, slots, rows, cap_rows, flags, blobs=None, meta=None):
    """Pack the slots' state into one blob each and leave the slots idle (ergm_slots_save): ``slots`` / ``rows`` /
    ``cap_rows`` / ``flags`` host ints per session, ``blobs`` uint8 tensors of at least ``state.bytes(...)`` each
    (default: allocated here, on the current stream).  Returns the blobs."""
    n = len(slots)
    slots, rows, cap_rows, flags = ([int(v) for v in x] for x in (slots, rows, cap_rows, flags))
    if not (n == len(rows) == len(cap_rows) == len(flags)) or n < 1:
        raise ValueError("slots_save takes one row count, one caption row count and one flag word per slot")
    if blobs is None:
        blobs = [torch.empty(state.bytes(r, c, f), dtype=torch.uint8, device=state.device) for r, c, f in zip(rows, cap_rows, flags)]
    if len(blobs) != n:
        raise ValueError("slots_save takes one blob per slot")
    ptrs, sizes = _session_blobs(blobs)
    if meta is None:
        meta = session_meta(slots, rows, cap_rows, blobs, flags, state.device)
    assert meta.dtype == torch.int64 and meta.is_contiguous() and meta.shape == (L.SESSION_META_ROWS, n) and meta.is_cuda
    arr = lambda v: (C.c_int * n)(*v)
    L.call("ergm_slots_save", C.byref(state.c), n, arr(slots), arr(rows), arr(cap_rows), arr(flags), ptrs, sizes, _ptr(meta),
           _stream(state.device))
    return blobs


def slots_load(state: SessionState, slots, hdrs, blobs, row_ids=None, meta=None):
    """Unpack blobs into slots and leave the slots parked (ergm_slots_load): ``hdrs`` the host's ``SessionHdr`` of every
    blob, ``row_ids`` (int32 [n_seq] on the device, uint32 bits; optional) the ids the sessions draw under in place of
    the ones they were saved with."""
    n = len(slots)
    slots = [int(s) for s in slots]
    if not (n == len(hdrs) == len(blobs)) or n < 1:
        raise ValueError("slots_load takes one header and one blob per slot")
    ptrs, sizes = _session_blobs(blobs)
    if meta is None:
        meta = session_meta(slots, [h.rows for h in hdrs], [h.cap_rows for h in hdrs], blobs, [h.flags for h in hdrs],
                            state.device)
    assert meta.dtype == torch.int64 and meta.is_contiguous() and meta.shape == (L.SESSION_META_ROWS, n) and meta.is_cuda
    if row_ids is not None:
        _need_gpu(row_ids)
        assert row_ids.dtype == torch.int32 and row_ids.is_contiguous() and row_ids.numel() == n
    L.call("ergm_slots_load", C.byref(state.c), n, (C.c_int * n)(*slots), (L.SessionHdr * n)(*hdrs), ptrs, sizes, _ptr(row_ids),
           _ptr(meta), _stream(state.device))


def feat_pool(x: torch.Tensor, lengths: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """Mean over frames of encoder outputs x [B, T, D] (f32 / bf16, any row strides with unit
    last-dim stride) -> [B, D] f32; ``lengths`` [B] int32 limits each sample to its valid frames.

    The reference featurises offline (data_process/feature_extraction.py): wav2vec2-base-960h and BLIP-vision
    ``last_hidden_state`` outputs ([1, T_audio, 768] / [1, 197, 768]) mean-pooled over frames / patches
    (``torch.mean(features, dim=1)``, :63 and :69) into the 768-d vectors the model adds at positions 0 and 1
    (src/model.py:495-498).  The encoders download from the network and are out of scope; this pools encoder
    outputs already in HBM for a whole batch in one HIP kernel (``ergm_feat_pool``), padded audio included, so they
    feed the model (and at config 5 its projection GEMMs) without a host round trip."""
    _need_gpu(x)
    if x.dim() != 3 or x.stride(2) != 1:
        raise ValueError("feat_pool expects [B, T, D] with contiguous feature rows")
    B, T, D = x.shape
    if out is None:
        out = torch.empty(B, D, dtype=torch.float32, device=x.device)
    if lengths is not None:
        lengths = lengths.to(x.device, torch.int32).contiguous()
    dt = L.BF16 if x.dtype == torch.bfloat16 else L.F32
    L.call("ergm_feat_pool", _ptr(x), dt, B, T, D, x.stride(1), x.stride(0), _ptr(lengths), _ptr(out), out.stride(0),
           _stream(x.device))
    return out


def embed_bwd(ids, tt, cap_ids, dh0, dcap, dwte, dwpe):
    B, S = ids.shape
    V, E = dwte.shape
    lib = L.load()
    wsb = lib.ergm_embed_bwd_workspace_size(B * S)
    ws = torch.empty(wsb, dtype=torch.uint8, device=ids.device)
    L.call("ergm_embed_bwd", _ptr(ids), _ptr(tt), _ptr(cap_ids), _ptr(dh0), _ptr(dcap), _ptr(dwte), _ptr(dwpe),
           _ptr(ws), wsb, B, S, E, V, _stream(ids.device))


def count_valid(labels, emotion_labels=None, V: int = 2 ** 31 - 1, C_emo: int = 7):
    """int32 [2] on the device: valid LM labels (s >= 1, 0 <= y < V) and valid emotion labels."""
    B, S = labels.shape
    out = torch.empty(2, dtype=torch.int32, device=labels.device)
    L.call("ergm_count_valid", _ptr(labels), _ptr(emotion_labels), B, S, V, C_emo, _ptr(out), _stream(labels.device))
    return out


def xent(logits, labels, n_valid, V, with_grad=True):
    """logits: [B*S, ldl] bf16.  Returns (row_loss[B*S], dlogits or None)."""
    B, S = labels.shape
    rl = torch.empty(B * S, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if with_grad else None
    L.call("ergm_xent_fwd_bwd", _ptr(logits), logits.stride(0), _ptr(labels), _ptr(n_valid), _ptr(rl), _ptr(dl), B, S, V,
           1.0, _stream(logits.device))
    return rl, dl


def lm_rows(labels, V):
    """The rows the LM loss scores (ergm_lm_rows): (rows int32 [B*S], pos int32 [B*S], counts int32 [2] = n, n
    rounded up to 64), all on the device."""
    B, S = labels.shape
    dev = labels.device
    rows = torch.empty(B * S, dtype=torch.int32, device=dev)
    pos = torch.empty(B * S, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    L.call("ergm_lm_rows", _ptr(labels), B, S, V, _ptr(rows), _ptr(pos), _ptr(counts), _stream(dev))
    return rows, pos, counts


def xent_compact(logits, labels, n_valid, V, pos, counts, out=None):
    """ergm_xent_compact: (row_loss [B*S], dlogits_c [B*S rounded up to 64, ldl]) with the gradient row of scored
    row t at row pos[t] and zero rows from counts[0] to counts[1]; the other rows of ``out`` are left as they are."""
    B, S = labels.shape
    rl = torch.empty(B * S, dtype=torch.float32, device=logits.device)
    if out is None:
        out = torch.empty((B * S + 63) // 64 * 64, logits.stride(0), dtype=torch.bfloat16, device=logits.device)
    assert out.shape[0] >= (B * S + 63) // 64 * 64 and out.stride(0) == logits.stride(0)
    L.call("ergm_xent_compact", _ptr(logits), logits.stride(0), _ptr(labels), _ptr(n_valid), _ptr(rl), _ptr(out),
           _ptr(pos), _ptr(counts), B, S, V, _stream(logits.device))
    return rl, out


def emotion_head(h, W, labels, B, S, n_valid=None, dh=None, grad_scale=None):
    """``n_valid``: device int32 count of valid labels (default: counted from ``labels``)."""
    E = h.shape[-1]
    Cn = W.shape[0]
    logits = torch.empty(B, Cn, dtype=torch.float32, device=h.device)
    loss_sum = torch.empty(1, dtype=torch.float32, device=h.device)
    dW = torch.empty_like(W) if dh is not None else None
    scratch = torch.empty(B * (Cn + 1), dtype=torch.float32, device=h.device)
    if labels is not None and n_valid is None:
        n_valid = ((labels >= 0) & (labels < Cn)).sum().to(torch.int32).reshape(1)
    L.call("ergm_emotion_head", _ptr(h), _ptr(W), _ptr(labels), _ptr(logits), _ptr(loss_sum), _ptr(dW), _ptr(dh),
           _ptr(scratch), B, S, E, Cn, _ptr(n_valid), _ptr(grad_scale), _stream(h.device))
    return logits, loss_sum, dW


def adamw_step(p, g, m, v, p_bf16, lr, beta1, beta2, eps, weight_decay, step, max_blocks=0):
    """One torch.optim.AdamW step (flat fp32 buffers), bias corrections formed in double like torch.
    ``max_blocks`` > 0 caps the grid (for updates overlapped with other work)."""
    import math
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    L.call("ergm_adamw_step", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), p.numel(), lr, beta1, beta2, eps,
           weight_decay, lr / bc1, math.sqrt(bc2), int(max_blocks), _stream(p.device))


def adamw_rows(p, g, m, v, p_bf16, row_len, row_flag, select, lr, beta1, beta2, eps, weight_decay, step,
               max_blocks=0):
    """``adamw_step`` restricted to rows r of the [numel/row_len, row_len] block with
    (row_flag[r] != 0) == select (row_flag: a uint8 tensor or a raw device pointer)."""
    import math
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    rows = p.numel() // row_len
    flag = C.c_void_p(row_flag) if isinstance(row_flag, int) else _ptr(row_flag)
    L.call("ergm_adamw_rows", _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(p_bf16), rows, row_len, flag, int(select), lr,
           beta1, beta2, eps, weight_decay, lr / bc1, math.sqrt(bc2), int(max_blocks), _stream(p.device))


def cast_bf16(src, dst):
    L.call("ergm_cast_bf16", _ptr(src), _ptr(dst), src.numel(), _stream(src.device))


def axpy(x, y, alpha=1.0):
    L.call("ergm_axpy", _ptr(x), _ptr(y), x.numel(), alpha, _stream(x.device))
