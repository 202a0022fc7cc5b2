"""Cases, fp64 references and the error bound of the ergm_linear_rows tests (CPU tensors only: the GPU test and the
float32 self-check of tests/test_decode_exec_abi.py share them).

Bound, per element: ``u_out*|ref| + 2*K*u32*T`` -- the bound of tests/test_gpu_gemm_matrix.py, whose derivation holds
here word for word (bf16 operands, exact products, K terms summed in fp32 in some order, a few fp32 epilogue
operations on magnitudes at most T, one rounding to the output type).  With the LayerNorm prologue the reference is
the UNROUNDED fp64 LayerNorm, and the bound gains ``(u16 + 4*K*u32) * (A_hat @ |W|)`` with A_hat = |gamma|*|x_hat| +
|beta|: the kernel's operand is an fp32 LayerNorm value (within K*u32-order relative error of the fp64 one for any
summation order of a two-pass variance) rounded once to bf16 (within u16 of it, whichever neighbour it picks).

Second opinion, the relative Frobenius norm: tests/test_gpu_gemm_matrix.py's 6e-3 for a bf16 output and 1e-5 for an
f32 output.  The 1e-5 was set for a reference that shares the kernel's operands, and it stays for every call without
the prologue.  With the prologue the kernel's operand is the reference's rounded once to bf16, so an f32 result carries
the error of one bf16 rounding, the very error the 6e-3 gate was set for: the gate for an f32 output with the prologue
is 6e-3 as well (a plain float32 evaluation sits at 1.6e-3 there, tests/test_decode_exec_abi.py, so 1e-5 cannot be met
by any implementation that rounds the operand to bf16, and 6e-3 can).  Nothing here is measured from the kernel."""
import functools
import math

import torch

from ergm_amd import _lib as L

U32, U16 = 2.0 ** -24, 2.0 ** -8
SENT = -12288.0  # exact in bf16 and f32
EPS = 1e-5
MS = (1, 15, 16, 17, 32, 33)
MMAX = max(MS)
# (K, N, weight layout): one K step; a K split with idle waves; ragged N; the E x E shape; the deep contraction; NK
SHAPES = ((64, 72, L.KN), (192, 128, L.KN), (128, 384, L.KN), (768, 768, L.KN), (3072, 768, L.KN), (768, 512, L.NK))
EPILOGUES = {"none": L.EPI_NONE, "bias": L.EPI_BIAS, "gelu": L.EPI_BIAS_GELU, "resid": L.EPI_BIAS_RESID}


def gelu64(z):
    k0 = math.sqrt(2.0 / math.pi)
    return 0.5 * z * (1.0 + torch.tanh(k0 * (z + 0.044715 * z ** 3)))


def epilogues_of(layout):
    return tuple(EPILOGUES) if layout == L.KN else ("none", "resid")


@functools.lru_cache(maxsize=None)
def case(K, N, layout):
    """Inputs for MMAX rows (a call on M rows uses the first M) and, per (prologue, epilogue), the fp64 reference as
    (ref, T, out_bf16, extra): extra = the prologue's term of the bound."""
    g = torch.Generator().manual_seed(7000 + K + N)
    scale = 0.1 * 100.0 ** torch.rand(MMAX, 1, generator=g)           # per row, in [0.1, 10]
    x = ((0.5 + torch.randn(MMAX, K, generator=g)) * scale).float()
    gamma = (1.0 + 0.2 * torch.randn(K, generator=g)).float()
    beta = (0.2 * torch.randn(K, generator=g)).float()
    W = (0.1 * torch.randn(K, N, generator=g)).bfloat16()             # logical [K][N]
    bias = torch.randn(N, generator=g).float()
    resid = torch.randn(MMAX, N, generator=g).float()
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    xh = (xd - mu) / torch.sqrt(var + EPS)
    a_ln = xh * gamma.double() + beta.double()                        # the unrounded fp64 LayerNorm
    a_hat = gamma.double().abs() * xh.abs() + beta.double().abs()
    A = a_ln.bfloat16()                                               # the operand of the calls without the prologue
    Wd = W.double()
    refs = {}
    for ln in (False, True):
        a, qa = (a_ln, a_hat) if ln else (A.double(), A.double().abs())
        P, Q = a @ Wd, qa @ Wd.abs()
        z, ab, rd = P + bias.double(), bias.double().abs(), resid.double()
        extra = (U16 + 4.0 * K * U32) * Q if ln else torch.zeros_like(Q)
        for name, (ref, T, ob) in {"none": (P, Q, False), "bias": (z, Q + ab, True), "gelu": (gelu64(z), Q + ab + 1.0, True),
                                   "resid": (rd + z, Q + ab + rd.abs(), False)}.items():
            refs[(ln, name)] = (ref, T, ob, extra)
    return dict(K=K, N=N, layout=layout, x=x, gamma=gamma, beta=beta, A=A, W=W,
                W_stored=W if layout == L.KN else W.t().contiguous(), bias=bias, resid=resid, refs=refs)


def bound(ref, T, K, out_bf16, extra):
    return (U16 if out_bf16 else U32) * ref.abs() + 2.0 * K * U32 * T + extra


def frob_gate(out_bf16, ln):
    return 6e-3 if out_bf16 or ln else 1e-5


def check(what, got, c, ln, epi, M):
    """``got`` [M, N] against the first M rows of the fp64 reference: finite, every element within the bound, the
    Frobenius gate.  Prints nothing; returns (worst err/bound, rel Frobenius)."""
    ref, T, ob, extra = (t[:M] if torch.is_tensor(t) else t for t in c["refs"][(ln, epi)])
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, what
    assert torch.isfinite(got).all().item(), f"{what}: non-finite value in the result"
    b = bound(ref, T, c["K"], ob, extra)
    err = (got - ref).abs()
    ratio = (err / b.clamp_min(1e-300)).max().item()
    bad = err > b
    if bad.any().item():
        i = [int(v[0]) for v in torch.nonzero(bad)[:1].t()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements past the bound, worst err/bound "
                             f"{ratio:.3g}, first at {i}: got {got[tuple(i)].item()!r} want {ref[tuple(i)].item()!r}")
    rel = ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()
    assert rel < frob_gate(ob, ln), (what, rel, frob_gate(ob, ln))
    return ratio, rel
