"""Every GEMM tile configuration (kCfgs of gemm.hip) against fp64: per epilogue, K depth and ragged edge, the bias
gradient's column sums, the device-extent kernels and the dropout placement.

How a case is built (all of it on the CPU from a seeded generator, operands rounded to bf16, the reference fp64 on
the rounded values):
* every operand lives at row 8 of a larger buffer whose rows are ``round8(extent) + 24`` elements long; everything
  around it is NaN, the [M, round8(M)) tail of an m-contiguous operand included, so a value the kernel may read but
  must not use shows up as a NaN in the output;
* every output, ``aux`` and ``aux_out`` is the [M][N] view at row 8, column 8 of an [M+16][N+24(+extra)] buffer filled
  with a finite sentinel, the view itself NaN before the call; afterwards the surround must still hold the sentinel
  bit for bit and the view no NaN;
* before each call ergm_gemm_plan must report the configuration and split the case means to run, so a case cannot
  pass on the register-staged kernel by accident; the split-K workspace is NaN-filled with a tail that must stay NaN.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from ergm_amd import _lib as L
from ergm_amd import ops
from oracle import philox as X

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -12288.0  # exact in bf16 and f32
U32, U16 = 2.0 ** -24, 2.0 ** -8
N_CFGS = 47  # ergm_gemm_cfg_count(); tests/test_gemm_plan.py pins it
DYN_CFGS = (0, 2, 6, 14)  # built for device-side extents
WORST = {}  # test name -> largest err/bound it saw


def bound(ref, T, K, out_bf16):
    """Elementwise error bound of one GEMM output: ``u_out*|ref| + 2*K*u32*T``.

    Derivation.  The operands are bf16, so every product a*b is exact in fp32 (8 + 8 significand bits).  Summing K
    exact terms in fp32 in ANY order is off by at most (K-1)*u32*sum|a*b| <= K*u32*Q to first order (Higham,
    Accuracy and Stability, eq. 4.4, u32 = 2^-24 the fp32 unit roundoff, Q = |A|@|B|).  MFMA does not specify its
    internal summation order or whether it rounds per term, and split-K / intra-workgroup split-K add the partial
    sums in a few more fp32 additions (at most ``split`` + 1 more terms, each bounded by the same Q): twice the
    any-order bound, 2*K*u32*Q, covers both.  The epilogue then does a handful (< 10 <= K) of fp32 operations on
    values of magnitude at most T: alpha*Q (the scaled sum) plus |bias| plus |resid| where they are added, the whole
    times |aux| where GELU_BWD multiplies by it, plus 1 for the two GELU outputs (gelu_new and gelu_new' have Lipschitz
    constants 1.13 and 0.8 < 2, so the error of the pre-activation passes through within the factor 2, and tanhf's
    few-ulp error enters on quantities of magnitude <= 1 + |z|).  Each such operation adds at most u32*T, which the
    slack between (K-1) and 2*K absorbs for K >= 10 (K >= 64 here; the K = 1 case below is exact products).  Finally
    the result is rounded once to the output type: u_out*|ref| with u_out the unit roundoff of the type, 2^-24 for
    f32 and 2^-8 for bf16 (8 significand bits).  The kernel rounds an fp32 value that already carries the error E
    above, so it may land on the other side of a rounding boundary: |got - ref| <= u_out*(|ref| + E) + E, and the
    u_out*E is again within the factor 2.  A correctly rounded bf16 result alone therefore reaches err/bound close to
    1; a wrong element is off by orders of magnitude.  Nothing here is measured from the kernels; the plain-float32
    self-check (tests/test_gemm_plan.py::test_bound_admits_fp32_reference) shows a straightforward fp32 evaluation
    fits."""
    return (U16 if out_bf16 else U32) * ref.abs() + 2.0 * K * U32 * T


def check(what, got, ref, T, K, out_bf16, name=None, factor=1.0):
    """got against the fp64 ref: no NaN, every element within factor * bound(), then the relative Frobenius norm the
    older tests use as a second opinion (its threshold times the same factor).  Returns (and records under `name`) the worst err/bound (of the bound as
    derived, whatever the factor).  factor is 1 for every bf16 GEMM; the fp8 / MX cases pass the one measured for the
    block-scaled MFMA (tests/test_gpu_mx.py LP_FACTOR)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, what
    assert not torch.isnan(got).any().item(), f"{what}: NaN in the result"
    b = bound(ref, T, K, out_bf16)
    err = (got - ref).abs()
    ratio = (err / b.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    if name is not None:
        WORST[name] = max(WORST.get(name, 0.0), ratio)
    bad = err > factor * b
    if bad.any().item():
        i = [int(v[0]) for v in torch.nonzero(bad)[:1].t()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements past the bound, worst err/bound "
                             f"{ratio:.3g}, first at {i}: got {got[tuple(i)].item()!r} want {ref[tuple(i)].item()!r}")
    rel = ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()
    assert rel < factor * (6e-3 if out_bf16 else 1e-5), (what, rel)
    return ratio


def gelu64(z):
    """gelu_new and its derivative in fp64 (transformers NewGELUActivation)."""
    k0 = math.sqrt(2.0 / math.pi)
    t = torch.tanh(k0 * (z + 0.044715 * z ** 3))
    return 0.5 * z * (1.0 + t), 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * k0 * (1.0 + 3.0 * 0.044715 * z * z)


def eff_split(K, split):
    """The split ergm_gemm runs when asked for `split`: slices are whole 64-deep K steps."""
    kps = -(-(-(-K // split)) // 64) * 64
    return -(-K // kps)


def _r8(n):
    return (n + 7) // 8 * 8


# ---- the cases: CPU tensors only (shared with the float32 self-check, which needs no GPU) ---------------------------
ALPHA, ALPHA_DEV = 0.5, 0.5  # desc.alpha and the device scalar multiplied into it
C1_SHAPE = (328, 392, 192)
C2_MN, C2_KS, C2_SPLITS = (136, 72), (64, 128, 192, 320, 448, 576), (1, 2, 3)
C2_LAYOUTS = ((L.MK, L.NK), (L.MK, L.KN), (L.KM, L.KN))
C3_N, C3_MS, C3_KS = 136, (200, 100), (192, 448)
C4_T, C4_E, C4_K, C4_NS, C4_DW_M = 160, 64, 1088, (1, 65, 155), 208
C5_DROP = dict(p=0.1, seed=11, offset=2, site=7, row0=512)


@functools.lru_cache(maxsize=None)
def c1_case():
    """Logical A [M][K], B [K][N], bias, residual, the stored gelu' and the fp64 reference of every epilogue as
    name -> (ref, T, out_bf16)."""
    M, N, K = C1_SHAPE
    g = torch.Generator().manual_seed(1001)
    A = torch.randn(M, K, generator=g).bfloat16()
    B = (0.1 * torch.randn(K, N, generator=g)).bfloat16()
    bias = torch.randn(N, generator=g)
    resid = torch.randn(M, N, generator=g)
    a = ALPHA * ALPHA_DEV
    P, Q = A.double() @ B.double(), a * (A.double().abs() @ B.double().abs())
    z = a * P + bias.double()
    ge, dge = gelu64(z)
    aux = dge.bfloat16()  # what BIAS_GELU stores and GELU_BWD reads
    ab = bias.double().abs()
    refs = {"bias": (z, Q + ab, True), "gelu": (ge, Q + ab + 1.0, True), "dgelu": (dge, Q + ab + 1.0, True),
            "resid": (resid.double() + z, Q + ab + resid.double().abs(), False), "none": (a * P, Q, False),
            "none_bf16": (a * P, Q, True), "gelu_bwd": (a * P * aux.double(), Q * aux.double().abs(), True)}
    keep = torch.from_numpy(X.keep_mask(C5_DROP["seed"], C5_DROP["offset"], C5_DROP["site"], C5_DROP["p"], M, N,
                                        C5_DROP["row0"]))
    sc = 1.0 / (1.0 - C5_DROP["p"])
    refs["drop"] = (resid.double() + keep.double() * sc * z, (Q + ab) * sc + resid.double().abs(), False)
    return dict(M=M, N=N, K=K, A=A, B=B, bias=bias, resid=resid, aux=aux, keep=keep, refs=refs)


@functools.lru_cache(maxsize=None)
def c2_case(K):
    M, N = C2_MN
    g = torch.Generator().manual_seed(2000 + K)
    A, B = torch.randn(M, K, generator=g).bfloat16(), torch.randn(K, N, generator=g).bfloat16()
    return dict(M=M, N=N, K=K, A=A, B=B, ref=A.double() @ B.double(), T=A.double().abs() @ B.double().abs())


@functools.lru_cache(maxsize=None)
def c3_case(M, K):
    N = C3_N
    g = torch.Generator().manual_seed(3000 + M + K)
    Xt = (0.5 * torch.randn(K, M, generator=g)).bfloat16()   # [tokens][in]  (KM)
    dY = (0.5 * torch.randn(K, N, generator=g)).bfloat16()   # [tokens][out] (KN)
    a = ALPHA * ALPHA_DEV
    return dict(M=M, N=N, K=K, X=Xt, dY=dY, ref_w=a * (Xt.double().t() @ dY.double()),
                T_w=a * (Xt.double().abs().t() @ dY.double().abs()), ref_b=a * dY.double().sum(0),
                T_b=a * dY.double().abs().sum(0))


def _scored_rows(n, seed, T=C4_T, S=32):
    """n ascending rows among those the loss can score (s < S-1), and the -1 tail (as tests/test_gpu_lmhead_rows.py)."""
    cand = torch.tensor([t for t in range(T) if t % S < S - 1])
    pick = cand[torch.randperm(cand.numel(), generator=torch.Generator().manual_seed(seed))[:n]].sort().values
    rows = torch.full((T,), -1, dtype=torch.int32)
    rows[:n] = pick.to(torch.int32)
    return rows


@functools.lru_cache(maxsize=None)
def c4_dx_case(n):
    T, E, K = C4_T, C4_E, C4_K
    g = torch.Generator().manual_seed(4000 + n)
    A = torch.full(((T + 63) // 64 * 64, K), NAN, dtype=torch.bfloat16)  # rows at or past the count: NaN
    A[:n] = (0.1 * torch.randn(n, K, generator=g)).bfloat16()
    W = torch.randn(K, E, generator=g).bfloat16()
    return dict(n=n, A=A, W=W, rows=_scored_rows(n, 4000 + n), ref=A[:n].double() @ W.double(),
                T=A[:n].double().abs() @ W.double().abs())


@functools.lru_cache(maxsize=None)
def c4_dw_case(n):
    M, N, T = C4_DW_M, C4_E, C4_T
    n_pad, R64 = (n + 63) // 64 * 64, (T + 63) // 64 * 64
    g = torch.Generator().manual_seed(4500 + n)
    A = torch.full((R64, M), NAN, dtype=torch.bfloat16)   # [k][m]
    Bm = torch.full((R64, N), NAN, dtype=torch.bfloat16)  # [k][n]
    A[:n] = (0.1 * torch.randn(n, M, generator=g)).bfloat16()
    Bm[:n] = torch.randn(n, N, generator=g).bfloat16()
    A[n:n_pad] = 0
    Bm[n:n_pad] = 0
    return dict(n=n, n_pad=n_pad, A=A, B=Bm, ref=A[:n].double().t() @ Bm[:n].double(),
                T=A[:n].double().abs().t() @ Bm[:n].double().abs())


# ---- device-side plumbing -------------------------------------------------------------------------------------------
def operand(x, gpu):
    """The [rows][extent] bf16 storage matrix x at row 8 of a NaN buffer with rows of round8(extent) + 24 elements."""
    rows, ext = x.shape
    buf = torch.full((rows + 16, _r8(ext) + 24), NAN, dtype=torch.bfloat16)
    buf[8:8 + rows, :ext] = x
    return buf.to(gpu)[8:8 + rows, :ext]


def vector(x, gpu, dtype=torch.float32, surround=NAN, tail=8):
    """x [n] at element 8 of a 1-D buffer filled with `surround`; returns (buffer, view)."""
    n = x.numel()
    buf = torch.full((8 + n + tail,), surround, dtype=dtype)
    buf[8:8 + n] = x
    buf = buf.to(gpu)
    return buf, buf[8:8 + n]


def padded(M, N, dtype, gpu, fill=NAN, extra=0):
    """An [M][N] view at (8, 8) of a sentinel-filled [M+16][N+24+extra] buffer; the view holds `fill`."""
    buf = torch.full((M + 16, N + 24 + extra), SENT, dtype=dtype, device=gpu)
    view = buf[8:8 + M, 8:8 + N]
    if isinstance(fill, torch.Tensor):
        view.copy_(fill)
    else:
        view.fill_(fill)
    return buf, view


def surround_intact(buf, view):
    b = buf.clone()
    r0, c0 = 8, 8
    if b.dim() == 1:
        b[r0:r0 + view.numel()] = SENT
    else:
        b[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = SENT
    return bool((b == SENT).all().item())


def plan_of(d):
    cfg, split, flags = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    L.check(L.load().ergm_gemm_plan(C.byref(d), C.byref(cfg), C.byref(split), C.byref(flags)), "ergm_gemm_plan")
    return cfg.value, split.value, flags.value


def run(A, B, out, M, N, K, al, bl, expect, epi=L.EPI_NONE, alpha=1.0, alpha_dev=None, bias=None, aux=None,
        aux_out=None, bias_grad=None, dropout=None, m_count=None, k_count=None, row_map=None):
    """One ergm_gemm on padded views; `expect` = the (cfg, split) the plan must report first.  Returns the flags."""
    d = L.GemmDesc(M=M, N=N, K=K, lda=A.stride(0), ldb=B.stride(0), ldc=out.stride(0), a_layout=al, b_layout=bl,
                   c_dtype=L.BF16 if out.dtype == torch.bfloat16 else L.F32, epilogue=epi, alpha=alpha,
                   bias=ops._ptr(bias), aux=ops._ptr(aux), ld_aux=aux.stride(0) if aux is not None else 0,
                   aux_out=ops._ptr(aux_out), ld_aux_out=aux_out.stride(0) if aux_out is not None else 0,
                   alpha_dev=ops._ptr(alpha_dev), bias_grad=ops._ptr(bias_grad), m_count_dev=ops._ptr(m_count),
                   k_count_dev=ops._ptr(k_count), row_map=ops._ptr(row_map))
    if dropout is not None:
        d.dropout = C.pointer(dropout)
    lib = L.load()
    cfg, split, flags = plan_of(d)
    assert (cfg, split) == tuple(expect), f"planned cfg {cfg} split {split}, the case means {expect}"
    wsb = lib.ergm_gemm_workspace_size(C.byref(d))
    assert wsb % 4 == 0
    ws = torch.full((wsb // 4 + 1024,), NAN, dtype=torch.float32, device=A.device)
    L.check(lib.ergm_gemm(C.byref(d), ops._ptr(A), ops._ptr(B), ops._ptr(out), ops._ptr(ws), wsb,
                          ops._stream(A.device)), "ergm_gemm")
    assert torch.isnan(ws[wsb // 4:]).all().item(), "written past the workspace ergm_gemm_workspace_size asked for"
    return flags


@pytest.fixture
def tune():
    """ergm_gemm_tune for the test, reset to automatic afterwards."""
    lib = L.load()

    def force(cfg, split):
        L.check(lib.ergm_gemm_tune(cfg, split), "ergm_gemm_tune")
    try:
        yield force
    finally:
        lib.ergm_gemm_tune(-1, 0)


def report(name):
    print(f"{name}: worst err/bound {WORST.get(name, 0.0):.4f}")


# ---- C1: epilogue x configuration x split ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1_dev(gpu):
    c = c1_case()
    A, B = c["A"], c["B"]
    return dict(A_mk=operand(A, gpu), A_km=operand(A.t().contiguous(), gpu), B_kn=operand(B, gpu),
                B_nk=operand(B.t().contiguous(), gpu), bias=vector(c["bias"], gpu)[1],
                alpha_dev=torch.tensor([ALPHA_DEV], device=gpu), resid=c["resid"].to(gpu), aux=c["aux"].to(gpu))


@pytest.mark.parametrize("cfg", range(N_CFGS))
def test_epilogues_every_config(gpu, tune, c1_dev, cfg):
    """C1: BIAS, BIAS_GELU (+ its gelu' side output), BIAS_RESID (separate and in-place residual), GELU_BWD and the
    plain f32 / bf16 stores of every pipelined layout, on a shape ragged against 64 / 128 / 256 tiles with 3 K steps,
    unsplit and as an uneven 2-way split (the epilogue then runs in the split-K reduce)."""
    c, dv = c1_case(), c1_dev
    M, N, K, refs = c["M"], c["N"], c["K"], c["refs"]
    name = f"C1 cfg {cfg}"
    kw = dict(alpha=ALPHA, alpha_dev=dv["alpha_dev"])
    f32, b16 = torch.float32, torch.bfloat16

    def done(what, key, buf, view):
        ref, T, ob = refs[key]
        check(f"{name} split {split} {what}", view, ref, T, K, ob, name)
        assert surround_intact(buf, view), f"{name} split {split} {what}: wrote outside C[:M, :N]"

    for split in (1, 2):
        tune(cfg, split)
        exp = (cfg, eff_split(K, split))
        assert exp[1] == split
        # (MK, KN): the forward Conv1D GEMMs
        buf, out = padded(M, N, b16, gpu)
        run(dv["A_mk"], dv["B_kn"], out, M, N, K, L.MK, L.KN, exp, L.EPI_BIAS, bias=dv["bias"], **kw)
        done("BIAS", "bias", buf, out)
        buf, out = padded(M, N, b16, gpu)
        xbuf, xout = padded(M, N, b16, gpu, extra=16)
        run(dv["A_mk"], dv["B_kn"], out, M, N, K, L.MK, L.KN, exp, L.EPI_BIAS_GELU, bias=dv["bias"], aux_out=xout, **kw)
        done("BIAS_GELU", "gelu", buf, out)
        done("BIAS_GELU aux_out", "dgelu", xbuf, xout)
        buf, out = padded(M, N, f32, gpu)
        rbuf, res = padded(M, N, f32, gpu, fill=dv["resid"], extra=16)
        run(dv["A_mk"], dv["B_kn"], out, M, N, K, L.MK, L.KN, exp, L.EPI_BIAS_RESID, bias=dv["bias"], aux=res, **kw)
        done("BIAS_RESID", "resid", buf, out)
        assert torch.equal(res, dv["resid"]) and surround_intact(rbuf, res)
        buf, out = padded(M, N, f32, gpu, fill=dv["resid"])
        run(dv["A_mk"], dv["B_kn"], out, M, N, K, L.MK, L.KN, exp, L.EPI_BIAS_RESID, bias=dv["bias"], aux=out, **kw)
        done("BIAS_RESID in place", "resid", buf, out)
        buf, out = padded(M, N, f32, gpu)
        run(dv["A_mk"], dv["B_kn"], out, M, N, K, L.MK, L.KN, exp, **kw)
        done("NONE f32 (MK,KN)", "none", buf, out)
        # (MK, NK): the data gradients
        buf, out = padded(M, N, f32, gpu)
        run(dv["A_mk"], dv["B_nk"], out, M, N, K, L.MK, L.NK, exp, **kw)
        done("NONE f32 (MK,NK)", "none", buf, out)
        buf, out = padded(M, N, b16, gpu)
        run(dv["A_mk"], dv["B_nk"], out, M, N, K, L.MK, L.NK, exp, **kw)
        done("NONE bf16 (MK,NK)", "none_bf16", buf, out)
        buf, out = padded(M, N, b16, gpu)
        abuf, aux = padded(M, N, b16, gpu, fill=dv["aux"], extra=16)  # ld_aux != ldc
        run(dv["A_mk"], dv["B_nk"], out, M, N, K, L.MK, L.NK, exp, L.EPI_GELU_BWD, aux=aux, **kw)
        done("GELU_BWD", "gelu_bwd", buf, out)
        # (KM, KN): the weight gradients
        buf, out = padded(M, N, f32, gpu)
        run(dv["A_km"], dv["B_kn"], out, M, N, K, L.KM, L.KN, exp, **kw)
        done("NONE f32 (KM,KN)", "none", buf, out)
    report(name)


# ---- C2: K depth ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2_dev(gpu):
    dev = {}
    for K in C2_KS:
        c = c2_case(K)
        dev[K] = {L.MK: operand(c["A"], gpu), L.KM: operand(c["A"].t().contiguous(), gpu),
                  (L.KN,): operand(c["B"], gpu), (L.NK,): operand(c["B"].t().contiguous(), gpu)}
    return dev


@pytest.mark.parametrize("cfg", range(N_CFGS))
def test_k_depth_every_config(gpu, tune, c2_dev, cfg):
    """C2: 1, 2, 3, 5, 7 and 9 K steps (below, at and above every ring depth; odd and even for the intra-workgroup
    split-K's pairs) under forced splits 1, 2, 3 (uneven last slices, splits that round down), three layouts; each
    result within the bound and bitwise the same on a second run."""
    M, N = C2_MN
    name = f"C2 cfg {cfg}"
    for K in C2_KS:
        c = c2_case(K)
        for split in C2_SPLITS:
            tune(cfg, split)
            exp = (cfg, eff_split(K, split))
            for al, bl in C2_LAYOUTS:
                A, B = c2_dev[K][al], c2_dev[K][(bl,)]
                bufs = []
                for _ in range(2):
                    buf, out = padded(M, N, torch.float32, gpu)
                    run(A, B, out, M, N, K, al, bl, exp)
                    bufs.append((buf, out))
                what = f"{name} K {K} split {split} layouts ({al},{bl})"
                check(what, bufs[0][1], c["ref"], c["T"], K, False, name)
                assert surround_intact(*bufs[0]), what
                assert torch.equal(bufs[0][0].view(torch.int32), bufs[1][0].view(torch.int32)), what + ": not bitwise"
    report(name)


# ---- C3: the weight gradient's bias gradient ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c3_dev(gpu):
    dev = {}
    for M in C3_MS:
        for K in C3_KS:
            c = c3_case(M, K)
            dev[M, K] = (operand(c["X"], gpu), operand(c["dY"], gpu))
    dev["alpha_dev"] = torch.tensor([ALPHA_DEV], device=gpu)
    return dev


@pytest.mark.parametrize("cfg", range(N_CFGS))
def test_bias_gradient_every_config(gpu, tune, c3_dev, cfg):
    """C3: dW = alpha X^T dY with db = alpha sum_k dY in the same call, M ragged against every tile (and M % 8 != 0
    with a NaN tail in X's rows), N = 136 ragged against every tile width, odd K-step counts, unsplit and split:
    the in-kernel column sums where the configuration has them (plan flag bit 0), the column-sum pass otherwise."""
    N = C3_N
    name, name_b = f"C3 cfg {cfg} dW", f"C3 cfg {cfg} db"
    paths = set()
    for M in C3_MS:
        for K in C3_KS:
            c = c3_case(M, K)
            Xd, dYd = c3_dev[M, K]
            assert Xd.stride(0) == _r8(M) + 24
            for split in (1, 2):
                tune(cfg, split)
                exp = (cfg, eff_split(K, split))
                assert exp[1] == split
                what = f"C3 cfg {cfg} M {M} K {K} split {split}"
                dbs = []
                for _ in range(2):
                    buf, out = padded(M, N, torch.float32, gpu)
                    # 248 sentinel floats behind db: the widest tile's columns past N land there, not outside
                    dbuf, db = vector(torch.full((N,), NAN), gpu, surround=SENT, tail=248)
                    flags = run(Xd, dYd, out, M, N, K, L.KM, L.KN, exp, alpha=ALPHA, alpha_dev=c3_dev["alpha_dev"],
                                bias_grad=db)
                    paths.add(flags & 1)
                    dbs.append((dbuf, db))
                check(what + " dW", out, c["ref_w"], c["T_w"], K, False, name)
                assert surround_intact(buf, out), what
                got = db.double().cpu()
                assert not torch.isnan(got).any().item(), what + ": db not fully written"
                b = 2.0 * K * U32 * c["T_b"]
                err = (got - c["ref_b"]).abs()
                WORST[name_b] = max(WORST.get(name_b, 0.0), (err / b).max().item())
                assert (err <= b).all().item(), (what, "db", (err / b).max().item())
                assert surround_intact(dbuf, db), what + ": wrote outside db[:N]"
                assert torch.equal(dbs[0][0].view(torch.int32), dbs[1][0].view(torch.int32)), what + ": db not bitwise"
    assert len(paths) == 1  # one path per configuration
    print(f"C3 cfg {cfg}: {'in-kernel column sums' if paths.pop() else 'column-sum pass'}")
    report(name)
    report(name_b)


# ---- C4: device-side extents on every configuration built for them --------------------------------------------------
def _dyn_expect(cfg):
    return cfg if cfg in DYN_CFGS else 2  # any other forced configuration: the plan's own choice


@pytest.mark.parametrize("n", C4_NS)
@pytest.mark.parametrize("cfg", DYN_CFGS + (38,))
def test_device_row_count_every_built_config(gpu, tune, cfg, n):
    """C4, dX: rows past the device-side count are NaN and never used, the computed rows go through row_map into a
    zero-filled output, 2 K slices (17 K steps: 9 + 8)."""
    T, E, K = C4_T, C4_E, C4_K
    c = c4_dx_case(n)
    name = f"C4 dX cfg {cfg} n {n}"
    tune(cfg, 0)
    A, W = operand(c["A"], gpu), operand(c["W"], gpu)
    cnt = torch.tensor([n, (n + 63) // 64 * 64], dtype=torch.int32, device=gpu)
    buf, out = padded(T, E, torch.float32, gpu, fill=0.0)  # the executor's zero fill of dy
    flags = run(A, W, out, T, E, K, L.MK, L.KN, (_dyn_expect(cfg), 2), m_count=cnt[0:1], row_map=c["rows"].to(gpu))
    assert flags == 4
    got = out.cpu()
    scored = c["rows"][:n].long()
    other = torch.ones(T, dtype=torch.bool)
    other[scored] = False
    assert (got[other] == 0).all().item()
    assert torch.isfinite(got).all().item()
    check(name, got[scored], c["ref"], c["T"], K, False, name)
    assert surround_intact(buf, out), name
    report(name)


@pytest.mark.parametrize("n", C4_NS)
@pytest.mark.parametrize("cfg", DYN_CFGS + (38,))
def test_device_contraction_length_every_built_config(gpu, tune, cfg, n):
    """C4, dW: the contraction runs over the device-side padded count; operand rows past it are NaN."""
    M, N, T = C4_DW_M, C4_E, C4_T
    c = c4_dw_case(n)
    name = f"C4 dW cfg {cfg} n {n}"
    tune(cfg, 0)
    cnt = torch.tensor([n, c["n_pad"]], dtype=torch.int32, device=gpu)
    buf, out = padded(M, N, torch.float32, gpu)
    flags = run(operand(c["A"], gpu), operand(c["B"], gpu), out, M, N, T, L.KM, L.KN, (_dyn_expect(cfg), 1),
                k_count=cnt[1:2])
    assert flags == 4
    check(name, out, c["ref"], c["T"], n, False, name)  # n terms; the zero rows up to the padded count add nothing
    assert surround_intact(buf, out), name
    report(name)


# ---- C5: dropout placement ------------------------------------------------------------------------------------------
def test_dropout_placement_is_config_independent(gpu, tune, c1_dev):
    """C5: BIAS_RESID with dropout p = 0.1 on one configuration of each family and epilogue kind (staged 0,
    warp-specialised 16, LDS-free store 22, intra-workgroup split-K 33, 32x32 MFMA 38) and on the register-staged
    kernel (reached through ldc % 8 != 0): the positions where out == resid exactly are the same set everywhere,
    they contain every position the mask generator drops, and the values fit the bound with that mask."""
    c, dv = c1_case(), c1_dev
    M, N, K = c["M"], c["N"], c["K"]
    ref, T, _ = c["refs"]["drop"]
    drop = ops.dropout_desc(**C5_DROP)
    kw = dict(alpha=ALPHA, alpha_dev=dv["alpha_dev"], bias=dv["bias"], dropout=drop)
    sets = {}
    for cfg in (0, 16, 22, 33, 38, -1):
        name = f"C5 cfg {cfg}"
        tune(max(cfg, 0), 1)
        buf, out = padded(M, N, torch.float32, gpu, extra=0 if cfg >= 0 else 4)  # ldc = N + 28 for the fallback
        rbuf, res = padded(M, N, torch.float32, gpu, fill=dv["resid"], extra=16)
        run(dv["A_mk"], dv["B_kn"], out, M, N, K, L.MK, L.KN, (cfg, 1), L.EPI_BIAS_RESID, aux=res, **kw)
        check(name, out, ref, T, K, False, name)
        assert surround_intact(buf, out), name
        sets[cfg] = (out == dv["resid"]).cpu()
        report(name)
    for cfg, s in sets.items():
        assert torch.equal(s, sets[0]), cfg
    dropped = ~c["keep"]
    assert (sets[0] | ~dropped).all().item()  # every dropped position left the residual untouched
    assert 0.08 < sets[0].float().mean().item() < 0.12
