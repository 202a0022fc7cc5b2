"""MX-fp8 (OCP microscaling) path of config 5 on the GPU, through the C-ABI: e4m3fn elements with an e8m0
scale per 32-element K block, consumed by v_mfma_scale_f32_16x16x128_f8f6f4 itself.

* quantisers (rows; weights into their transpose and, for the fp8 data-gradient GEMMs, their row form): bit-exact
  against a torch restatement of the rule
  (block exponent e = the smallest integer with max|block| <= 448·2^e, from the bits of the maximum; values
  scaled by 2^-e exactly, then torch's float8_e4m3fn cast: round to nearest even);
* ergm_gemm_mx: exact MX inputs with random block scales, f32 accumulation -> against an fp64 product of the
  dequantised operands (rel 5e-5), every tile configuration, ragged M / N;
* the GELU / GELU' epilogues' MX copy of their bf16 output is bit-identical to quantising that output afterwards.
* ergm_gemm_f8 and ergm_gemm_mx per element against fp64 with the GEMM matrix's derived bound, every tile
  configuration, on a shape ragged against every tile, 1 / 2 / 3 / 5 K steps, operands and scales inside NaN buffers.
Scales travel in the library's K-step-major layout (ops.mx_tile / mx_untile convert).
The model-level fp8 gates (tests/test_gpu_c5.py) run on this path by default (ERGM_FP8_MX=1).
"""
import functools

import pytest
import torch

import test_gpu_gemm_matrix as G
from ergm_amd import _lib as L
from ergm_amd import ops

pytestmark = pytest.mark.gpu
E4M3 = torch.float8_e4m3fn


def mx_ref(X: torch.Tensor):
    """(Q [R, C] uint8, S [R, C/32] uint8) of rows X [R, C] (C % 32 == 0)."""
    X = X.float()
    R, Cc = X.shape
    Xb = X.reshape(R, Cc // 32, 32)
    am = Xb.abs().amax(-1).contiguous()
    bits = am.view(torch.int32)
    ea = ((bits >> 23) & 0xFF) - 127
    e = ea - 8 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    eb = torch.where(am == 0, torch.full_like(e, 127), (e + 127).clamp(0, 254))
    inv = torch.pow(2.0, (127 - eb).double()).float()
    q = (Xb * inv[..., None]).clamp(-448, 448).to(E4M3)
    return q.view(torch.uint8).reshape(R, Cc), eb.to(torch.uint8)


def mx_dequant(Q: torch.Tensor, S: torch.Tensor) -> torch.Tensor:
    R, Cc = Q.shape
    v = Q.view(E4M3).double().reshape(R, Cc // 32, 32)
    return (v * torch.pow(2.0, S.double() - 127)[..., None]).reshape(R, Cc)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,cols,ld", [(64, 1024, 1032), (37, 4096, 4104), (5, 96, 104)])
def test_quant_rows_mx_bit_exact(gpu, dtype, rows, cols, ld):
    g = torch.Generator().manual_seed(rows + cols)
    X = torch.randn(rows, ld, generator=g) * torch.logspace(-3, 2, rows)[:, None]
    X[0] = 0.0                      # zero blocks -> scale 1
    X[1, :32] = 448.0 * 2.0 ** -3   # a block whose maximum is exactly 448·2^e
    X[1, 32:64] = 1.8               # mantissa above 1.75: the next exponent up
    X = X.to(dtype)
    q, s = ops.quant_rows_mx(X.to(gpu), cols)
    rq, rs = mx_ref(X[:, :cols])
    s = ops.mx_untile(s.cpu(), rows, cols // 32)
    assert torch.equal(s, rs)
    assert torch.equal(q.cpu(), rq)
    # no element saturates and the dequantised values are within e4m3's half-ulp (2^-4 relative)
    deq = mx_dequant(q.cpu(), s)
    ref = X[:, :cols].double()
    assert ((deq - ref).abs() <= ref.abs() * 2.0 ** -4 + 2.0 ** -9 * ref.abs().amax()).all()


@pytest.mark.parametrize("K,N", [(1024, 3072), (4096, 1024), (128, 192)])
def test_quant_weight_mx_bit_exact(gpu, K, N):
    g = torch.Generator().manual_seed(K + N)
    W = torch.randn(K, N, generator=g) * 0.02
    W[:, 5] = 0.0
    W[:32, 7] *= 1000.0
    W[9, 64:96] = 0.0
    W = W.bfloat16()
    Wt, s, Wr, sr = ops.quant_weight_mx(W.to(gpu), row_form=True)
    rq, rs = mx_ref(W.t().contiguous())
    assert torch.equal(ops.mx_untile(s.cpu(), N, K // 32), rs)
    assert torch.equal(Wt.cpu(), rq)
    rq, rs = mx_ref(W)  # the row form: W's rows along N
    assert torch.equal(ops.mx_untile(sr.cpu(), K, N // 32), rs)
    assert torch.equal(Wr.cpu(), rq)


def _mx_operand(rows, K, g):
    q = (torch.randn(rows, K, generator=g) * 3.0).clamp(-448, 448).to(E4M3).view(torch.uint8)
    s = torch.randint(120, 135, (rows, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    return q, s


N_F8_CFGS = 5  # kF8Cfgs in gemm.hip (shared by the MX kernel)


@pytest.mark.parametrize("cfg", [-1] + list(range(N_F8_CFGS)))
@pytest.mark.parametrize("M,N,K", [(256, 384, 512), (200, 136, 256), (2048, 1024, 1024), (64, 4096, 128)])
def test_gemm_mx_matches_fp64(gpu, cfg, M, N, K):
    lib = L.load()
    g = torch.Generator().manual_seed(M + N + K + cfg)
    A8, sa = _mx_operand(M, K, g)
    B8, sb = _mx_operand(N, K, g)
    ref = mx_dequant(A8, sa) @ mx_dequant(B8, sb).t()
    try:
        L.check(lib.ergm_gemm_f8_tune(cfg), "tune")
        out = ops.gemm_mx(A8.to(gpu), ops.mx_tile(sa).to(gpu), B8.to(gpu), ops.mx_tile(sb, N + 8).to(gpu))
        torch.cuda.synchronize()
    finally:
        lib.ergm_gemm_f8_tune(-1)
    err = ((out.double().cpu() - ref).norm() / ref.norm()).item()
    assert err < 5e-5, err


def test_gemm_mx_epilogues_and_gelu_mx_copy(gpu):
    M, N, K = 512, 1024, 768
    g = torch.Generator().manual_seed(3)
    A8, sa = _mx_operand(M, K, g)
    B8, sb = _mx_operand(N, K, g)
    sa = (sa.int() - 8).to(torch.uint8)  # keep the products O(1) for the GELU
    sb = (sb.int() - 8).to(torch.uint8)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    v = mx_dequant(A8, sa) @ mx_dequant(B8, sb).t() + bias.double()
    dev = lambda t: t.to(gpu)  # noqa: E731
    a8, b8, xa, xb = dev(A8), dev(B8), dev(ops.mx_tile(sa)), dev(ops.mx_tile(sb))
    out = ops.gemm_mx(a8, xa, b8, xb, epilogue=L.EPI_BIAS_RESID, bias=dev(bias), aux=dev(res))
    assert ((out.double().cpu() - (v + res.double())).norm() / (v + res.double()).norm()).item() < 5e-5
    pre = torch.empty(M, N, dtype=torch.bfloat16, device=gpu)
    act = torch.empty(M, N + 8, dtype=torch.bfloat16, device=gpu)[:, :N]
    q = torch.empty(M, N, dtype=torch.uint8, device=gpu)
    qs = torch.empty(N // 128, M + 16, 4, dtype=torch.uint8, device=gpu)
    ops.gemm_mx(a8, xa, b8, xb, out=act, epilogue=L.EPI_BIAS_GELU, bias=dev(bias), aux_out=pre, q_out=q, q_sc=qs)
    vv = v.clone().requires_grad_(True)
    gelu = 0.5 * vv * (1 + torch.tanh((2 / torch.pi) ** 0.5 * (vv + 0.044715 * vv ** 3)))
    gelu.sum().backward()
    gelu = gelu.detach()
    assert (pre.double().cpu() - vv.grad).abs().max().item() <= 8e-3 * vv.grad.abs().max().item()
    assert (act.double().cpu() - gelu).abs().max().item() <= 8e-3 * gelu.abs().max().item()
    # the epilogue's MX copy is exactly the MX quantisation of the bf16 output it stored
    rq, rs = mx_ref(act.cpu())
    assert torch.equal(ops.mx_untile(qs.cpu(), M, N // 32), rs)
    assert torch.equal(q.cpu(), rq)
    outb = ops.gemm_mx(a8, xa, b8, xb, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS, bias=dev(bias))
    assert ((outb.double().cpu() - v).norm() / v.norm()).item() < 4e-3
    # GELU' (the fp8 data-gradient path's mlp c_proj dX): C = (A·Bᵀ) · aux, with the MX copy of C for the c_fc dX
    dg = (torch.rand(M, N, generator=g) * 1.2 - 0.1).bfloat16()
    gb = torch.empty(M, N, dtype=torch.bfloat16, device=gpu)
    ops.gemm_mx(a8, xa, b8, xb, out=gb, epilogue=L.EPI_GELU_BWD, aux=dev(dg), q_out=q, q_sc=qs)
    vb = (v - bias.double()) * dg.double()
    assert ((gb.double().cpu() - vb).norm() / vb.norm()).item() < 4e-3
    rq, rs = mx_ref(gb.cpu())
    assert torch.equal(ops.mx_untile(qs.cpu(), M, N // 32), rs)
    assert torch.equal(q.cpu(), rq)


# ---- per element: both low-precision GEMMs, every tile configuration -------------------------------------------------
# M x N is ragged against every tile from 64 to 256 in both dimensions; K = 1, 2, 3 and 5 steps of 128 is, for the
# rings of 2, 3 and 4 stages, fewer steps than the prologue issues, exactly the prologue, and a refill.  The bound is
# the matrix's (test_gpu_gemm_matrix.bound): e4m3 values times power-of-two scales multiply exactly in fp32, so its
# derivation holds as it stands, with K the element count of the contraction, IF the block-scaled MFMA keeps full
# fp32 accumulation inside its 128-deep step.  It does not: at the commit before these cases existed, and bit for bit
# the same after it, the worst err/bound is 2.42 (MX, K = 128; fp8 with unit scales 1.15 at K = 128), falling with K
# (0.87 at 256, 0.59 at 384, 0.35 at 640) as the derived bound grows and the per-step error does not
# (profiles/r16_lowp_bound.txt).  A property of v_mfma_scale_f32_16x16x128_f8f6f4, not of the kernels, so the bound
# carries a factor of twice the measured worst; a wrong scale row or a leaked NaN is off by orders of magnitude.  The
# same factor scales check()'s relative-norm second opinion (1e-5 for f32 out; measured 1.44e-5 in both trees), to
# 4.85e-5: what the older norm tests above gate these kernels with (5e-5).
LP_FACTOR = 2 * 2.425
LP_M, LP_N, LP_KS, LP_K_EPI, LP_N_GELU = 200, 136, (128, 256, 384, 640), 384, 160
NAN8, NANS = 0x7F, 0xFF  # the e4m3fn NaN byte; the e8m0 NaN


@functools.lru_cache(maxsize=None)
def lowp_case(mx, K, N=LP_N):
    """CPU operands of one low-precision case and its fp64 references: name -> (ref, T, out_bf16)."""
    g = torch.Generator().manual_seed(7000 + K + N + (1 if mx else 0))
    M = LP_M
    A8 = (torch.randn(M, K, generator=g) * 3.0).clamp(-448, 448).to(E4M3).view(torch.uint8)
    B8 = (torch.randn(N, K, generator=g) * 3.0).clamp(-448, 448).to(E4M3).view(torch.uint8)
    c = dict(M=M, N=N, K=K, A8=A8, B8=B8)
    if mx:  # 2^-8 .. 2^-1 per 32-element block: the products stay O(1) for the GELU
        c["sa"] = torch.randint(119, 127, (M, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
        c["sb"] = torch.randint(119, 127, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
        A, B = mx_dequant(A8, c["sa"]), mx_dequant(B8, c["sb"])
    else:   # power-of-two row / column scales: the epilogue's two multiplications are exact
        c["sa"] = torch.pow(2.0, torch.randint(-6, -1, (M,), generator=g).float())
        c["sb"] = torch.pow(2.0, torch.randint(-6, -1, (N,), generator=g).float())
        A = A8.view(E4M3).double() * c["sa"].double()[:, None]
        B = B8.view(E4M3).double() * c["sb"].double()[:, None]
    c["bias"] = torch.randn(N, generator=g)
    c["resid"] = torch.randn(M, N, generator=g)
    P, Q = A @ B.t(), A.abs() @ B.abs().t()
    z, ab = P + c["bias"].double(), c["bias"].double().abs()
    ge, dge = G.gelu64(z)
    c["refs"] = {"none": (P, Q, False), "resid": (c["resid"].double() + z, Q + ab + c["resid"].double().abs(), False),
                 "gelu": (ge, Q + ab + 1.0, True), "dgelu": (dge, Q + ab + 1.0, True)}
    return c


def _bytes_in_nan(x, gpu):
    """The [rows][K] e4m3 matrix x at (8, 16) of a buffer of e4m3 NaN bytes (16-byte aligned, pitch K + 32)."""
    rows, K = x.shape
    buf = torch.full((rows + 16, K + 32), NAN8, dtype=torch.uint8)
    buf[8:8 + rows, 16:16 + K] = x
    return buf.to(gpu)[8:8 + rows, 16:16 + K]


def _scales_in_nan(s, gpu):
    """[rows][K/32] block scales in the library layout with a pitch of rows + 8, between two planes of e8m0 NaN and
    with NaN in the pitch's spare rows."""
    rows = s.shape[0]
    t = ops.mx_tile(s, rows + 8)
    t[:, rows:] = NANS
    buf = torch.full((t.shape[0] + 2, rows + 8, 4), NANS, dtype=torch.uint8)
    buf[1:-1] = t
    return buf.to(gpu)[1:-1]


def lowp_launches(gpu, mx, cfg):
    """Every launch of the per-element cases for one kernel form and tile configuration: yields (what, case, key,
    buffer, view) after each, the forced configuration reset at the end."""
    lib = L.load()
    f32, b16 = torch.float32, torch.bfloat16
    try:
        L.check(lib.ergm_gemm_f8_tune(cfg), "tune")
        for K in LP_KS:
            c = lowp_case(mx, K)
            M, N = c["M"], c["N"]
            a8, b8 = _bytes_in_nan(c["A8"], gpu), _bytes_in_nan(c["B8"], gpu)
            if mx:
                xa, xb = _scales_in_nan(c["sa"], gpu), _scales_in_nan(c["sb"], gpu)
                gemm = functools.partial(ops.gemm_mx, a8, xa, b8, xb)
            else:
                gemm = functools.partial(ops.gemm_f8, a8, G.vector(c["sa"], gpu)[1], b8, G.vector(c["sb"], gpu)[1])
            buf, out = G.padded(M, N, f32, gpu)
            gemm(out=out)
            yield f"K {K} NONE", c, "none", buf, out
            if K != LP_K_EPI:
                continue
            bias = G.vector(c["bias"], gpu)[1]
            buf, out = G.padded(M, N, f32, gpu)
            rbuf, res = G.padded(M, N, f32, gpu, fill=c["resid"].to(gpu), extra=16)
            gemm(out=out, epilogue=L.EPI_BIAS_RESID, bias=bias, aux=res)
            yield f"K {K} BIAS_RESID", c, "resid", buf, out
            if not mx:
                continue
            c = lowp_case(True, K, LP_N_GELU)  # the MX copy of the output needs whole 32-column blocks
            N = c["N"]
            a8, b8 = _bytes_in_nan(c["A8"], gpu), _bytes_in_nan(c["B8"], gpu)
            xa, xb = _scales_in_nan(c["sa"], gpu), _scales_in_nan(c["sb"], gpu)
            buf, out = G.padded(M, N, b16, gpu)
            pbuf, pre = G.padded(M, N, b16, gpu, extra=16)
            qbuf = torch.full((M + 16, N + 24), 0xA5, dtype=torch.uint8, device=gpu)
            sbuf = torch.full((N // 128 + 3, M + 8, 4), 0xA5, dtype=torch.uint8, device=gpu)
            q, qs = qbuf[8:8 + M, 8:8 + N], sbuf[1:-1]
            ops.gemm_mx(a8, xa, b8, xb, out=out, epilogue=L.EPI_BIAS_GELU, bias=G.vector(c["bias"], gpu)[1],
                        aux_out=pre, q_out=q, q_sc=qs)
            yield f"K {K} BIAS_GELU", c, "gelu", buf, out
            yield f"K {K} BIAS_GELU aux_out", c, "dgelu", pbuf, pre
            # the MX copy is the quantisation of the stored bf16 output, and nothing lands outside it
            rq, rs = mx_ref(out.cpu())
            assert torch.equal(q.cpu(), rq) and torch.equal(ops.mx_untile(qs.cpu(), M, N // 32), rs)
            qb, sb = qbuf.clone(), sbuf.clone()
            qb[8:8 + M, 8:8 + N] = 0xA5
            sb[1:-1, :M] = 0xA5
            assert bool((qb == 0xA5).all()) and bool((sb == 0xA5).all()), "MX copy written outside q_out / q_sc"
            yield f"K {K} BIAS_GELU q_out", c, None, qbuf, q
            yield f"K {K} BIAS_GELU q_sc", c, None, sbuf, qs
    finally:
        lib.ergm_gemm_f8_tune(-1)


@pytest.mark.parametrize("cfg", range(N_F8_CFGS))
@pytest.mark.parametrize("mx", [False, True], ids=["f8", "mx"])
def test_lowp_gemm_per_element(gpu, mx, cfg):
    """ergm_gemm_f8 / ergm_gemm_mx, every element of every case against fp64 within LP_FACTOR times the derived bound,
    no NaN (a clamped read that leaked the surround would be one), nothing written outside the output."""
    name = f"{'MX' if mx else 'F8'} cfg {cfg}"
    for what, c, key, buf, view in lowp_launches(gpu, mx, cfg):
        if key is None:
            continue
        ref, T, ob = c["refs"][key]
        G.check(f"{name} {what}", view, ref, T, c["K"], ob, name, factor=LP_FACTOR)
        assert G.surround_intact(buf, view), f"{name} {what}: wrote outside C[:M, :N]"
    G.report(name)


def test_gemm_mx_rejects_bad_arguments(gpu):
    a = torch.zeros(64, 128, dtype=torch.uint8, device=gpu)
    s = torch.zeros(1, 64, 4, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        ops.gemm_mx(a[:, :100], s, a[:, :100], s)  # K = 100 is not a multiple of 128
    q = torch.zeros(64, 64, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):  # an MX copy of the output needs the GELU epilogue
        ops.gemm_mx(a, s, a, s, out_dtype=torch.bfloat16, epilogue=L.EPI_BIAS,
                    bias=torch.zeros(64, device=gpu), q_out=q, q_sc=s)
