"""The GEMM planning query (ergm_gemm_plan / ergm_gemm_cfg_count, ABI 14) without a GPU: which kernel configuration,
split and path ergm_gemm would take for a descriptor, under ergm_gemm_tune and by its own rules.  The GPU tests of
tests/test_gpu_gemm_matrix.py lean on it to know that a forced configuration is the one that ran.  Also here, because
it needs no GPU either: the self-check of that file's error bound against a plain float32 evaluation."""
import ctypes as C
import math

import pytest
import torch

import test_gpu_gemm_matrix as G
from ergm_amd import _lib as L

# (a_layout, b_layout, epilogue, c_dtype) instantiated for the pipelined kernels: combo_ok in gemm.hip
PIPE_COMBOS = [(L.MK, L.KN, L.EPI_BIAS, L.BF16), (L.MK, L.KN, L.EPI_BIAS_GELU, L.BF16),
               (L.MK, L.KN, L.EPI_BIAS_RESID, L.F32), (L.MK, L.KN, L.EPI_NONE, L.F32),
               (L.MK, L.NK, L.EPI_NONE, L.F32), (L.MK, L.NK, L.EPI_NONE, L.BF16),
               (L.MK, L.NK, L.EPI_GELU_BWD, L.BF16), (L.KM, L.KN, L.EPI_NONE, L.F32)]
PTR = 0x1000  # a non-NULL value for the pointer fields: the query only tests them for NULL


def desc(M=328, N=392, K=192, al=L.MK, bl=L.KN, epi=L.EPI_NONE, dt=L.F32, ldc=None, split_k=0, **kw):
    lda = (K if al == L.MK else (M + 7) // 8 * 8) + 24
    ldb = (K if bl == L.NK else (N + 7) // 8 * 8) + 24
    ldc = N + 24 if ldc is None else ldc
    d = L.GemmDesc(M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, a_layout=al, b_layout=bl, c_dtype=dt, epilogue=epi,
                   alpha=1.0, split_k=split_k, **kw)
    if epi in (L.EPI_BIAS, L.EPI_BIAS_GELU, L.EPI_BIAS_RESID):
        d.bias = PTR
    if epi in (L.EPI_BIAS_RESID, L.EPI_GELU_BWD):
        d.aux, d.ld_aux = PTR, N + 24
    if epi == L.EPI_BIAS_GELU:
        d.aux_out, d.ld_aux_out = PTR, N + 24
    return d


def plan(d):
    cfg, split, flags = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    L.check(L.load().ergm_gemm_plan(C.byref(d), C.byref(cfg), C.byref(split), C.byref(flags)), "ergm_gemm_plan")
    return cfg.value, split.value, flags.value


@pytest.fixture
def lib():
    """The library with the shape trace switched on and empty; afterwards the trace must still be empty (the query
    records nothing) and the forced configuration is cleared."""
    lib = L.load()
    lib.ergm_gemm_trace(0, None, 0)
    lib.ergm_gemm_trace(1, None, 0)
    try:
        yield lib
        assert lib.ergm_gemm_trace(1, None, 0) == 0
    finally:
        lib.ergm_gemm_tune(-1, 0)
        lib.ergm_gemm_trace(0, None, 0)


def test_cfg_count_bounds_the_tuning_hook(lib):
    n = lib.ergm_gemm_cfg_count()
    assert n == 47
    assert lib.ergm_gemm_tune(n - 1, 1) == L.ERGM_OK
    assert lib.ergm_gemm_tune(n, 1) == L.ERGM_EINVAL


def test_forced_config_is_reported_for_every_pipelined_combination(lib):
    for cfg in range(lib.ergm_gemm_cfg_count()):
        for split in (1, 2):
            L.check(lib.ergm_gemm_tune(cfg, split), "tune")
            for al, bl, epi, dt in PIPE_COMBOS:
                got = plan(desc(al=al, bl=bl, epi=epi, dt=dt))
                assert got[:2] == (cfg, split) and not got[2] & 4, (cfg, split, al, bl, epi, dt, got)


@pytest.mark.parametrize("forced", [-1, 0, 16, 33, 38])
def test_register_staged_kernel_is_reported(lib, forced):
    L.check(lib.ergm_gemm_tune(forced, 1 if forced >= 0 else 0), "tune")
    cases = {"K % 64": desc(K=200), "N % 8": desc(N=396, ldc=400), "ldc % 8": desc(ldc=396),
             "KM x NK": desc(al=L.KM, bl=L.NK), "BIAS f32": desc(epi=L.EPI_BIAS, dt=L.F32),
             "ACCUM": desc(epi=L.EPI_ACCUM), "ld_aux % 8": desc(epi=L.EPI_BIAS_RESID)}
    cases["ld_aux % 8"].ld_aux = 396
    for name, d in cases.items():
        assert plan(d)[0] == -1, name


def test_split_rounds_to_whole_k_steps(lib):
    for K, want, got in ((320, 3, 3), (128, 5, 2), (64, 2, 1)):
        L.check(lib.ergm_gemm_tune(-1, 0), "tune")
        assert plan(desc(K=K, split_k=want))[1] == got, (K, want)
        L.check(lib.ergm_gemm_tune(0, want), "tune")
        assert plan(desc(K=K))[:2] == (0, got), (K, want)
        assert plan(desc(K=K, al=L.KM, bl=L.NK))[:2] == (-1, 1)  # the forced split is the pipelined kernels' only


def test_workspace_size_follows_the_plan(lib):
    M, N, K = 200, 136, 448
    for cfg in (2, 16, 33, 38):
        for want in (1, 2, 3):
            L.check(lib.ergm_gemm_tune(cfg, want), "tune")
            for bias_grad in (False, True):
                d = desc(M, N, K, al=L.KM, bl=L.KN)
                if bias_grad:
                    d.bias_grad = PTR
                c, split, flags = plan(d)
                assert (c, split) == (cfg, want)
                assert bool(flags & 1) == (bias_grad and cfg == 2)
                # the partial column sums live in the workspace exactly when the kernel sums them
                need = 0 if split == 1 else split * M * N * 4 + (split * N * 4 if bias_grad and flags & 1 else 0)
                assert lib.ergm_gemm_workspace_size(C.byref(d)) == need, (cfg, want, bias_grad)
    L.check(lib.ergm_gemm_tune(-1, 0), "tune")
    d = desc(M, N, K)
    assert plan(d)[1] == 1 and lib.ergm_gemm_workspace_size(C.byref(d)) == 0


def test_device_extent_descriptors(lib):
    T, E, K = 160, 64, 1088
    n = lib.ergm_gemm_cfg_count()
    for forced in range(-1, n):
        L.check(lib.ergm_gemm_tune(forced, 0), "tune")
        want = forced if forced in (0, 2, 6, 14) else 2
        dx = desc(T, E, K, m_count_dev=PTR, row_map=PTR)
        assert plan(dx) == (want, 2, 4), forced  # K / 512 slices
        assert lib.ergm_gemm_workspace_size(C.byref(dx)) == 2 * T * E * 4
        for split in (0, 3):
            L.check(lib.ergm_gemm_tune(forced, split), "tune")
            dw = desc(208, E, T, al=L.KM, bl=L.KN, k_count_dev=PTR)
            assert plan(dw) == (want, 1, 4), (forced, split)  # a device-side contraction length is never split
            assert lib.ergm_gemm_workspace_size(C.byref(dw)) == 0
    L.check(lib.ergm_gemm_tune(-1, 0), "tune")
    assert plan(desc(T, E, 208, m_count_dev=PTR)) == (-1, 1, 4)  # K % 64 != 0
    assert plan(desc(T, E, 4160, m_count_dev=PTR)) == (2, 8, 4 | 2)  # 8 slices under a row count: one per XCD
    assert plan(desc(T, E, 4160, row_map=PTR)) == (2, 8, 4)


def test_in_kernel_bias_gradient_flag(lib):
    n = lib.ergm_gemm_cfg_count()
    flag = {}
    for cfg in range(n):
        for split in (1, 2):
            L.check(lib.ergm_gemm_tune(cfg, split), "tune")
            d = desc(200, 136, 448, al=L.KM, bl=L.KN, bias_grad=PTR)
            c, s, f = plan(d)
            assert (c, s) == (cfg, split)
            flag.setdefault(cfg, f & 1)
            assert flag[cfg] == f & 1  # a property of the configuration, split or not
            assert not plan(desc(200, 136, 448, al=L.KM, bl=L.KN))[2] & 1  # nothing to sum without bias_grad
    assert flag[2] == 1 and flag[16] == 0 and flag[33] == 0 and flag[38] == 0
    assert 0 < sum(flag.values()) < n
    # the register-staged kernel never sums in-kernel
    L.check(lib.ergm_gemm_tune(2, 1), "tune")
    assert plan(desc(200, 136, 1000, al=L.KM, bl=L.KN, bias_grad=PTR)) == (-1, 1, 0)


def test_automatic_plan_and_overrides(lib):
    L.check(lib.ergm_gemm_tune(-1, 0), "tune")
    assert plan(desc()) == (0, 1, 0)  # 6 x 7 tiles of 64 x 64: the small-output configuration, unsplit
    assert plan(desc(768, 768, 2048, al=L.KM, bl=L.KN))[0] >= 0
    assert plan(desc(1024, 2304, 768, al=L.MK, bl=L.KN)) == (3, 1, 0)  # a built-in step-tuned entry
    key = (328, 392, 192, L.MK, L.KN)
    L.check(lib.ergm_gemm_set_override(*key, 21, 3), "override")
    try:
        assert plan(desc()) == (21, 3, 0)
        assert plan(desc(split_k=1)) == (0, 1, 0)  # an explicit split_k bypasses the table
        L.check(lib.ergm_gemm_tune(7, 1), "tune")
        assert plan(desc()) == (7, 1, 0)  # the thread's forced configuration wins
    finally:
        lib.ergm_gemm_tune(-1, 0)
        L.check(lib.ergm_gemm_set_override(*key, -1, 1), "override")
    assert plan(desc()) == (0, 1, 0)


def test_descriptor_checks_need_no_operands(lib):
    out = [C.c_int(), C.c_int(), C.c_int()]
    refs = [C.byref(x) for x in out]
    assert lib.ergm_gemm_plan(None, *refs) == L.ERGM_EINVAL
    assert lib.ergm_gemm_plan(C.byref(desc()), None, refs[1], refs[2]) == L.ERGM_EINVAL
    bad = {"shape": desc(M=0), "K=": desc(K=100, al=L.MK, bl=L.NK), "lda/ldb": desc(),
           "bad a_layout": desc(al=2), "ldc < N": desc(ldc=384), "bad c_dtype": desc(dt=2),
           "bad epilogue": desc(epi=6), "f32 C": desc(epi=L.EPI_BIAS_RESID, dt=L.BF16), "needs aux": desc(),
           "aux_out": desc(), "bias_grad": desc(bias_grad=PTR), "m_count_dev": desc(bl=L.NK, m_count_dev=PTR),
           "lda too small": desc(M=100, al=L.KM)}
    bad["lda/ldb"].lda += 4
    bad["needs aux"].epilogue = L.EPI_GELU_BWD
    bad["aux_out"].epilogue = L.EPI_BIAS_GELU
    bad["lda too small"].lda = 96
    for word, d in bad.items():
        assert lib.ergm_gemm_plan(C.byref(d), *refs) == L.ERGM_EINVAL, word
        assert word in L.last_error(), (word, L.last_error())
    assert lib.ergm_gemm_plan(C.byref(desc()), *refs) == L.ERGM_OK


def test_bound_admits_fp32_reference():
    """The elementwise bound of tests/test_gpu_gemm_matrix.py, checked without the library: every epilogue of every
    case that file runs, evaluated with plain torch float32 on the CPU and rounded to the output type, must fit it.
    If float32 arithmetic in some order did not fit, the bound would be wrong, not the kernels."""
    f32 = torch.float32
    a = torch.tensor(G.ALPHA, dtype=f32) * torch.tensor(G.ALPHA_DEV, dtype=f32)
    worst = {}

    def fits(name, got, ref, T, K, ob):
        worst[name] = max(worst.get(name, 0.0), G.check(name, got, ref, T, K, ob))

    c = G.c1_case()
    K = c["K"]
    P = c["A"].float() @ c["B"].float()
    z = a * P + c["bias"]
    k0 = torch.tensor(math.sqrt(2.0 / math.pi), dtype=f32)
    t = torch.tanh(k0 * (z + 0.044715 * z * z * z))
    ge = 0.5 * z * (1.0 + t)
    dge = 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * k0 * (1.0 + 3.0 * 0.044715 * z * z)
    sc = torch.tensor(1.0, dtype=f32) / (1.0 - torch.tensor(G.C5_DROP["p"], dtype=f32))
    outs = {"bias": z.bfloat16(), "gelu": ge.bfloat16(), "dgelu": dge.bfloat16(), "resid": c["resid"] + z,
            "none": a * P, "none_bf16": (a * P).bfloat16(), "gelu_bwd": (a * P * c["aux"].float()).bfloat16(),
            "drop": torch.where(c["keep"], z * sc, torch.zeros((), dtype=f32)) + c["resid"]}
    assert set(outs) == set(c["refs"])
    for key, got in outs.items():
        ref, T, ob = c["refs"][key]
        assert got.dtype == (torch.bfloat16 if ob else f32)
        fits("C1 " + key, got, ref, T, K, ob)
    for K in G.C2_KS:
        c = G.c2_case(K)
        fits("C2", c["A"].float() @ c["B"].float(), c["ref"], c["T"], K, False)
    for M in G.C3_MS:
        for K in G.C3_KS:
            c = G.c3_case(M, K)
            fits("C3 dW", a * (c["X"].float().t() @ c["dY"].float()), c["ref_w"], c["T_w"], K, False)
            err = ((a * c["dY"].float().sum(0)).double() - c["ref_b"]).abs()
            b = 2.0 * K * G.U32 * c["T_b"]
            assert (err <= b).all().item()
            worst["C3 db"] = max(worst.get("C3 db", 0.0), (err / b).max().item())
    for n in G.C4_NS:
        c = G.c4_dx_case(n)
        fits("C4 dX", c["A"][:n].float() @ c["W"].float(), c["ref"], c["T"], G.C4_K, False)
        c = G.c4_dw_case(n)
        fits("C4 dW", c["A"][:n].float().t() @ c["B"][:n].float(), c["ref"], c["T"], n, False)
    for name, r in worst.items():
        print(f"float32 on the CPU, {name}: worst err/bound {r:.4f}")
