"""ergm_linear_rows and the decode executor (ergm_decode_*) without a GPU: exported, declared and bound with the ABI
still 14; the workspace query host-only and monotone; a plan created and destroyed on fake pointers; argument errors
reported from the host before anything launches; the launch count of the fused engine; and the float32 self-check of
the error bound tests/test_gpu_linear_rows.py applies on the GPU (tests/_linear_rows.py)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import _linear_rows as R
from ergm_amd import _lib as L

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ergm_hip.h")
NEW = ["ergm_linear_rows", "ergm_decode_workspace_size", "ergm_decode_create", "ergm_decode_destroy", "ergm_decode_bind",
       "ergm_decode_set_engine", "ergm_decode_step", "ergm_decode_run", "ergm_decode_launches"]
TINY = dict(vocab=500, vocab_pad=512, n_embd=128, n_layer=2, n_head=2, n_inner=512, n_positions=64, max_batch=4,
            max_len=32, cap_max=32, eps=1e-5)


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14


def _buf(nbytes=1024, align=256):
    """A host buffer and an aligned address inside it (never dereferenced: no call below launches anything)."""
    raw = C.create_string_buffer(nbytes + align)
    return raw, C.c_void_p((C.addressof(raw) + align - 1) & ~(align - 1))


def _ws(**kw):
    return L.load().ergm_decode_workspace_size(C.byref(L.DecodeDims(**{**TINY, **kw})))


def test_decode_workspace_query_is_host_only_and_monotone():
    base = _ws()
    assert base > 4 * (128 * 4 + 3 * 128 * 2 + 2 * 512 * 2)   # at least the step's activations
    assert _ws(max_batch=8) > base and _ws(max_batch=32) > _ws(max_batch=8)
    assert _ws(max_len=64) >= base and _ws(max_len=1024, n_positions=1024) >= _ws(max_len=64)
    assert _ws(max_len=1024, n_positions=1024) > base          # the decode attention splits a long cache
    assert _ws(n_layer=12) >= base
    for bad in (dict(max_batch=0), dict(max_len=0), dict(n_layer=0), dict(n_embd=0), dict(vocab=-1), dict(cap_max=0),
                dict(max_len=65), dict(n_head=3), dict(n_inner=100)):
        assert _ws(**bad) == 0, bad
    assert L.load().ergm_decode_workspace_size(None) == 0


def _params(p):
    prm = L.ModelParams()
    prm.wte = prm.wte_b = prm.wpe = prm.ln_f_w = prm.ln_f_b = prm.layer_f32 = prm.layer_b16 = p
    return prm


def _plan(**kw):
    lib = L.load()
    dims = L.DecodeDims(**{**TINY, **kw})
    keep, p = _buf()
    plan = C.c_void_p()
    rc = lib.ergm_decode_create(C.byref(dims), C.byref(_params(p)), p, lib.ergm_decode_workspace_size(C.byref(dims)),
                                C.byref(plan))
    return rc, plan, keep, p


def test_create_and_destroy_without_a_gpu():
    lib = L.load()
    rc, plan, keep, p = _plan()
    assert rc == L.ERGM_OK and plan.value
    assert lib.ergm_decode_destroy(plan) == L.ERGM_OK
    assert lib.ergm_decode_destroy(None) == L.ERGM_OK


def test_executor_errors_without_a_gpu():
    lib = L.load()
    rc, plan, keep, p = _plan(n_head=3)
    assert rc == L.ERGM_EINVAL and "head_dim" in L.last_error() and not plan.value
    dims = L.DecodeDims(**TINY)
    out = C.c_void_p()
    assert lib.ergm_decode_create(C.byref(dims), C.byref(_params(p)), None, 1 << 30, C.byref(out)) == L.ERGM_EINVAL
    assert "null" in L.last_error()
    assert lib.ergm_decode_create(C.byref(dims), C.byref(_params(p)), p, 16, C.byref(out)) == L.ERGM_EINVAL
    assert "workspace" in L.last_error()
    assert lib.ergm_decode_create(C.byref(dims), C.byref(_params(None)), p, 1 << 30, C.byref(out)) == L.ERGM_EINVAL
    assert "parameter" in L.last_error()

    rc, plan, keep, p = _plan()
    assert rc == L.ERGM_OK
    try:
        ptrs = (C.c_void_p * 2)(p.value, p.value)
        # step and run before a bind
        assert lib.ergm_decode_step(plan, p, p, None) == L.ERGM_EINVAL and "bound" in L.last_error()
        assert lib.ergm_decode_run(plan, 0, 1, 0.9, 1, 497, 499, p, None) == L.ERGM_EINVAL and "bound" in L.last_error()
        assert lib.ergm_decode_bind(plan, 5, 8, ptrs, ptrs, 4, p, p, p, p) == L.ERGM_EINVAL
        assert "max_batch" in L.last_error()
        assert lib.ergm_decode_bind(plan, 0, 8, ptrs, ptrs, 4, p, p, p, p) == L.ERGM_EINVAL
        assert lib.ergm_decode_bind(plan, 2, 33, ptrs, ptrs, 4, p, p, p, p) == L.ERGM_EINVAL and "n_max" in L.last_error()
        assert lib.ergm_decode_bind(plan, 2, 8, ptrs, ptrs, 33, p, p, p, p) == L.ERGM_EINVAL and "Sc" in L.last_error()
        assert lib.ergm_decode_bind(plan, 2, 8, ptrs, ptrs, 4, None, p, p, p) == L.ERGM_EINVAL and "null" in L.last_error()
        assert lib.ergm_decode_bind(plan, 2, 8, (C.c_void_p * 2)(p.value, None), ptrs, 4, p, p, p, p) == L.ERGM_EINVAL
        assert "layer 1" in L.last_error()
        assert lib.ergm_decode_step(plan, p, p, None) == L.ERGM_EINVAL   # a failed bind binds nothing
        # a full cache: bound at n_max == max_len, every step is refused before it launches
        assert lib.ergm_decode_bind(plan, 2, 32, ptrs, ptrs, 4, p, p, p, p) == L.ERGM_OK
        for engine in (0, 1):
            assert lib.ergm_decode_set_engine(plan, engine) == L.ERGM_OK
            assert lib.ergm_decode_step(plan, p, p, None) == L.ERGM_EINVAL and "cache full" in L.last_error()
            assert lib.ergm_decode_run(plan, 3, 1, 0.9, 1, 497, 499, p, None) == L.ERGM_EINVAL
            assert "cache full" in L.last_error()
        assert lib.ergm_decode_set_engine(plan, 2) == L.ERGM_EINVAL and "engine" in L.last_error()
        assert lib.ergm_decode_set_engine(plan, -1) == L.ERGM_EINVAL
        # run: n < 1, a negative start, more steps than rows left (30 used: samples 0..2 need 2 steps, 0..3 need 3)
        assert lib.ergm_decode_bind(plan, 2, 30, ptrs, ptrs, 4, p, p, p, p) == L.ERGM_OK
        assert lib.ergm_decode_run(plan, 0, 0, 0.9, 1, 497, 499, p, None) == L.ERGM_EINVAL and "range" in L.last_error()
        assert lib.ergm_decode_run(plan, -1, 2, 0.9, 1, 497, 499, p, None) == L.ERGM_EINVAL and "range" in L.last_error()
        assert lib.ergm_decode_run(plan, 0, 4, 0.9, 1, 497, 499, p, None) == L.ERGM_EINVAL
        assert "cache full" in L.last_error()
        assert lib.ergm_decode_run(plan, 5, 3, 0.9, 1, 497, 499, p, None) == L.ERGM_EINVAL
        assert lib.ergm_decode_run(plan, 0, 2, 0.9, 1, 497, 499, None, None) == L.ERGM_EINVAL and "null" in L.last_error()
        assert lib.ergm_decode_run(plan, 0, 2, float("nan"), 1, 497, 499, p, None) == L.ERGM_EINVAL
        assert lib.ergm_decode_step(plan, None, p, None) == L.ERGM_EINVAL and "null" in L.last_error()
        assert lib.ergm_decode_step(None, p, p, None) == L.ERGM_EINVAL
        assert lib.ergm_decode_launches(None, 0) == L.ERGM_EINVAL and lib.ergm_decode_launches(plan, 7) == L.ERGM_EINVAL
    finally:
        lib.ergm_decode_destroy(plan)


@pytest.mark.parametrize("kw", [dict(), dict(n_layer=12, n_embd=768, n_head=12, n_inner=3072, vocab=50260,
                                             vocab_pad=50304, n_positions=1024, max_len=1024, cap_max=128, max_batch=32)])
def test_fused_engine_saves_three_launches_per_block(kw):
    lib = L.load()
    rc, plan, keep, p = _plan(**kw)
    assert rc == L.ERGM_OK
    try:
        n0, n1 = (lib.ergm_decode_launches(plan, e) for e in (0, 1))
        layers = {**TINY, **kw}["n_layer"]
        assert n0 >= 11 * layers + 4                       # embed, 11 per block, ln_f, head, the length update
        assert n1 <= n0 - 3 * layers
        ptrs = (C.c_void_p * layers)(*[p.value] * layers)   # bound to one sequence: the count follows the bound batch
        assert lib.ergm_decode_bind(plan, 1, 8, ptrs, ptrs, 4, p, p, p, p) == L.ERGM_OK
        assert lib.ergm_decode_launches(plan, 1) <= lib.ergm_decode_launches(plan, 0) - 3 * layers
    finally:
        lib.ergm_decode_destroy(plan)


def _lr(lib, p, A="p", W="p", Cc="p", **kw):
    d = dict(M=4, N=128, K=128, lda=128, ldw=128, ldc=128, w_layout=L.KN, epilogue=L.EPI_NONE)
    d.update(kw)
    desc = L.LinearRowsDesc(**d)
    pick = lambda v: p if v == "p" else v
    return lib.ergm_linear_rows(C.byref(desc), pick(A), pick(W), pick(Cc), None)


def test_linear_rows_errors_without_a_gpu():
    lib = L.load()
    keep, p = _buf()
    odd = C.c_void_p(p.value + 8)
    assert lib.ergm_linear_rows(None, p, p, p, None) == L.ERGM_EINVAL and "null" in L.last_error()
    for kw in (dict(A=None), dict(W=None), dict(Cc=None)):
        assert _lr(lib, p, **kw) == L.ERGM_EINVAL and "null" in L.last_error(), kw
    for kw, word in ((dict(M=0), "M 0"), (dict(M=-2), "M -2"), (dict(K=96, lda=96), "K 96"), (dict(K=0), "K 0"),
                     (dict(N=100), "N 100"), (dict(N=0), "N 0"), (dict(lda=132), "lda"), (dict(lda=64), "lda"),
                     (dict(ldw=132), "ldw"), (dict(ldw=64), "ldw"), (dict(ldc=120), "ldc"), (dict(w_layout=2), "layout"),
                     (dict(w_layout=L.NK, K=256, lda=256, ldw=128), "ldw"),
                     (dict(epilogue=L.EPI_GELU_BWD, bias=p), "epilogue"), (dict(epilogue=L.EPI_ACCUM), "epilogue"),
                     (dict(epilogue=L.EPI_BIAS), "bias"), (dict(epilogue=L.EPI_BIAS_GELU), "bias"),
                     (dict(epilogue=L.EPI_BIAS_RESID, bias=p), "aux"),
                     (dict(epilogue=L.EPI_BIAS_RESID, bias=p, aux=p, ld_aux=64), "aux"),
                     (dict(ln_gamma=p), "gamma and beta"), (dict(ln_beta=p), "gamma and beta"),
                     (dict(ln_gamma=p, ln_beta=p, ln_eps=-1.0), "eps"),
                     (dict(ln_gamma=p, ln_beta=p, ln_eps=1e-5, lda=130), "lda"),   # f32 rows: a multiple of 4
                     (dict(ln_gamma=odd, ln_beta=p, ln_eps=1e-5), "alignment"), (dict(A=odd), "alignment"),
                     (dict(W=odd), "alignment"), (dict(Cc=C.c_void_p(p.value + 2)), "misaligned")):
        assert _lr(lib, p, **kw) == L.ERGM_EINVAL, kw
        assert word in L.last_error(), (kw, L.last_error())


@pytest.mark.parametrize("K,N,layout", R.SHAPES)
def test_bound_admits_fp32_reference(K, N, layout):
    """The bound and the Frobenius gates of tests/_linear_rows.py, checked without the library: LayerNorm in plain
    torch float32 -> one rounding to bf16 -> float32 matmul -> epilogue, rounded to the output type, for every
    epilogue with and without the prologue on the GPU test's own inputs.  If a straightforward float32 evaluation did
    not fit, the bound would be wrong, not the kernel."""
    c = R.case(K, N, layout)
    f32 = torch.float32
    x, g, b = c["x"], c["gamma"], c["beta"]
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) * (x - mu)).mean(1, keepdim=True)
    a_ln = ((x - mu) * (1.0 / torch.sqrt(var + torch.tensor(R.EPS, dtype=f32))) * g + b).bfloat16()
    k0 = torch.tensor(math.sqrt(2.0 / math.pi), dtype=f32)
    worst = {}
    for ln in (False, True):
        P = (a_ln if ln else c["A"]).float() @ c["W"].float()
        z = P + c["bias"]
        outs = {"none": P, "bias": z.bfloat16(), "resid": c["resid"] + z,
                "gelu": (0.5 * z * (1.0 + torch.tanh(k0 * (z + 0.044715 * z * z * z)))).bfloat16()}
        for epi in R.epilogues_of(layout):
            ref, T, ob, extra = c["refs"][(ln, epi)]
            assert outs[epi].dtype == (torch.bfloat16 if ob else f32)
            worst[(ln, epi)] = R.check(f"K {K} N {N} ln {ln} {epi}", outs[epi], c, ln, epi, R.MMAX)
    print({k: (round(v[0], 3), float("%.2g" % v[1])) for k, v in worst.items()})
    assert max(v[0] for v in worst.values()) <= 1.0
    # why an f32 output with the prologue is gated at 6e-3: the operand's one bf16 rounding alone is far above 1e-5,
    # and well inside 6e-3
    assert 3e-3 > worst[(True, "none")][1] > 1e-4 > worst[(False, "none")][1]
