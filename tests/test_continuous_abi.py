"""Continuous batching without a GPU: the new entry points (ergm_attn_fwd_ragged, ergm_rows_to_slots, ergm_embed_packed,
ergm_topp_sample_rows and the executor's slot mode) are declared, bound and exported with the ABI still 14; the
admission workspace query is host-only and monotone; every refusal of ergm_decode_admit comes back as ERGM_EINVAL with
a telling message on fake pointers, before anything launches; and the dry launch count of an admission."""
import ctypes as C
import os
import re

from ergm_amd import _lib as L

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ergm_hip.h")
NEW = ["ergm_attn_fwd_ragged", "ergm_rows_to_slots", "ergm_embed_packed", "ergm_topp_sample_rows", "ergm_decode_bind_slots",
       "ergm_decode_admit_workspace_size", "ergm_decode_admit", "ergm_decode_admit_launches", "ergm_decode_step_slots",
       "ergm_decode_run_slots"]
TINY = dict(vocab=500, vocab_pad=512, n_embd=128, n_layer=2, n_head=2, n_inner=512, n_positions=64, max_batch=4,
            max_len=32, cap_max=32, eps=1e-5)


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14
    assert int(re.search(r"#define ERGM_ADMIT_META_ROWS (\d+)", src).group(1)) == L.ADMIT_META_ROWS


def _buf(nbytes=1024, align=256):
    """A host buffer and an aligned address inside it (never dereferenced: no call below launches anything)."""
    raw = C.create_string_buffer(nbytes + align)
    return raw, C.c_void_p((C.addressof(raw) + align - 1) & ~(align - 1))


def _admit_ws(rows, cap_rows, **kw):
    return L.load().ergm_decode_admit_workspace_size(C.byref(L.DecodeDims(**{**TINY, **kw})), rows, cap_rows)


def test_admit_workspace_query_is_host_only_and_monotone():
    sizes = [_admit_ws(r, 32) for r in (1, 2, 5, 31, 32, 33, 64, 100, 128)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # at least the packed activations: h, x, qkv, att, q (E-wide) and the two MLP buffers
    assert sizes[-1] > 128 * (128 * 4 + 128 * 2 * 3 + 3 * 128 * 2 + 2 * 512 * 2)
    assert _admit_ws(64, 64) >= _admit_ws(64, 32) and _admit_ws(64, 128) > _admit_ws(64, 1)
    for rows, cap in ((0, 8), (8, 0), (-1, 8), (4 * 32 + 1, 8), (8, 4 * 32 + 1)):   # more rows than the slots hold
        assert _admit_ws(rows, cap) == 0, (rows, cap)
    assert _admit_ws(8, 8, n_head=3) == 0
    assert L.load().ergm_decode_admit_workspace_size(None, 8, 8) == 0


def _plan(capkv=True):
    lib = L.load()
    dims = L.DecodeDims(**TINY)
    keep, p = _buf()
    prm = L.ModelParams()
    prm.wte = prm.wte_b = prm.wpe = prm.ln_f_w = prm.ln_f_b = prm.layer_f32 = prm.layer_b16 = p
    if capkv:
        prm.capkv_w_b = prm.capkv_b = p
    plan = C.c_void_p()
    rc = lib.ergm_decode_create(C.byref(dims), C.byref(prm), p, lib.ergm_decode_workspace_size(C.byref(dims)), C.byref(plan))
    assert rc == L.ERGM_OK
    return plan, keep, p


def _arr(*v):
    return (C.c_int * len(v))(*v)


def test_admit_refusals_without_a_gpu():
    lib = L.load()
    plan, keep, p = _plan()
    big = 1 << 30
    try:
        ptrs = (C.c_void_p * 2)(p.value, p.value)

        def admit(slots, lens, caps, new, ws_bytes=big, ids=p, meta=p):
            n = len(slots)
            return lib.ergm_decode_admit(plan, n, _arr(*slots), _arr(*lens), _arr(*caps), _arr(*new), meta, ids, p, p,
                                         None, None, None, p, ws_bytes, None)

        def refused(word, *a, **kw):
            assert admit(*a, **kw) == L.ERGM_EINVAL
            assert word in L.last_error(), (word, L.last_error())

        # before the slots are bound every slot call refuses, and the slot bind checks its pointers
        refused("slots bound", [0], [5], [7], [4])
        assert lib.ergm_decode_step_slots(plan, p, p, None) == L.ERGM_EINVAL and "slots bound" in L.last_error()
        assert lib.ergm_decode_run_slots(plan, 8, 0.9, 1, 497, 499, p, None) == L.ERGM_EINVAL
        assert lib.ergm_decode_bind_slots(plan, ptrs, ptrs, p, p, p, p, p, p, None) == L.ERGM_EINVAL
        assert "null" in L.last_error()
        assert lib.ergm_decode_bind_slots(plan, (C.c_void_p * 2)(p.value, None), ptrs, p, p, p, p, p, p, p) == L.ERGM_EINVAL
        assert "layer 1" in L.last_error()
        assert lib.ergm_decode_bind_slots(plan, ptrs, ptrs, p, p, p, p, p, p, p) == L.ERGM_OK
        # the static path's calls now refuse: they serve ergm_decode_bind
        assert lib.ergm_decode_step(plan, p, p, None) == L.ERGM_EINVAL and "bound" in L.last_error()
        # every refusal of the issue's list
        refused("slot 4", [4], [5], [7], [4])                       # a slot out of range
        refused("slot -1", [-1], [5], [7], [4])
        refused("named twice", [2, 0, 2], [5, 6, 7], [7, 7, 7], [4, 4, 4])
        refused("empty prompt", [0], [0], [7], [4])                 # n_b < 1
        refused("empty caption", [0], [5], [0], [4])                # c_b < 1
        refused("cap_max", [0], [5], [33], [4])                     # c_b > cap_max
        refused("max_len", [0], [5], [7], [28])                     # n_b + max_new > max_len
        refused("max_len", [0], [33], [7], [1])
        refused("max_new", [0], [5], [7], [0])                      # max_new < 1
        refused("workspace", [0, 1], [16, 15], [7, 7], [4, 4], ws_bytes=_admit_ws(30, 14))   # 31 rows > the 30 sized for
        refused("n_seq", [0, 1, 2, 3, 0], [1] * 5, [1] * 5, [1] * 5)
        refused("null", [0], [5], [7], [4], ids=None)
        refused("null", [0], [5], [7], [4], meta=None)
        assert lib.ergm_decode_admit(None, 1, _arr(0), _arr(5), _arr(7), _arr(4), p, p, p, p, None, None, None, p, big,
                                     None) == L.ERGM_EINVAL
        # visual without audio
        assert lib.ergm_decode_admit(plan, 1, _arr(0), _arr(5), _arr(7), _arr(4), p, p, p, p, p, None, None, p, big,
                                     None) == L.ERGM_EINVAL and "together" in L.last_error()
        assert lib.ergm_decode_run_slots(plan, 0, 0.9, 1, 497, 499, p, None) == L.ERGM_EINVAL and "n 0" in L.last_error()
        assert lib.ergm_decode_run_slots(plan, 8, float("nan"), 1, 497, 499, p, None) == L.ERGM_EINVAL
        assert lib.ergm_decode_run_slots(plan, 8, 0.9, 1, 497, 499, None, None) == L.ERGM_EINVAL
        assert lib.ergm_decode_step_slots(plan, None, p, None) == L.ERGM_EINVAL and "null" in L.last_error()
        # rebinding the static state takes the plan out of slot mode
        assert lib.ergm_decode_bind(plan, 2, 8, ptrs, ptrs, 4, p, p, p, p) == L.ERGM_OK
        refused("slots bound", [0], [5], [7], [4])
    finally:
        lib.ergm_decode_destroy(plan)
    plan, keep, p = _plan(capkv=False)
    try:
        ptrs = (C.c_void_p * 2)(p.value, p.value)
        assert lib.ergm_decode_bind_slots(plan, ptrs, ptrs, p, p, p, p, p, p, p) == L.ERGM_OK
        assert lib.ergm_decode_admit(plan, 1, _arr(0), _arr(5), _arr(7), _arr(4), p, p, p, p, None, None, None, p, big,
                                     None) == L.ERGM_EINVAL and "caption K/V" in L.last_error()
    finally:
        lib.ergm_decode_destroy(plan)


def test_admit_launch_count_is_a_dry_walk():
    """One admission of the tiny model: the embedding, 14 kernels per block when no GEMM splits K (3 LayerNorms, 7
    GEMMs, 2 ragged attentions, 2 row scatters), the gather of the last rows, ln_f, the head, the logits scatter and
    the slot state: 14·L + 6, a split-K GEMM adding its reduction.  The count does not depend on the number of
    sequences, which is what the ragged kernels buy over a launch per sequence."""
    lib = L.load()
    plan, keep, p = _plan()
    try:
        base = 14 * TINY["n_layer"] + 6
        one, three = lib.ergm_decode_admit_launches(plan, 1, 30, 22), lib.ergm_decode_admit_launches(plan, 3, 30, 22)
        assert base <= one <= base + 7 * TINY["n_layer"] + 1
        assert three - one in range(-1, 2)   # only the head GEMM's row count (1 or 3) differs
        assert lib.ergm_decode_admit_launches(plan, 0, 30, 22) == L.ERGM_EINVAL
        assert lib.ergm_decode_admit_launches(plan, 3, 2, 22) == L.ERGM_EINVAL
        assert lib.ergm_decode_admit_launches(None, 1, 30, 22) == L.ERGM_EINVAL
        # the existing step count is what it was: slot mode shares the step's walk
        assert lib.ergm_decode_launches(plan, 0) - lib.ergm_decode_launches(plan, 1) == 3 * TINY["n_layer"]
    finally:
        lib.ergm_decode_destroy(plan)
