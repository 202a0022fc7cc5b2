"""Beam search in slot mode without a GPU: ergm_beam_seed and ergm_decode_run_slot_beams are declared, bound and exported
with the ABI number unchanged, and every refusal of both comes back as ERGM_EINVAL on fake pointers, on an unbound plan
or on a plan bound in slot mode to host memory, before anything launches (no call below is valid, so none reaches a
device).  ergm_decode_run_beams keeps refusing a plan bound in slot mode."""
import ctypes as C
import os
import re

from ergm_amd import _lib as L

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ergm_hip.h")
NEW = ["ergm_beam_seed", "ergm_decode_run_slot_beams"]
TINY = dict(vocab=500, vocab_pad=512, n_embd=128, n_layer=2, n_head=2, n_inner=512, n_positions=64, max_batch=8,
            max_len=32, cap_max=16, eps=1e-5)


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14


def _buf(nbytes=1024, align=256):
    raw = C.create_string_buffer(nbytes + align)
    return raw, C.c_void_p((C.addressof(raw) + align - 1) & ~(align - 1))


def _arr(*v):
    return (C.c_int * len(v))(*v)


def test_seed_refusals_without_a_gpu():
    lib = L.load()
    keep, p = _buf()
    row = 2 * 128 * 2   # a K | V row of E = 128 in bytes
    ok = dict(n_layer=2, ld_seq=16 * row, ld_row=row, row_bytes=row, groups_dev=p, groups=(2, 0, 3), W=2, max_batch=8, cap_max=16,
              lens=p, cap_lens=p, stop_lens=p, finished=p, scores=p, xkv=(p.value, p.value))

    def seed(**kw):
        a = {**ok, **kw}
        xkv = None if a["xkv"] is None else (C.c_void_p * len(a["xkv"]))(*a["xkv"])
        groups = None if a["groups"] is None else _arr(*a["groups"])
        n_grp = a.get("n_grp", 0 if a["groups"] is None else len(a["groups"]))
        return lib.ergm_beam_seed(xkv, a["n_layer"], a["ld_seq"], a["ld_row"], a["row_bytes"], a["groups_dev"], groups, n_grp,
                                  a["W"], a["max_batch"], a["cap_max"], a["lens"], a["cap_lens"], a["stop_lens"], a["finished"],
                                  a["scores"], None)

    def refused(word, **kw):
        assert seed(**kw) == L.ERGM_EINVAL, kw
        assert word in L.last_error(), (word, L.last_error())

    refused("outside [0, 4)", groups=(2, 4))                 # G = 8 / 2
    refused("outside [0, 4)", groups=(-1,))
    refused("outside [0, 1)", groups=(1,), W=8)
    refused("named twice", groups=(2, 0, 2))
    refused("n_grp", groups=(0, 1, 2, 3, 0))                 # more entries than groups
    refused("n_grp", groups=(0,), n_grp=0)
    for W in (0, 9, -1):
        refused("W %d outside" % W, W=W)
    refused("multiple of W", W=3)
    refused("multiple of W", max_batch=0)
    refused("multiples of 16", ld_seq=16 * row + 8)
    refused("multiples of 16", ld_row=row + 4, ld_seq=32 * row)
    refused("multiples of 16", row_bytes=row - 2)
    refused("multiples of 16", row_bytes=0)
    refused("shorter", ld_row=row - 16)
    refused("shorter", ld_seq=15 * row)                      # cap_max rows do not fit a slot
    refused("n_layer", n_layer=0)
    refused("cap_max", cap_max=0)
    for name in ("xkv", "groups_dev", "groups", "lens", "cap_lens", "stop_lens", "finished", "scores"):
        refused("null", **{name: None})
    refused("layer 1", xkv=(p.value, 0))
    refused("layer 0", xkv=(p.value + 8, p.value))
    refused("W 0 outside", W=0, groups=(9,))                 # W is looked at before the ids are divided by it


def _plan(**kw):
    lib = L.load()
    dims = L.DecodeDims(**{**TINY, **kw})
    keep, p = _buf()
    prm = L.ModelParams()
    prm.wte = prm.wte_b = prm.wpe = prm.ln_f_w = prm.ln_f_b = prm.layer_f32 = prm.layer_b16 = p
    prm.capkv_w_b = prm.capkv_b = p
    plan = C.c_void_p()
    rc = lib.ergm_decode_create(C.byref(dims), C.byref(prm), p, lib.ergm_decode_workspace_size(C.byref(dims)), C.byref(plan))
    assert rc == L.ERGM_OK
    return plan, keep, p


def _bind_slots(plan, p, n_layer=2):
    ptrs = (C.c_void_p * n_layer)(*[p.value] * n_layer)
    assert L.load().ergm_decode_bind_slots(plan, ptrs, ptrs, p, p, p, p, p, p, p) == L.ERGM_OK


def test_run_slot_beams_refusals_without_a_gpu():
    lib = L.load()
    plan, keep, p = _plan()
    big = 1 << 20
    try:
        ok = dict(plan=plan, n=1, W=2, rows_bound=5, eos=497, sp2=499, scores=p, toks=p, pars=p, ws=p, ws_bytes=big)

        def run(**kw):
            a = {**ok, **kw}
            return lib.ergm_decode_run_slot_beams(a["plan"], a["n"], a["W"], a["rows_bound"], a["eos"], a["sp2"], a["scores"],
                                                  a["toks"], a["pars"], a["ws"], a["ws_bytes"], None)

        def refused(word, **kw):
            assert run(**kw) == L.ERGM_EINVAL, kw
            assert word in L.last_error(), (word, L.last_error())

        refused("null plan", plan=None)
        refused("no slots bound")                               # created, never bound
        ptrs = (C.c_void_p * 2)(p.value, p.value)
        assert lib.ergm_decode_bind(plan, 8, 5, ptrs, ptrs, 16, p, p, p, p) == L.ERGM_OK
        refused("no slots bound")                               # bound by ergm_decode_bind: not slot mode
        _bind_slots(plan, p)
        refused("n 0", n=0)
        refused("n -2", n=-2)
        for W in (0, 9, -1):
            refused("W %d outside" % W, W=W)
        refused("multiple of W", W=3)
        refused("eos_id", eos=500)
        refused("eos_id", eos=-1)
        refused("rows_bound", rows_bound=33)
        refused("rows_bound", rows_bound=-1)
        for name in ("scores", "toks", "pars", "ws"):
            refused("null", **{name: None})
        refused("misaligned", ws=C.c_void_p(p.value + 4))
        refused("misaligned", toks=C.c_void_p(p.value + 4))
        refused("misaligned", scores=C.c_void_p(p.value + 2))
        refused("misaligned", pars=C.c_void_p(p.value + 1))
        need = lib.ergm_beam_select_workspace_size(8, 2)
        assert need > 0
        refused("workspace", ws_bytes=need - 1)
        refused("workspace", ws_bytes=lib.ergm_beam_select_workspace_size(8, 1), W=4)
        # ergm_decode_run_beams keeps its refusal of a plan in slot mode
        assert lib.ergm_decode_run_beams(plan, 1, 2, 497, 499, p, p, p, p, big, None) == L.ERGM_EINVAL
        assert "slot mode" in L.last_error()
    finally:
        lib.ergm_decode_destroy(plan)
    # W above the vocabulary
    plan, keep, p = _plan(vocab=4, vocab_pad=64)
    try:
        _bind_slots(plan, p)
        assert lib.ergm_decode_run_slot_beams(plan, 1, 8, 5, 1, 3, p, p, p, p, big, None) == L.ERGM_EINVAL
        assert "vocabulary" in L.last_error()
    finally:
        lib.ergm_decode_destroy(plan)
