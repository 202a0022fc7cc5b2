"""Beam search without a GPU: ergm_beam_select, ergm_beam_gather and ergm_decode_run_beams are declared, bound and
exported with the ABI still 14; each refuses its bad arguments with ERGM_EINVAL on fake pointers before anything
launches; and the host side of BatchedGenerator.beam_search (beam_backtrack: the walk through the parents and the
length-penalty ordering) on hand-made arrays."""
import ctypes as C
import math
import os
import re

import pytest

from ergm_amd import _lib as L
from ergm_amd.generate import beam_backtrack

import test_continuous_abi as CA

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ergm_hip.h")
NEW = ["ergm_beam_select", "ergm_beam_gather", "ergm_decode_run_beams"]


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW + ["ergm_beam_select_workspace_size"]:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14
    assert lib.ergm_beam_select_workspace_size(12, 4) >= 12 * 4 * 8
    for R, W in ((0, 1), (8, 0), (8, 9), (-4, 2)):
        assert lib.ergm_beam_select_workspace_size(R, W) == 0


def test_beam_select_refuses_before_any_launch():
    lib = L.load()
    keep, p = CA._buf()

    def sel(logits=p, ldl=512, R=12, W=4, V=500, scores=p, fin=p, eos=497, par=p, tok=p, ws=p, ws_bytes=1 << 20):
        return lib.ergm_beam_select(logits, ldl, R, W, V, scores, fin, eos, par, tok, ws, ws_bytes, None)

    def refused(word, **kw):
        assert sel(**kw) == L.ERGM_EINVAL
        assert word in L.last_error(), (word, L.last_error())

    for name in ("logits", "scores", "fin", "par", "tok"):
        refused("null", **{name: None})
    refused("outside [1, 8]", W=0)
    refused("outside [1, 8]", W=9, R=18)
    refused("multiple", R=10)
    refused("multiple", R=0)
    refused("bad shape", V=3)            # W > V
    refused("bad shape", ldl=499)
    refused("bad shape", V=52 * 1024 + 1, ldl=60000)
    refused("eos_id", eos=500)
    refused("eos_id", eos=-1)
    refused("workspace", ws=None)
    refused("workspace", ws_bytes=12 * 4 * 8 - 1)


def test_beam_gather_refuses_before_any_launch():
    lib = L.load()
    keep, p = CA._buf()
    two = (C.c_void_p * 2)(p.value, p.value)

    def gather(caches=two, n_layer=2, ld_seq=32 * 512, ld_row=512, row_bytes=512, par=p, lens=p, R=12, W=4, max_len=32):
        return lib.ergm_beam_gather(caches, n_layer, ld_seq, ld_row, row_bytes, par, lens, R, W, max_len, None)

    def refused(word, **kw):
        assert gather(**kw) == L.ERGM_EINVAL
        assert word in L.last_error(), (word, L.last_error())

    refused("null", caches=None)
    refused("null", par=None)
    refused("null", lens=None)
    refused("outside [1, 8]", W=0)
    refused("outside [1, 8]", W=9, R=18)
    refused("multiple", R=10)
    refused("bad shape", n_layer=0)
    refused("bad shape", max_len=0)
    refused("multiples of 16", row_bytes=24)
    refused("multiples of 16", ld_row=520)
    refused("stride shorter", ld_row=256)
    refused("stride shorter", ld_seq=31 * 512)
    refused("layer 1", caches=(C.c_void_p * 2)(p.value, None))
    refused("layer 0", caches=(C.c_void_p * 2)(p.value + 8, p.value))


def test_run_beams_refuses_before_any_launch():
    lib = L.load()
    plan, keep, p = CA._plan()
    try:
        ptrs = (C.c_void_p * 2)(p.value, p.value)

        def run(n=1, W=2, eos=497, scores=p, toks=p, pars=p, ws=p, ws_bytes=1 << 20, plan=plan):
            return lib.ergm_decode_run_beams(plan, n, W, eos, 499, scores, toks, pars, ws, ws_bytes, None)

        def refused(word, **kw):
            assert run(**kw) == L.ERGM_EINVAL
            assert word in L.last_error(), (word, L.last_error())

        assert run(plan=None) == L.ERGM_EINVAL
        refused("no state bound")
        # slot mode
        assert lib.ergm_decode_bind_slots(plan, ptrs, ptrs, p, p, p, p, p, p, p) == L.ERGM_OK
        refused("slot mode")
        # bound with B = 4 rows, 20 of max_len 32 cache rows in use
        assert lib.ergm_decode_bind(plan, 4, 20, ptrs, ptrs, 8, p, p, p, p) == L.ERGM_OK
        refused("outside [1, 8]", W=0)
        refused("outside [1, 8]", W=9)
        refused("no multiple", W=3)
        refused("n 0", n=0)
        refused("KV cache full", n=13)       # 20 + 13 > 32
        refused("vocabulary", eos=500)
        for name in ("scores", "toks", "pars", "ws"):
            refused("null", **{name: None})
        refused("workspace", ws_bytes=4 * 2 * 8 - 1)
        # the step's launch count is what it was
        assert lib.ergm_decode_launches(plan, 0) - lib.ergm_decode_launches(plan, 1) == 3 * CA.TINY["n_layer"]
    finally:
        lib.ergm_decode_destroy(plan)


def test_fixed_seeds_give_every_select_case_its_margin():
    """The numpy rule alone: every case of tests/test_gpu_beam_ops.py has its margin of 1e-3 at its fixed seed."""
    import test_gpu_beam_ops as BO
    for kind in BO.KINDS:
        for W in (1, 2, 4, 8):
            assert BO.case_margin(kind, W, *BO.SMALL, BO.seed_of(kind, W)) >= BO.MARGIN, (kind, W)
    assert BO.case_margin("live", 4, *BO.LARGE, BO.LARGE_SEED) >= BO.MARGIN


EOS = 9


def test_backtrack_follows_a_beam_that_moved_rows():
    # W = 2, one group, 3 rounds.  Round 1: both children come from row 1 (token 4 stays, token 6 moves to row 0).
    tokens = [[3, 5], [6, 4], [7, 8]]
    parents = [[0, 0], [1, 1], [0, 1]]
    out = beam_backtrack(tokens, parents, [-1.0, -2.0], 2, EOS, num_return=2)
    assert out == [[([5, 6, 7], -1.0), ([5, 4, 8], -2.0)]]


def test_backtrack_ends_at_the_first_eos_and_orders_by_length_penalty():
    # row 0 finished at round 1 and keeps emitting eos; row 1 runs to the bound
    tokens = [[3, 5], [EOS, 4], [EOS, 8], [EOS, 2]]
    parents = [[0, 0], [0, 1], [0, 1], [0, 1]]
    scores = [-3.0, -4.4]
    raw = beam_backtrack(tokens, parents, scores, 2, EOS, length_penalty=0.0, num_return=2)
    assert raw == [[([3, EOS], -3.0), ([5, 4, 8, 2], -4.4)]]
    # -3 / 2 = -1.5 against -4.4 / 4 = -1.1: the longer one first, the sums unchanged
    pen = beam_backtrack(tokens, parents, scores, 2, EOS, length_penalty=1.0, num_return=2)
    assert pen == [[([5, 4, 8, 2], -4.4), ([3, EOS], -3.0)]]
    assert beam_backtrack(tokens, parents, scores, 2, EOS, length_penalty=1.0) == [[([5, 4, 8, 2], -4.4)]]


def test_backtrack_ties_groups_and_dead_rows():
    # two groups of W = 3; group 0: rows 0 and 2 tie (the lower row first), row 1 is dead; group 1: all alive
    tokens = [[1, EOS, 2, 3, 4, 5]]
    parents = [[0, 1, 0, 3, 3, 3]]
    scores = [-2.0, -math.inf, -2.0, -1.5, -0.5, -1.0]
    out = beam_backtrack(tokens, parents, scores, 3, EOS, num_return=3)
    assert out == [[([1], -2.0), ([2], -2.0)], [([4], -0.5), ([5], -1.0), ([3], -1.5)]]
    assert beam_backtrack(tokens, parents, scores, 3, EOS, num_return=1) == [[([1], -2.0)], [([4], -0.5)]]
    for bad in (dict(num_beams=4), dict(num_beams=0), dict(num_return=0), dict(num_return=4)):
        kw = dict(num_beams=3, num_return=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            beam_backtrack(tokens, parents, scores, eos_id=EOS, **kw)
