"""The bounds of tests/_lmscore.py, checked without a GPU from both sides: (a) a plain float32 restatement of
ergm_lm_score's partition and combine order fits its bounds (err/bound <= 1) on every case
tests/test_gpu_lmscore_ops.py runs, and (b) the fp64 result of a slightly WRONG operation, measured against the right
operation's bound, breaches it on the output named.  (c) The planted maxima of the ``edge`` / ``peaked`` / ``tie``
families stand clear of both logit bounds in the fp64 reference itself, so the exact column may be demanded."""
import math

import pytest
import torch

import _lmscore as S


def _admit(c):
    r = S.ref(c)
    b = S.bounds(c, r)
    return S.judge(c, r, b, *S.emu(c)), r, b


def _merge(worst, res):
    for k, v in res.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ---- (a) the float32 restatement fits ------------------------------------------------------------------------------
def test_bound_admits_float32_emulation_on_the_matrix():
    worst = {}
    for args in S.matrix():
        c = S.case(*args)
        res, _, _ = _admit(c)
        assert max(res.values()) <= 1.0, (c.name, res)
        _merge(worst, res)
    print("lm_score matrix: worst emulation err/bound " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("shape", range(len(S.FAMILY_SHAPES)))
def test_bound_admits_float32_emulation_on_the_families(shape):
    R, K, vw = S.FAMILY_SHAPES[shape]
    worst = {}
    for args in S.family_cases():
        if args[:3] != (R, K, vw):
            continue
        c = S.case(*args)
        res, r, b = _admit(c)
        assert max(res.values()) <= 1.0, (c.name, res)
        _merge(worst, res)
    print(f"lm_score families {R}x{K}x{vw[0]}: worst emulation err/bound " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- (c) the planted maxima are decided by the fp64 reference ------------------------------------------------------
@pytest.mark.parametrize("shape", range(len(S.FAMILY_SHAPES)))
def test_planted_margins_exceed_the_logit_bounds(shape):
    R, K, vw = S.FAMILY_SHAPES[shape]
    seen = set()
    for args in S.family_cases():
        if args[:3] != (R, K, vw) or args[3] not in ("edge", "peaked", "tie"):
            continue
        c = S.case(*args)
        r = S.ref(c)
        b = S.bounds(c, r)
        ok = S.margins_ok(c, r, b)
        assert c.planted, c.name
        rows = torch.arange(c.R)
        for row, col in c.planted.items():
            assert int(r.top1[row]) == col, (c.name, row, col, int(r.top1[row]))
            if c.family == "tie":  # an exact tie by construction: the pair stands clear of every third column
                c2 = dict(c.ties)[col]
                assert r.x[row, col] == r.x[row, c2], (c.name, row)
                x = r.x[row].clone()
                x[col] = x[c2] = -math.inf
                third = int(x.argmax())
                assert r.x[row, col] - x[third] > b.x[row, col] + b.x[row, third], (c.name, row)
            else:
                assert bool(ok[row]), (c.name, row, col)
            if c.family == "edge":
                seen.add(col)
                assert bool(r.valid[row]) and int(c.targets[row]) != col or len(S.edges(c.V)) == 1
    assert seen == set(S.edges(vw[0])), "the edge plan must put a maximum on every edge column"


def test_edges_cover_every_tile_and_partition_boundary():
    for V in (203, S.BN, S.BN + 1, S.PW + 1, 50257):
        e = set(S.edges(V))
        assert {0, V - 1} <= e
        for c in range(S.BN, V, S.BN):
            assert {c - 1, c} <= e
        for c in range(S.PW, V, S.PW):
            assert {c - 1, c} <= e


# ---- (b) wrong operations breach -----------------------------------------------------------------------------------
def _breach(c, wrong):
    r = S.ref(c)
    b = S.bounds(c, r)
    w = S.ref(c, wrong)
    return S.judge(c, r, b, w.logprob, w.lse, w.top1_logit, w.top1.int())


EDGE = (33, 192, (S.PW + 1, S.PW + 8), "edge", 0)  # row 0: maximum on V - 1 = PW, alone in the last partition


def test_a_lost_last_column_breaches_lse_and_top1():
    res = _breach(S.case(*EDGE), "lost_last")
    assert res["lse"] > 1e3 and res["top1"] == math.inf, res
    # on benign data the same loss hides below the bound of most rows: the reason the edge family exists
    ben = _breach(S.case(33, 192, (S.PW + 1, S.PW + 8)), "lost_last")
    assert ben["lse"] < res["lse"] / 100, (ben, res)


def test_an_included_pad_row_breaches_lse():
    pads = set()
    for fam in S.FAMILIES:  # pads of 1e4 and of NaN
        c = S.case(33, 192, (S.PW + 1, S.PW + 8), fam, 0)
        assert _breach(c, "col_v")["lse"] > 1e3, c.name
        pads.add(bool(torch.isnan(c.W[-1, 0])))
    assert pads == {True, False}


def test_a_dropped_last_partition_breaches_lse():
    assert _breach(S.case(*EDGE), "drop_last_part")["lse"] > 1e3


def test_a_shifted_target_breaches_logprob():
    res = _breach(S.case(*EDGE), "target_next")
    assert res["logprob"] > 1e3 and res["lse"] == 0.0, res


def test_a_combine_without_rescale_breaches_lse():
    for fam in ("wide", "edge"):
        c = S.case(33, 192, (S.PW + 1, S.PW + 8), fam, 0)
        assert _breach(c, "no_rescale")["lse"] > 10.0, c.name
    # and the float32 restatement without it, measured the same way
    c = S.case(33, 192, (S.PW + 1, S.PW + 8), "wide", 0)
    r = S.ref(c)
    b = S.bounds(c, r)
    keep = S._combine
    try:
        S._combine = lambda *a: keep(*a, rescale=False)
        res = S.judge(c, r, b, *S.emu(c))
    finally:
        S._combine = keep
    assert res["lse"] > 10.0, res


def test_workspace_plan_is_a_function_of_the_vocabulary_only():
    assert S.parts(1) == 1 and S.parts(S.PW) == 1 and S.parts(S.PW + 1) == 2 and S.parts(50257) == 99
