"""The attention bound of tests/_attn.py, checked without a GPU from both sides: (a) a plain float32 evaluation with
the kernels' rounding points fits it on every case tests/test_gpu_attn_matrix.py runs, and (b) the fp64 result of a
slightly WRONG operation (one key lost from one row, one pair at a tile corner masked, the diagonal shifted by one,
the last key dropped, one keep bit flipped, the row sum taken after dropping) breaches it.  A bound loose enough to
admit (b) or tight enough to reject (a) is wrong; neither side is tuned to the other."""
import math

import pytest
import torch

import _attn as A


def _emulate(c, r, bf):
    """err/bound of the float32 emulation on O, LSE and, for the backward fed the reference's bf16 O / fp32 LSE and
    fed the emulation's own, on dQ, dK, dV; each output also through the whole-tensor norm gate, as on the GPU."""
    q, k, v, do = c.q.float(), c.k.float(), c.v.float(), c.do.float()
    o, lse = A.emu_fwd(q, k, v, c.vis, c.Z)
    out = {"O": A.ratio(o, r.O, bf["O"]), "LSE": A.ratio(lse, r.LSE, bf["LSE"])}
    A.norm_gate(c.name, "O", o, r.O)
    A.norm_gate(c.name, "LSE", lse, r.LSE)
    for tag, (o_in, lse_in) in (("ref", (r.O.bfloat16(), r.LSE.float())), ("own", (o, lse))):
        rb, bb = A.case_bwd(c, o_in, lse_in)
        got = A.emu_bwd(q, k, v, do, o_in.float(), lse_in, c.vis, c.Z)
        for n, g in zip(("dQ", "dK", "dV"), got):
            out[f"{n}/{tag}"] = A.ratio(g, getattr(rb, n), bb[n])
            A.norm_gate(f"{c.name} fed {tag}", n, g, getattr(rb, n), n not in A.ungated(c))
    return out


def _admit(args):
    c, r, bf = A.case_fwd(*args)
    ratios = _emulate(c, r, bf)
    print(f"{c.name}: emulation err/bound " + "  ".join(f"{k} {x:.3f}" for k, x in ratios.items()))
    assert max(ratios.values()) <= 1.0, (c.name, ratios)
    return max(ratios.values())


@pytest.mark.parametrize("Sq,Sk,causal,family,scale", A.SELF_CHECK, ids=lambda x: str(x))
def test_bound_admits_float32_emulation(Sq, Sk, causal, family, scale):
    """The emulation fits the bound on nine cases at B = H = 1: benign, q and k scaled x0.25 .. x10, a late maximum."""
    _admit((Sq, Sk, causal, (1, 1), family, scale))


def test_bound_admits_float32_emulation_on_the_gpu_matrix():
    """The emulation fits the bound on every case of the GPU matrix: all lengths, input families and dropout shapes."""
    worst = 0.0
    for Sq, Sk, causal, bh in A.LENGTHS:
        worst = max(worst, _admit((Sq, Sk, causal, bh)))
    for Sq, Sk, causal, bh in A.FAMILY_SHAPES:
        for fam in A.FAMILIES:
            worst = max(worst, _admit((Sq, Sk, causal, bh, fam)))
    for Sq, Sk, causal, bh in A.DROP_SHAPES:
        worst = max(worst, _admit((Sq, Sk, causal, bh, "benign", 1.0, True)))
    print(f"worst emulation err/bound over the matrix: {worst:.3f}")


# ---- wrong operations -----------------------------------------------------------------------------------------------
def _lose(vis, row, key):
    vis = vis.clone()
    vis[row, key] = False
    return vis


# name -> (applies to causal?, to non-causal?, visibility of the wrong operation, the pair _draw looks at)
MUTATIONS = {
    "key 64 lost from row 100": (True, True, lambda vis: _lose(vis, 100, 64), (100, 64)),
    "diagonal pair (128, 128) masked": (True, False, lambda vis: _lose(vis, 128, 128), (128, 128)),
    "diagonal shifted: key <= q + 1": (True, False, lambda vis: torch.ones_like(vis).tril(1), None),
    "last key lost from every row": (False, True, lambda vis: _lose(vis, slice(None), vis.shape[1] - 1), None),
}
SHAPES = {"causal 192": (192, 192, True), "129x200": (129, 200, False)}


def _draw(Sq, Sk, causal, drop, pair=(100, 64)):
    """The data of the mutation checks.  A pair that carries next to no weight, or whose dP*Z - delta is next to zero,
    can be lost without changing anything a test could see, so the checks run on the first draw (benign randn inputs)
    in which the pair the mutation removes or flips carries at least the mean weight of its row and an above-RMS
    |dP/(1-p) - delta|.  The criterion reads the fp64 reference only; the chosen draw is printed.  On draw 0 the pair
    (100, 64) of 129x200 has a tenth of the mean weight and its loss stays at 0.2x of the bound on O: an arbitrary
    pair can go unseen, by this gate as by any other.  (Breach factors quoted elsewhere for these mutations, such as
    a smallest one of 1.44x, were measured on other data and are not comparable with the ones printed here.)
    ``pair`` = None (a mutation of the whole mask): draw 0."""
    if pair is None:
        return 0
    i, j = pair
    for salt in range(256):
        c, r, _ = A.case_fwd(Sq, Sk, causal, (1, 1), "benign", 1.0, drop, salt)
        _, _, rb, _ = A.case_bwd_ref_fed(Sq, Sk, causal, (1, 1), "benign", 1.0, drop, salt)
        scale = 1.0 / (1.0 - A.DROP["p"]) if drop else 1.0
        g = (rb.dP * scale - rb.delta[..., None])[0, 0]
        n = int(c.vis[i].sum())
        rms = g[i][c.vis[i]].pow(2).mean().sqrt().item()
        if r.P[0, 0, i, j].item() * n >= 1.0 and abs(g[i, j].item()) >= rms:
            print(f"{'causal ' if causal else ''}{Sq}x{Sk}{', dropout' if drop else ''}, pair {pair}: draw {salt}, "
                  f"weight {r.P[0, 0, i, j].item() * n:.2f} x the row's mean")
            return salt
    raise AssertionError("no draw meets the criterion")


def _breaches(c, bf, wrong_fwd, wrong_vis, wrong_Z, outs):
    """err/bound of the wrong operation's fp64 results against the RIGHT operation's bounds; its backward is the
    formula on its own (bf16) O and (fp32) LSE."""
    q, k, v, do = c.q.double(), c.k.double(), c.v.double(), c.do.double()
    _, _, rb, bb = A.case_bwd_ref_fed(c.Sq, c.Sk, c.causal, (c.B, c.H), c.family, 1.0, c.drop is not None, c.salt)
    _, r, _ = A.case_fwd(c.Sq, c.Sk, c.causal, (c.B, c.H), c.family, 1.0, c.drop is not None, c.salt)
    w = A.ref_bwd(q, k, v, do, wrong_fwd.O.bfloat16().double(), wrong_fwd.LSE.float().double(), wrong_vis, wrong_Z)
    res = {"O": A.ratio(wrong_fwd.O, r.O, bf["O"]), "LSE": A.ratio(wrong_fwd.LSE, r.LSE, bf["LSE"])}
    for n in ("dQ", "dK", "dV"):
        res[n] = A.ratio(getattr(w, n), getattr(rb, n), bb[n])
    return {n: res[n] for n in outs}


@pytest.mark.parametrize("mutation,shape", [(m, s) for m in MUTATIONS for s in SHAPES
                                            if MUTATIONS[m][0 if SHAPES[s][2] else 1]])
def test_bound_rejects_wrong_mask(mutation, shape):
    """Each wrong mask breaches the bound on O, on LSE and on each of dQ, dK, dV (B = H = 1, benign inputs)."""
    Sq, Sk, causal = SHAPES[shape]
    mutate, pair = MUTATIONS[mutation][2:]
    c, r, bf = A.case_fwd(Sq, Sk, causal, (1, 1), "benign", 1.0, False, _draw(Sq, Sk, causal, False, pair))
    vis = mutate(c.vis)
    assert not torch.equal(vis, c.vis)
    q, k, v = c.q.double(), c.k.double(), c.v.double()
    res = _breaches(c, bf, A.ref_fwd(q, k, v, vis), vis, None, ("O", "LSE", "dQ", "dK", "dV"))
    print(f"{shape}, {mutation}: breach " + "  ".join(f"{n} {x:.3g}x" for n, x in res.items()))
    assert min(res.values()) > 1.0, res


@pytest.mark.parametrize("shape", SHAPES)
def test_bound_rejects_wrong_dropout(shape):
    """With dropout (p = 0.1): one keep bit flipped at a visible pair breaches O, dQ, dK and dV (the LSE is taken
    before dropping and does not depend on the bits); the row sum taken after dropping instead of before breaches
    all five."""
    Sq, Sk, causal = SHAPES[shape]
    c, r, bf = A.case_fwd(Sq, Sk, causal, (1, 1), "benign", 1.0, True, _draw(Sq, Sk, causal, True))
    q, k, v = c.q.double(), c.k.double(), c.v.double()
    keep = c.keep.clone()
    keep[0, 0, 100, 64] = ~keep[0, 0, 100, 64]
    Z = keep.double() / (1.0 - A.DROP["p"])
    res = _breaches(c, bf, A.ref_fwd(q, k, v, c.vis, Z), c.vis, Z, ("O", "dQ", "dK", "dV"))
    print(f"{shape}, keep bit (100, 64) flipped: breach " + "  ".join(f"{n} {x:.3g}x" for n, x in res.items()))
    assert min(res.values()) > 1.0, res
    res = _breaches(c, bf, A.ref_fwd(q, k, v, c.vis, c.Z, sum_after_drop=True), c.vis, c.Z,
                    ("O", "LSE", "dQ", "dK", "dV"))
    print(f"{shape}, row sum after dropping: breach " + "  ".join(f"{n} {x:.3g}x" for n, x in res.items()))
    assert min(res.values()) > 1.0, res


def test_reference_matches_autograd():
    """The backward formula with o_in, lse_in = the forward's own fp64 results is the autograd gradient of the
    forward (dropout included): the reference the bound is built around is the operation itself."""
    c = A.make_case(70, 90, False, (2, 2), "benign", 1.0, True)
    q, k, v = (t.double().requires_grad_(True) for t in (c.q, c.k, c.v))
    r = A.ref_fwd(q, k, v, c.vis, c.Z)
    r.O.backward(c.do.double())
    rb = A.ref_bwd(q.detach(), k.detach(), v.detach(), c.do.double(), r.O.detach(), r.LSE.detach(), c.vis, c.Z)
    for got, want in ((rb.dQ, q.grad), (rb.dK, k.grad), (rb.dV, v.grad)):
        assert (got - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item())


def test_ratio_counts_nan_as_a_breach():
    one = torch.ones(1, dtype=torch.float64)
    assert A.ratio(torch.tensor([math.nan]), 0.0 * one, one) == math.inf
