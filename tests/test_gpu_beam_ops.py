"""ergm_beam_select and ergm_beam_gather (ergm_amd/csrc/beam.hip) on the GPU.  Select against the numpy restatement of
the rule (tests/_beam.py): the same set of (parent, token) per group, the slot-assignment property, the flags, and the
scores within 1e-4 (c is three f32 roundings and one f32 logarithm on magnitudes below 128, under 4 ulp = 3e-5; the
integer mass adds at most V·2^-30 = 4.7e-5 at V = 50,260).  A case counts only with a margin of at least 1e-3 between
the W-th and the (W+1)-th candidate of every group; the seeds are fixed so that the helper alone gives every case that
margin, which is asserted, so no case is skipped.  Gather against a numpy copy: bitwise, with canaries."""
import math

import numpy as np
import pytest
import torch

import _beam
from ergm_amd import ops

pytestmark = pytest.mark.gpu
EOS = 497
MARGIN = 1e-3
TOL = 1e-4
KINDS = ("live", "round0", "one_finished", "all_finished", "ties", "nan_logit", "sparse")
SMALL, LARGE = (3, 500, 512), (2, 50260, 50304)   # G, V, ldl


def make_case(kind, W, G, V, ldl, seed):
    """logits [R, ldl] f32 (the padding columns NaN: they are not part of the row), scores [R] f32, finished [R]."""
    rng = np.random.default_rng(1000 * seed + 10 * W + KINDS.index(kind))
    R = G * W
    logits = np.full((R, ldl), np.nan, dtype=np.float32)
    logits[:, :V] = (3.0 * rng.standard_normal((R, V))).astype(np.float32)
    scores = (-5.0 * rng.random(R)).astype(np.float32)
    fin = np.zeros(R, dtype=np.uint8)
    if kind == "round0":
        scores[:] = -np.inf
        scores[::W] = 0.0
        for r in range(R):
            if r % W:
                logits[r] = np.nan
    elif kind == "one_finished":
        fin[W // 2::W] = 1      # one beam of every group (the only one at W = 1)
        scores[W // 2::W] = -0.5
    elif kind == "all_finished":
        fin[:] = 1
    elif kind == "ties":
        # beams 0 and 1 of every group: bitwise-equal rows and equal scores, the two best logits of the row equal too;
        # the other beams dead.  W = 1 has one beam: the tie is between its two best tokens.
        scores[:] = -np.inf
        for g0 in range(0, R, W):
            a, b = sorted(rng.choice(V, 2, replace=False).tolist())
            logits[g0, a] = logits[g0, b] = np.float32(logits[g0, :V].max() + 1.0)
            scores[g0] = -1.25
            if W > 1:
                logits[g0 + 1] = logits[g0]
                scores[g0 + 1] = scores[g0]
            for r in range(g0 + 2, g0 + W):
                logits[r] = np.nan
    elif kind == "nan_logit":
        for r in range(R):
            logits[r, rng.choice(V, 5, replace=False)] = np.nan
            logits[r, int(np.nanargmax(logits[r, :V]))] = np.nan   # the best token of the row among them
            logits[r, rng.integers(V)] = np.inf                    # not finite: no candidate, no part of the maximum
    elif kind == "sparse":
        # fewer than W candidates: one live beam per group with two finite logits, the others dead
        scores[:] = -np.inf
        scores[::W] = -0.75
        keep = logits[::W, :2].copy()
        logits[:] = np.nan
        logits[::W, 5:7] = keep
    return logits, scores, fin


def case_margin(kind, W, G, V, ldl, seed):
    logits, scores, fin = make_case(kind, W, G, V, ldl, seed)
    ref = _beam.select(logits[:, :V], scores, fin, W, EOS)
    return min(ref["strict"] if kind == "ties" else ref["margin"])


# The first seed (from 0) at which the helper gives every group of the case the margin, where that is not seed 0; found
# on the CPU, and asserted there for every case (tests/test_beam_abi.py) and again in each GPU case.
SEEDS = {}
LARGE_SEED = 0


def seed_of(kind, W):
    return SEEDS.get((kind, W), 0)


def check_select(gpu, kind, W, G, V, ldl, seed):
    logits, scores, fin = make_case(kind, W, G, V, ldl, seed)
    R = G * W
    finite = logits[:, :V][np.isfinite(logits[:, :V])]
    assert np.abs(finite).max() < 128 and np.abs(scores[np.isfinite(scores)]).max(initial=0) < 128
    ref = _beam.select(logits[:, :V], scores, fin, W, EOS)
    margin = min(ref["strict"] if kind == "ties" else ref["margin"])
    print(f"{kind} W={W} V={V}: margin {margin:.3e}")
    assert margin >= MARGIN, (kind, W, seed, margin)
    lg = torch.from_numpy(logits).to(gpu)
    outs = []
    for _ in range(2):   # twice from the same state: the same bits
        sc, fl = torch.from_numpy(scores).to(gpu), torch.from_numpy(fin).to(gpu)
        parent, token = ops.beam_select(lg, V, W, sc, fl, EOS)
        outs.append((parent.cpu().numpy(), token.cpu().numpy(), sc.cpu().numpy(), fl.cpu().numpy()))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    parent, token, sc, fl = outs[0]
    assert ((parent >= 0) & (parent < R)).all() and ((token >= 0) & (token < V)).all()
    dead = np.isneginf(ref["score"])
    for g in range(G):
        rows = [r for r in range(g * W, (g + 1) * W) if not dead[r]]
        got = {(int(parent[r]), int(token[r])) for r in rows}
        assert got == ref["pairs"][g], (kind, W, g, got, ref["pairs"][g])
    assert _beam.slot_property(parent, token, W)
    # with the set and the property the rows are the helper's
    assert parent.tolist() == ref["parent"].tolist() and token.tolist() == ref["token"].tolist()
    assert fl.tolist() == ref["finished"].tolist()
    assert np.isneginf(sc[dead]).all() and (parent[dead] == np.nonzero(dead)[0]).all() and (token[dead] == EOS).all()
    err = np.abs(sc[~dead].astype(np.float64) - ref["score"][~dead])
    print(f"    max |score - fp64| {err.max(initial=0):.3e}")
    assert err.max(initial=0) <= TOL
    return parent, token, sc, fl


@pytest.mark.parametrize("W", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_select_small(gpu, kind, W):
    check_select(gpu, kind, W, *SMALL, seed_of(kind, W))


def test_select_ties_resolve_by_beam_then_token(gpu):
    """W = 2, beams 0 and 1 bitwise equal with their two best tokens a < b equal: four equal candidates, and the two
    taken are (beam 0, a) and (beam 0, b): row 0 keeps a, b goes to the childless row 1."""
    parent, token, sc, _ = check_select(gpu, "ties", 2, *SMALL, seed_of("ties", 2))
    for g0 in (0, 2, 4):
        assert parent[g0] == parent[g0 + 1] == g0 and token[g0] < token[g0 + 1]
        assert sc[g0].tobytes() == sc[g0 + 1].tobytes()


def test_select_large_vocabulary(gpu):
    check_select(gpu, "live", 4, *LARGE, LARGE_SEED)


def test_gather(gpu):
    """Two layers, G = 2, W = 4, 32 cache rows of 512 bytes.  Group 0: beam 0 has three children (rows 0, 1, 3), beam 2
    keeps its row, beams 1 and 3 are childless.  Group 1: row 4 self, row 5 names a parent outside its group (self),
    row 6 self, row 7 follows 6.  A second call with parents out of every range changes nothing."""
    R, W, rows, width, n_layer = 8, 4, 32, 128, 2
    parent = np.array([0, 0, 2, 0, 4, 2, 6, 6], dtype=np.int32)
    lens = np.array([5, 9, 7, 3, 11, 2, 6, 1], dtype=np.int32)
    canary = 64
    bufs, caches, before = [], [], []
    for l in range(n_layer):
        buf = torch.full((R * rows * width + canary,), -7 - l, dtype=torch.int32, device=gpu)
        c = buf[:R * rows * width].view(R, rows, width)
        # every element encodes (layer, slot, row, column)
        c.copy_((torch.arange(R * rows * width, dtype=torch.int32, device=gpu) + (l << 24)).view(R, rows, width))
        bufs.append(buf), caches.append(c), before.append(buf.cpu().numpy().copy())
    p_d, l_d = torch.from_numpy(parent).to(gpu), torch.from_numpy(lens).to(gpu)
    ops.beam_gather(caches, p_d, l_d, W)
    moved = {1: 0, 3: 0, 7: 6}
    want_lens = lens.copy()
    for r, p in moved.items():
        want_lens[r] = lens[p]
    assert l_d.cpu().tolist() == want_lens.tolist()
    for l in range(n_layer):
        want = before[l].copy()
        w3 = want[:R * rows * width].reshape(R, rows, width)
        src = before[l][:R * rows * width].reshape(R, rows, width)
        for r, p in moved.items():
            w3[r, :lens[p]] = src[p, :lens[p]]
        assert bufs[l].cpu().numpy().tobytes() == want.tobytes(), l   # the rows past the length, the other slots, the canary
    # nothing moves: every parent self, out of its group or out of every range
    state = [b.cpu().numpy().copy() for b in bufs]
    lens2 = l_d.cpu().numpy().copy()
    p_d = torch.tensor([0, -1, 2, 7, 4, 100, 6, 2 ** 31 - 1], dtype=torch.int32, device=gpu)
    ops.beam_gather(caches, p_d, l_d, W)
    # a parent that does not keep its own row counts as self too (row 1 -> 2 while 2 -> 3)
    p_d = torch.tensor([0, 2, 3, 3, 4, 5, 6, 7], dtype=torch.int32, device=gpu)
    ops.beam_gather(caches, p_d, l_d, W)
    assert l_d.cpu().tolist()[:2] == lens2.tolist()[:2]
    assert l_d.cpu().tolist()[2] == lens2[3]   # 2 -> 3 is a plain move
    for l in range(n_layer):
        now = bufs[l].cpu().numpy()
        w3 = state[l][:R * rows * width].reshape(R, rows, width)
        w3[2, :lens2[3]] = w3[3, :lens2[3]].copy()
        assert now.tobytes() == state[l].tobytes(), l


def test_gather_bounded_by_max_len(gpu):
    """max_len below the cache's rows (the generator's bound on the lengths): the copy stops there."""
    R, W, rows, width = 2, 2, 32, 128
    c = torch.arange(R * rows * width, dtype=torch.int32, device=gpu).view(R, rows, width).contiguous()
    before = c.cpu().numpy().copy()
    p_d = torch.tensor([0, 0], dtype=torch.int32, device=gpu)
    l_d = torch.tensor([20, 3], dtype=torch.int32, device=gpu)
    ops.beam_gather([c], p_d, l_d, W, max_len=12)
    want = before.copy()
    want[1, :12] = before[0, :12]
    assert c.cpu().numpy().tobytes() == want.tobytes() and l_d.cpu().tolist() == [20, 12]


