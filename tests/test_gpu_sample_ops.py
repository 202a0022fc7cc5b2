"""ergm_sample_rows and ergm_sample_mark (ergm_amd/csrc/decode.hip) on the GPU: with every control at its default the
new sampler is the old one bit for bit; each control against the fp64 restatement of the rule (tests/_sample.py), with
the margins of tests/test_gpu_decode_ops.py asserted for every row; the bitmap, the minimum length, the
log-probabilities, the distribution of the draws, wild control values, and the marking kernel's clamps."""
import numpy as np
import pytest
import torch

import _sample
import _topp
from ergm_amd import ops

pytestmark = pytest.mark.gpu

EOS = 7
# one token per thread; 5 per thread with threads 1000-1023 holding none (the middle instantiation); the widest
VS = [500, 5000, 50257]
# the rows of tests/test_gpu_decode_ops.py: head probabilities {token: p}, the tail shares the rest evenly
ROWS = [
    {311: 0.30, 12: 0.20, 140: 0.15, 77: 0.10, 499: 0.05},
    {205: 0.80},
    {300: 0.20, 100: 0.20, 40: 0.50},
    {EOS: 0.90, 33: 0.05},
    {1: 0.40, 2: 0.30},
]
SEEN = (311, 12)
# One call: (row, shift, controls, top_p, kept tokens expected or None).  "seen" is the row's bitmap before the call.
CASES = [
    (ROWS[0], 0.0, dict(top_k=4), 0.6, [12, 311]),                 # 3 without the renormalisation over the top-k set
    (ROWS[2], 0.0, dict(top_k=2), 1.0, [40, 100]),                 # the tie at 0.20 resolved by id
    (ROWS[0], 0.0, dict(temp=0.5), 0.6, [12, 311]),
    (ROWS[0], 0.0, dict(rep=2.0, seen=SEEN), 0.6, [77, 140, 311, 499]),   # negative logits: multiplied
    (ROWS[0], 12.0, dict(rep=2.0, seen=SEEN), 0.4, [77, 140]),     # every logit positive: divided ({311} if multiplied)
    (ROWS[0], 0.0, dict(), 0.6, [12, 140, 311]),                   # the plain cut beside them
]
# seeds chosen on the CPU (tests/_sample.py) so that every row of CASES has a draw gap >= 1e-4: {V: seed}
CASE_SEEDS = {500: 1, 5000: 1, 50257: 1}
CHI2_SEED = 1       # the helper's own 4,096 draws with this seed give the chi-square in the test's docstring
MIN_SEED = 1        # with it the helper draws EOS from ROWS[3] at step 0 with a gap >= 1e-4


def _logits(V, rows=ROWS, shift=0.0):
    out = np.empty((len(rows), V), dtype=np.float32)
    for r, head in enumerate(rows):
        p = np.full(V, (1.0 - sum(head.values())) / (V - len(head)))
        for t, v in head.items():
            p[t] = v
        out[r] = (np.log(p) + shift).astype(np.float32)
    return out


def _case_logits(V):
    return np.concatenate([_logits(V, [row], shift) for row, shift, _, _, _ in CASES])


def _words(V):
    return (V + 31) // 32


def _bitmap(B, V, seen_rows, extra=0):
    m = np.zeros((B, _words(V) + extra), dtype=np.uint32)
    for b, ids in enumerate(seen_rows):
        for j in ids:
            m[b, j >> 5] |= np.uint32(1 << (j & 31))
    return m


def _i32(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(gpu)


def _ctl(gpu, B, V, top_p=None, temp=None, rep=None, top_k=None, min_step=None, seen=None):
    """(ergm_sample_ctl, the tensors it points at).  Lists of one value per row; seen a uint32 array [B, >= words]."""
    f = lambda v: None if v is None else torch.tensor(v, dtype=torch.float32, device=gpu)
    i = lambda v: None if v is None else torch.tensor(v, dtype=torch.int64).to(torch.int32).to(gpu)
    t = dict(top_p=f(top_p), temperature=f(temp), rep_penalty=f(rep), top_k=i(top_k), min_step=i(min_step),
             seen=None if seen is None else _i32(seen, gpu))
    return ops.sample_ctl(**t), t


def _run(gpu, logits, V, top_p, seed, ctl=None, steps=None, finished=None, ids=None, logprob=False):
    lg = torch.from_numpy(logits).to(gpu)
    B = lg.shape[0]
    rid = torch.tensor(list(range(B)) if ids is None else ids, dtype=torch.int32, device=gpu)
    rst = torch.tensor([0] * B if steps is None else steps, dtype=torch.int32, device=gpu)
    fin = torch.tensor([0] * B if finished is None else finished, dtype=torch.uint8, device=gpu)
    kept = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    mass = torch.full((B,), -1.0, dtype=torch.float32, device=gpu)
    lp = torch.full((B,), -1.0, dtype=torch.float32, device=gpu) if logprob else None
    tok = ops.sample_rows(lg, V, top_p, seed, rid, rst, EOS, ctl=ctl, finished=fin, kept=kept, kept_mass=mass, logprob=lp)
    torch.cuda.synchronize()
    return dict(tok=tok.cpu(), kept=kept.cpu(), mass=mass.cpu(), fin=fin.cpu(), lp=None if lp is None else lp.cpu())


def _old(gpu, logits, V, top_p, seed, steps=None, finished=None):
    lg = torch.from_numpy(logits).to(gpu)
    B = lg.shape[0]
    rid = torch.arange(B, dtype=torch.int32, device=gpu)
    rst = torch.tensor([0] * B if steps is None else steps, dtype=torch.int32, device=gpu)
    fin = torch.tensor([0] * B if finished is None else finished, dtype=torch.uint8, device=gpu)
    kept = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    mass = torch.full((B,), -1.0, dtype=torch.float32, device=gpu)
    tok = ops.topp_sample_rows(lg, V, top_p, seed, rid, rst, EOS, finished=fin, kept=kept, kept_mass=mass)
    torch.cuda.synchronize()
    return dict(tok=tok.cpu(), kept=kept.cpu(), mass=mass.cpu(), fin=fin.cpu())


def _same(a, b, what):
    for k in ("tok", "kept", "fin"):
        assert torch.equal(a[k], b[k]), (what, k, a[k].tolist(), b[k].tolist())
    assert torch.equal(a["mass"].view(torch.int32), b["mass"].view(torch.int32)), (what, "mass")


def _default_rows(V):
    return np.concatenate([_logits(V), np.random.default_rng(8).normal(size=(2, V)).astype(np.float32)])


@pytest.mark.parametrize("V", VS)
def test_defaults_are_the_old_sampler_bitwise(gpu, V):
    logits = _default_rows(V)
    B = logits.shape[0]
    fin0, steps = [0, 0, 0, 0, 1, 0, 0], [3, 0, 1, 2, 0, 5, 9]
    for top_p in (0.6, 1.0):
        want = _old(gpu, logits, V, top_p, 21, steps, fin0)
        _same(_run(gpu, logits, V, top_p, 21, None, steps, fin0), want, f"V {V} top_p {top_p}, no ctl")
        ctl, keep = _ctl(gpu, B, V, top_p=[top_p] * B, temp=[1.0] * B, rep=[1.0] * B, top_k=[0] * B, min_step=[0] * B,
                         seen=_bitmap(B, V, [()] * B))
        _same(_run(gpu, logits, V, 0.123, 21, ctl, steps, fin0), want, f"V {V} top_p {top_p}, default arrays")


def test_top_p_per_row(gpu):
    V, ps = 500, [0.6, 1.0, 0.3, 0.9]
    logits = _logits(V)[:4]
    ctl, keep = _ctl(gpu, 4, V, top_p=ps)
    got = _run(gpu, logits, V, 0.5, 33, ctl)
    for r, p in enumerate(ps):
        want = _old(gpu, logits, V, p, 33)
        for k in ("tok", "kept", "fin"):
            assert got[k][r] == want[k][r], (r, k)
        assert got["mass"][r].view(torch.int32) == want["mass"][r].view(torch.int32)


def _case_proc(c):
    return dict(seen=c.get("seen", ()), rep=c.get("rep", 1.0), temp=c.get("temp", 1.0))


def _case_ctl(gpu, V, extra_rows=0):
    n = len(CASES) + extra_rows
    pad = [dict()] * extra_rows
    cs = [c for _, _, c, _, _ in CASES] + pad
    return _ctl(gpu, n, V, top_p=[p for _, _, _, p, _ in CASES] + [1.0] * extra_rows, temp=[c.get("temp", 1.0) for c in cs],
                rep=[c.get("rep", 1.0) for c in cs], top_k=[c.get("top_k", 0) for c in cs],
                seen=_bitmap(n, V, [c.get("seen", ()) for c in cs]))


def case_expectations(V, seed):
    """Per row of CASES: (token, gap, kept ids, kept mass, (lo, hi) or None), from the fp64 helper."""
    logits = _case_logits(V)
    out = []
    for r, (_, _, c, top_p, _) in enumerate(CASES):
        proc, k = _case_proc(c), c.get("top_k", 0)
        tok, gap, kept, mass = _sample.draw(logits[r], top_p, _sample.uniform(seed, r, 0), k, **proc)
        out.append((tok, gap, kept, mass, _sample.cut_margin(logits[r], top_p, k, **proc) if top_p < 1.0 else None))
    return out


@pytest.mark.parametrize("V", VS)
def test_known_cuts(gpu, V):
    """Every row of CASES in one call beside a finished row: tokens, kept counts, kept mass and log-probabilities
    against the helper.  The log-probability bound 1e-4: the quantised sum errs by at most V·2^-30 = 5e-5 relative,
    expf by about 2^-22, and x - max by 2^-24·|x - max| with |x - max| <= 32 in these rows."""
    seed = CASE_SEEDS[V]
    logits = np.concatenate([_case_logits(V), _logits(V, [ROWS[4]])])
    exp = case_expectations(V, seed)
    for r, (tok, gap, kept, _, margin) in enumerate(exp):
        if margin is not None:
            lo, hi = margin
            assert lo >= 0.008 and hi >= 0.008 and lo + hi >= 0.02, (r, lo, hi)
        assert gap >= 1e-4, (r, gap)   # a condition of the test: every row qualifies, none is left out
        assert kept.tolist() == CASES[r][4], (r, kept.tolist())
    n = len(CASES)
    ctl, keep = _case_ctl(gpu, V, extra_rows=1)
    got = _run(gpu, logits, V, 0.5, seed, ctl, finished=[0] * n + [1], logprob=True)
    print(f"V {V}: tokens {got['tok'].tolist()} kept {got['kept'].tolist()} mass {got['mass'].tolist()}")
    assert got["tok"].tolist() == [e[0] for e in exp] + [EOS]
    assert got["kept"].tolist() == [e[2].size for e in exp] + [0]
    assert got["fin"].tolist() == [int(e[0] == EOS) for e in exp] + [1]
    worst = 0.0
    for r, (tok, _, kept, mass, _) in enumerate(exp):
        assert abs(got["mass"][r].item() - mass) < 1e-4, (r, got["mass"][r].item(), mass)
        want = _sample.logprob(logits[r], tok, **_case_proc(CASES[r][2]))
        x = _sample.process(logits[r], **_case_proc(CASES[r][2]))
        assert x.max() - x.min() <= 32
        worst = max(worst, abs(got["lp"][r].item() - want))
    print(f"V {V}: largest |logprob - fp64| {worst:.3e}")
    assert worst <= 1e-4
    assert got["lp"][n].item() == 0.0 and got["mass"][n].item() == 0.0
    # the drawn tokens, and only they, joined the bitmaps of the live rows
    seen = keep["seen"].cpu().numpy().view(np.uint32)
    want_seen = _bitmap(n + 1, V, [tuple(c.get("seen", ())) + (exp[r][0],) for r, (_, _, c, _, _) in enumerate(CASES)] + [()])
    assert (seen == want_seen).all()


@pytest.mark.parametrize("V", VS)
def test_top_k_1_is_greedy(gpu, V):
    """The arg-max under 8 seeds, the lowest id on a tie at the top."""
    rows = [ROWS[0], ROWS[2], {300: 0.30, 100: 0.30}, ROWS[3]]
    logits = _logits(V, rows)
    ctl, keep = _ctl(gpu, 4, V, top_k=[1] * 4)
    for seed in range(8):
        got = _run(gpu, logits, V, 1.0, seed, ctl, logprob=True)
        assert got["tok"].tolist() == [311, 40, 100, EOS] and got["kept"].tolist() == [1] * 4
        assert got["fin"].tolist() == [0, 0, 0, 1]
    for r, tok in enumerate([311, 40, 100, EOS]):
        assert abs(got["lp"][r].item() - _sample.logprob(logits[r], tok)) <= 1e-4


def test_bitmap_gets_exactly_the_drawn_tokens(gpu):
    """V = 500 is no multiple of 32; the rows are 2 words longer than a row's bitmap.  Old bits stay, each live row
    gains the bit of its token, the finished row and the words past ceil(V / 32) are untouched."""
    V, B = 500, 5
    logits = _logits(V)
    old = np.random.default_rng(3).integers(0, 2 ** 32, size=(B, _words(V) + 2), dtype=np.uint64).astype(np.uint32)
    ctl, keep = _ctl(gpu, B, V, seen=old)
    got = _run(gpu, logits, V, 0.9, 5, ctl, finished=[0, 0, 0, 0, 1])
    want = old.copy()
    for b in range(4):
        t = int(got["tok"][b])
        want[b, t >> 5] |= np.uint32(1 << (t & 31))
    new = keep["seen"].cpu().numpy().view(np.uint32)
    assert (new == want).all()
    assert (new[:, _words(V):] == old[:, _words(V):]).all() and (new[4] == old[4]).all()


def test_minimum_length_masks_eos(gpu):
    """ROWS[3] gives EOS 0.90.  Below the minimum length it is never drawn over 64 steps, the flags stay 0 and EOS is
    not among the kept; at row_steps == min_step the helper's token is EOS and it is drawn."""
    V = 500
    row = _logits(V, [ROWS[3]])
    logits = np.repeat(row, 8, axis=0)
    ctl, keep = _ctl(gpu, 8, V, min_step=[100] * 8)
    for base in range(0, 64, 8):
        got = _run(gpu, logits, V, 1.0, MIN_SEED, ctl, steps=list(range(base, base + 8)), ids=[0] * 8)
        assert EOS not in got["tok"].tolist() and got["fin"].tolist() == [0] * 8
        assert got["kept"].tolist() == [V - 1] * 8
        for b in (0, 7):
            tok, gap, _, _ = _sample.draw(row[0], 1.0, _sample.uniform(MIN_SEED, 0, base + b), no_eos=EOS)
            if gap >= 1e-4:
                assert got["tok"][b].item() == tok
    tok, gap, kept, _ = _sample.draw(row[0], 1.0, _sample.uniform(MIN_SEED, 0, 0))
    assert tok == EOS and gap >= 1e-4
    ctl, keep = _ctl(gpu, 1, V, min_step=[0])
    got = _run(gpu, row, V, 1.0, MIN_SEED, ctl)
    assert got["tok"].tolist() == [EOS] and got["fin"].tolist() == [1] and got["kept"].tolist() == [V]
    # an unsigned comparison: a step counter at the minimum, wherever that is
    ctl, keep = _ctl(gpu, 1, V, min_step=[41])
    assert _run(gpu, row, V, 1.0, MIN_SEED, ctl, steps=[40])["tok"].item() != EOS
    tok41, gap41, _, _ = _sample.draw(row[0], 1.0, _sample.uniform(MIN_SEED, 0, 41))
    assert gap41 >= 1e-4
    assert _run(gpu, row, V, 1.0, MIN_SEED, ctl, steps=[41])["tok"].item() == tok41


CHI2_HEAD = {9: 0.25, 450: 0.20, 3: 0.15, 120: 0.10, 77: 0.08, 301: 0.06, 18: 0.04, 200: 0.04}


def chi2_of(tokens, kept, expect):
    counts = np.array([(tokens == t).sum() for t in kept])
    return float(((counts - expect) ** 2 / expect).sum()), counts


def test_distribution_with_temperature_and_top_k(gpu):
    """4,096 draws (steps 0 .. 4095, 8 rows a call) of one row with temperature 2 and top_k 8: chi-square against the
    helper's renormalised probabilities below the 99.9 % quantile of 7 degrees of freedom (24.322).  The helper's own
    draws with CHI2_SEED give 8.23."""
    V, n = 500, 4096
    row = _logits(V, [CHI2_HEAD])
    kept, p = _sample.kept_set(row[0], 1.0, 8, temp=2.0)
    assert kept.tolist() == sorted(CHI2_HEAD)
    expect = n * p[kept] / p[kept].sum()
    lg = torch.from_numpy(np.repeat(row, 8, axis=0)).to(gpu)
    ctl, keep = _ctl(gpu, 8, V, temp=[2.0] * 8, top_k=[8] * 8)
    out = torch.empty(n, dtype=torch.int64, device=gpu)
    rid = torch.zeros(8, dtype=torch.int32, device=gpu)
    steps = torch.arange(n, dtype=torch.int32, device=gpu)
    for s in range(0, n, 8):
        ops.sample_rows(lg, V, 1.0, CHI2_SEED, rid, steps[s:s + 8], EOS, ctl=ctl, tokens=out[s:s + 8])
    toks = out.cpu().numpy()
    assert np.isin(toks, kept).all()
    chi2, counts = chi2_of(toks, kept, expect)
    cpu = np.array([_sample.draw(row[0], 1.0, _sample.uniform(CHI2_SEED, 0, s), 8, temp=2.0)[0] for s in range(0, n, 64)])
    print(f"chi-square {chi2:.2f} over {n} draws; counts {counts.tolist()}")
    assert (toks[::64] == cpu).mean() > 0.9   # the same Philox stream as the helper
    assert chi2 < 24.322


@pytest.mark.parametrize("V", VS)
def test_wild_values_act_as_defaults(gpu, V):
    logits = _default_rows(V)
    B = logits.shape[0]
    seen = _bitmap(B, V, [(311, 12, 205, 40, EOS, 1, 2)] * B)   # the penalty would matter if it acted
    want = _old(gpu, logits, V, 0.6, 21)
    nan, inf = float("nan"), float("inf")
    wild = [nan, 0.0, -1.0, inf, -inf, -0.0, nan]
    for what, kw in (("temperature", dict(temp=wild)), ("penalty", dict(rep=wild, seen=seen)),
                     ("top_k", dict(top_k=[-1, -2 ** 31, 2 ** 31 - 1, V, V + 1, 0, 10 ** 6]))):
        ctl, keep = _ctl(gpu, B, V, **kw)
        _same(_run(gpu, logits, V, 0.6, 21, ctl), want, f"V {V}: wild {what}")


def test_sample_mark(gpu):
    """Five sequences over four slots: ragged lengths (one beyond a workgroup's 256 threads, one empty), reset and
    no reset, ids of -1 and V, slots of -1 and n_slots, min_step from non-zero row_steps, and sentinel rows and words
    around the bitmap."""
    V, n_slots, W = 500, 4, _words(500)
    rng = np.random.default_rng(12)
    buf = rng.integers(0, 2 ** 32, size=(n_slots + 2, W + 2), dtype=np.uint64).astype(np.uint32)
    lens = [5, 300, 3, 3, 0]
    slot = [2, 0, -1, n_slots, 3]
    reset = [1, 0, 1, 1, 1]
    min_new = [3, 4, 5, 5, 2]
    seqs = [np.array([4, -1, V, 499, 4])] + [rng.integers(0, V, size=n) for n in lens[1:]]
    ids = np.concatenate(seqs).astype(np.int64)
    start = np.concatenate(([0], np.cumsum(lens)[:-1])).tolist()
    row_steps = [7, 11, 13, 17]
    ms0 = [1000, 1001, 1002, 1003]
    want, want_ms = buf.copy(), list(ms0)
    for b, sl in enumerate(slot):
        if not 0 <= sl < n_slots:
            continue
        if reset[b]:
            want[1 + sl, :W] = 0
        for j in seqs[b]:
            if 0 <= j < V:
                want[1 + sl, j >> 5] |= np.uint32(1 << (int(j) & 31))
        want_ms[sl] = row_steps[sl] + min_new[b]
    whole = _i32(buf, gpu)
    seen = whole[1:1 + n_slots]
    i = lambda v: torch.tensor(v, dtype=torch.int32, device=gpu)
    ms = i(ms0)
    ops.sample_mark(torch.from_numpy(ids).to(gpu), i(slot), i(start), i(lens), V, seen=seen, reset=i(reset), min_new=i(min_new),
                    row_steps=i(row_steps), min_step=ms, n_slots=n_slots)
    torch.cuda.synchronize()
    got = whole.cpu().numpy().view(np.uint32)
    assert (got == want).all()
    assert (got[0] == buf[0]).all() and (got[-1] == buf[-1]).all() and (got[:, W:] == buf[:, W:]).all()
    assert (got[2] == buf[2]).all()   # slot 1: nobody's
    assert ms.cpu().tolist() == want_ms == [11, 1001, 16, 19]
    # wild starts and lengths are clamped to the packed array: nothing is read past it
    ops.sample_mark(torch.from_numpy(ids).to(gpu), i([1, 3]), i([10 ** 9, -5]), i([2, 10 ** 9]), V, seen=seen,
                    reset=i([1, 0]), n_slots=n_slots)
    torch.cuda.synchronize()
    got = whole.cpu().numpy().view(np.uint32)
    want[2, :W] = 0
    for sl, part in ((1, ids[-2:]), (3, ids)):   # the first sequence is the array's last two ids, the second all of it
        for j in part:
            if 0 <= j < V:
                want[1 + sl, j >> 5] |= np.uint32(1 << (int(j) & 31))
    assert (got == want).all()
