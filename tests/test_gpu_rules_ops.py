"""ergm_logit_rules_apply and the history kernels (ergm_hist_write, ergm_hist_append, ergm_hist_follow) against the plain
Python rule of tests/_rules.py, whole buffers compared bit for bit inside guarded allocations (the sentinel style of
tests/test_gpu_rows_matrix.py): the logits sit at element 8 of a sentinel buffer with the pad columns [V, ldl) part of
the surround, and every input the kernel must leave alone is compared with what it held before.

The rows come from _rules.cases: n in {1, 2, 3, 8} at L in {0, 1, n-2, n-1, n, max_len} over a 3-token alphabet, a match
straddling s0, s0 > L and < 0, eos at a banned position, entries -1 and V, the bad-word lists (one-token words, a prefix
that is the tail and one that is one off, a word longer than the history, a full pool, a zero length in front, a cut
sequence), finished rows and rows with everything off beside ruled ones, and lens of -5 and max_len + 7.  They run in
launches of R = 1, 5 and 33 rows at V = 500 / ldl = 512 / max_len = 64, once at V = 50,260 / ldl = 50,304, and once at
max_len = 1,024 with rows at L = 1,024 exactly."""
import numpy as np
import pytest
import torch

import _rules
from test_gpu_rows_matrix import Guard
from ergm_amd import ops

pytestmark = pytest.mark.gpu
i32, i64, f32, u8 = torch.int32, torch.int64, torch.float32, torch.uint8
EOS, CAP = 11, 64
ISENT = -12288


def _launch(rows, V, ldl, max_len, gpu, seed, twice=False, drop=()):
    """One ergm_logit_rules_apply over ``rows``; checks the whole logits buffer against _rules.apply and that nothing
    else changed.  Returns the logits after the call (CPU)."""
    R = len(rows)
    g = torch.Generator().manual_seed(seed)
    host = torch.randn(R, V, generator=g, dtype=f32)
    logits = Guard(R, V, f32, gpu, init=host, ld=ldl)
    hist_h = torch.tensor([r["hist"] for r in rows], dtype=i32)
    hist = Guard(R, max_len, i32, gpu, init=hist_h, ld=max_len + 8, fill=ISENT)
    dev = lambda k, dt=i32: torch.tensor([r[k] for r in rows], dtype=dt, device=gpu)
    lens, start, ngram, fin = dev("len"), dev("start"), dev("ngram"), dev("finished", u8)
    bad_h = torch.tensor([r["bad"] for r in rows], dtype=i32)
    bad = Guard(R, CAP, i32, gpu, init=bad_h, ld=CAP, fill=ISENT)   # rows back to back: a run that overran its row
    kw = dict(start=start, ngram=ngram, bad=bad.view)               # would read the next row's
    for k in drop:
        kw[k] = None
    rules = ops.rules_desc(hist.view, **kw)
    ops.logit_rules(logits.view, V, rules, lens, EOS, max_len, finished=fin)
    if twice:
        ops.logit_rules(logits.view, V, rules, lens, EOS, max_len, finished=fin)
    want = _rules.apply(host.numpy(), V, hist_h.tolist(), [r["len"] for r in rows], EOS, max_len,
                        start=None if "start" in drop else [r["start"] for r in rows],
                        ngram=None if "ngram" in drop else [r["ngram"] for r in rows],
                        bad=None if "bad" in drop else bad_h.tolist(), finished=[r["finished"] for r in rows])
    got = logits.cpu()
    assert logits.intact(), "wrote outside the logits rows (pad columns or surround)"
    assert got.numpy().tobytes() == want.tobytes()
    assert hist.intact() and torch.equal(hist.cpu(), hist_h) and torch.equal(bad.cpu(), bad_h)
    return got, want, host


@pytest.mark.parametrize("R", [1, 5, 33])
def test_rules_against_the_python_rule(gpu, R):
    rows = _rules.cases(500, EOS, 64, CAP)
    assert len(rows) >= 40
    banned_any = untouched_beside = 0
    for k in range(0, len(rows), R):
        chunk = rows[k:k + R]
        got, want, host = _launch(chunk, 500, 512, 64, gpu, seed=k)
        hit = (want != host.numpy()).any(axis=1)
        banned_any += int(hit.sum())
        untouched_beside += int(hit.any() and not hit.all())
    assert banned_any >= 15                 # the cases ban: the comparison is not between two untouched buffers
    assert R == 1 or untouched_beside >= 1  # finished / unruled rows sat beside ruled ones and kept their bits


def test_cases_ban_what_they_say(gpu):
    """A few rows by hand, so the helper is not the only witness."""
    a, b, c = 3, 499, 7
    rows = _rules.cases(500, EOS, 64, CAP)
    pick = lambda **kw: next(r for r in rows if all(r[k] == v for k, v in kw.items()))
    r1 = pick(start=2, ngram=2)                                           # [c, a, b, c, c, a], s0 = 2: (a, b) straddles
    r2 = dict(r1, start=1)
    got, _, host = _launch([r1, r2], 500, 512, 64, gpu, seed=1)
    assert torch.equal(got[0], host[0])                                   # nothing banned
    assert set(torch.nonzero(got[1] != host[1]).flatten().tolist()) == {b}
    words = [dict(hist=[c, c, a, b] + [a] * 60, len=4, start=0, ngram=0, finished=0, bad=_rules.pool([(a, b, c)], CAP)),
             dict(hist=[c, a, b, c] + [a] * 60, len=4, start=0, ngram=0, finished=0, bad=_rules.pool([(a, b, c)], CAP))]
    got, _, host = _launch(words, 500, 512, 64, gpu, seed=2)
    assert set(torch.nonzero(got[0] != host[0]).flatten().tolist()) == {c} and got[0, c] == -np.inf
    assert torch.equal(got[1], host[1])


def test_null_members_turn_a_rule_off(gpu):
    rows = _rules.cases(500, EOS, 64, CAP)[:33]
    for drop in (("start",), ("ngram",), ("bad",), ("ngram", "bad"), ("start", "ngram", "bad")):
        _launch(rows, 500, 512, 64, gpu, seed=3, drop=drop)


def test_full_vocabulary(gpu):
    V = 50260
    rows = _rules.cases(V, EOS, 64, CAP)
    five = [r for r in rows if r["ngram"] in (1, 3) and r["len"] == 64][:2] + [r for r in rows if any(r["bad"])][:2] + rows[-4:-3]
    assert len(five) == 5
    _, want, host = _launch(five, V, 50304, 64, gpu, seed=4)
    assert (want[:, V - 1] == -np.inf).any()   # b = V - 1, the last column, is banned somewhere


def test_longest_history(gpu):
    rows = _rules.cases(500, EOS, 1024, CAP, seed=5)
    full = [r for r in rows if r["len"] == 1024]
    assert len(full) >= 4 and {r["ngram"] for r in full} == {1, 2, 3, 8}
    _launch(full + rows[:12], 500, 512, 1024, gpu, seed=5)


def test_same_bits_every_run_and_idempotent(gpu):
    rows = _rules.cases(500, EOS, 64, CAP)[:33]
    first, _, _ = _launch(rows, 500, 512, 64, gpu, seed=6)
    again, _, _ = _launch(rows, 500, 512, 64, gpu, seed=6)
    twice, _, _ = _launch(rows, 500, 512, 64, gpu, seed=6, twice=True)
    assert first.numpy().tobytes() == again.numpy().tobytes() == twice.numpy().tobytes()


# ---- the history kernels ----------------------------------------------------------------------------------------
def _i(v, gpu, dt=i32):
    return torch.tensor(v, dtype=dt, device=gpu)


def test_hist_write(gpu):
    max_len, n_slots, total = 16, 4, 40
    ids_h = list(range(100, 100 + total))
    ids_h[2], ids_h[3] = -7, 2 ** 31 + 5            # no int32 / negative: stored as -1
    #        slot start len  pos0
    seqs = [(0, 0, 5, 0),
            (2, 5, 6, max_len - 1),                 # one token lands, at the last position
            (1, 11, 4, max_len),                    # nothing lands
            (-1, 0, 5, 0), (n_slots, 0, 5, 0),      # slots outside the table
            (3, 35, 100, -3)]                       # len clamped to total, start to total - len, pos0 to 0, the rest cut at max_len
    hist = Guard(n_slots, max_len, i32, gpu, init=ISENT + 1, ld=max_len + 8, fill=ISENT)
    col = lambda k: _i([s[k] for s in seqs], gpu)
    ops.hist_write(_i(ids_h, gpu, i64), col(0), col(1), col(2), hist.view, max_len, pos0=col(3), n_slots=n_slots)
    want = np.full((n_slots, max_len), ISENT + 1, dtype=np.int64)
    for sl, st, ln, p0 in seqs:
        if not 0 <= sl < n_slots:
            continue
        n = _rules.clamp(ln, 0, total)
        s0 = _rules.clamp(st, 0, total - n)
        p0 = _rules.clamp(p0, 0, max_len)
        for i in range(min(n, max_len - p0)):
            v = ids_h[s0 + i]
            want[sl, p0 + i] = v if 0 <= v < 2 ** 31 else -1
    assert hist.intact()
    assert hist.cpu().tolist() == want.tolist()
    assert want[0, 2] == -1 and want[0, 3] == -1 and want[2, max_len - 1] == 105 and (want[1] == ISENT + 1).all()
    # pos0 = None is position 0
    h2 = Guard(n_slots, max_len, i32, gpu, init=ISENT + 1, ld=max_len, fill=ISENT)
    ops.hist_write(_i(ids_h, gpu, i64), _i([1], gpu), _i([4], gpu), _i([3], gpu), h2.view, max_len)
    assert h2.intact() and h2.cpu()[1, :4].tolist() == [104, 105, 106, ISENT + 1]


def test_hist_append(gpu):
    max_len = 16
    lens = [0, 5, max_len - 1, max_len, -1, 7, max_len + 9]
    fin = [0, 0, 0, 0, 0, 1, 0]
    toks = [41, 42, 43, 44, 45, 46, 47]
    R = len(lens)
    for finished in (_i(fin, gpu, u8), None):
        hist = Guard(R, max_len, i32, gpu, init=ISENT + 1, ld=max_len + 8, fill=ISENT)
        ops.hist_append(_i(toks, gpu, i64), _i(lens, gpu), hist.view, max_len, finished=finished)
        want = np.full((R, max_len), ISENT + 1, dtype=np.int64)
        for r in range(R):
            if 0 <= lens[r] < max_len and not (finished is not None and fin[r]):
                want[r, lens[r]] = toks[r]
        assert hist.intact() and hist.cpu().tolist() == want.tolist()
        assert (want != ISENT + 1).sum() == (3 if finished is not None else 4)


def test_hist_follow_matches_a_host_gather(gpu):
    max_len, W = 16, 4
    #          group 0        group 1        group 2: 10's parent lies outside its group, 11's parent does not keep its row
    parent = [0, 0, 2, 2,    4, 4, 4, 7,    9, 9, 3, 10]
    lens = [5, 0, 9, 1,      max_len + 3, 2, 2, -4,    0, 6, 3, 3]
    R = len(parent)
    init = torch.full((R, max_len), 0, dtype=i32)
    for r in range(R):   # row r holds 1000·r + position below its length and a sentinel of its own past it
        n = _rules.clamp(lens[r], 0, max_len)
        init[r, :n] = torch.arange(n, dtype=i32) + 1000 * r
        init[r, n:] = -(r + 1)
    hist = Guard(R, max_len, i32, gpu, init=init, ld=max_len + 8, fill=ISENT)
    lens_d = _i(lens, gpu)
    ops.hist_follow(hist.view, _i(parent, gpu), lens_d, W, max_len)
    want = init.clone()
    moved = []
    for r in range(R):
        p, g0 = parent[r], r - r % W
        if p == r or not g0 <= p < g0 + W or parent[p] != p:
            continue
        n = _rules.clamp(lens[p], 0, max_len)
        want[r, :n] = init[p, :n]
        moved.append(r)
    assert moved == [1, 3, 5, 6, 8]
    assert hist.intact() and torch.equal(hist.cpu(), want)
    assert lens_d.cpu().tolist() == lens   # the lengths are the gather's to write
    assert hist.cpu()[5].tolist() == init[4].tolist()          # the whole row at a length clamped to max_len
    assert hist.cpu()[1, 5:].tolist() == [-2] * (max_len - 5)  # nothing past the parent's length
