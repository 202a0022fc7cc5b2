"""The group scheduler of beam search in slot mode (ergm_amd.generate.BeamScheduler) on a fake backend, no GPU: FIFO
admission into the least recently admitted free group under max_admit / max_admit_tokens, retirement at the first look
at which the device says all W rows are finished, backtracking over exactly min(rounds, max_new) rounds, the
RuntimeError when the device flags and the round count disagree, and the round count on tools/gen_bench.py's seeded
request list against static batches that each run their largest bound."""
import importlib.util
import math
import os

import pytest

from ergm_amd import generate as G

EOS = 97
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeBeams:
    """A device of n_groups · W rows.  A live row's token in round i of its request is 1000·i + its row within the group
    (so a hypothesis names the rows it came through); row w continues row (w + i) % W of its group; a group finishes at
    its bound or at ``eos_at[id]`` rounds; a finished or idle row offers EOS and keeps its row, at unchanged scores.
    scores[row w] = -(w + 1) - rounds·W: the last row is the worst."""

    def __init__(self, n_groups, W, eos_at=None, stuck=()):
        self.G, self.W = n_groups, W
        self.req = [None] * n_groups      # (request, rounds run)
        self.eos_at = eos_at or {}
        self.stuck = set(stuck)           # ids whose rows never finish: a device that disagrees with the host
        self.scores = [-math.inf] * (n_groups * W)
        self.calls, self.retired, self.chunks = [], [], 0

    def admit_requests(self, groups, requests):
        self.calls.append(([r.id for r in requests], list(groups)))
        for g, r in zip(groups, requests):
            assert self.req[g] is None or self._done(g)
            self.req[g] = [r, 0]
            for w in range(self.W):
                self.scores[g * self.W + w] = 0.0 if w == 0 else -math.inf

    def _done(self, g):
        if self.req[g] is None:
            return True
        r, k = self.req[g]
        return r.id not in self.stuck and k >= min(r.max_new, self.eos_at.get(r.id, r.max_new))

    def run_beam_chunk(self, n):
        self.chunks += 1
        W, R = self.W, self.G * self.W
        tokens, parents = [], []
        for _ in range(n):
            trow, prow = [EOS] * R, list(range(R))
            for g in range(self.G):
                if self._done(g):
                    continue
                r, k = self.req[g]
                last = k + 1 == self.eos_at.get(r.id, -1)
                for w in range(W):
                    trow[g * W + w] = EOS if last else 1000 * k + w
                    prow[g * W + w] = g * W + (w + k) % W
                    self.scores[g * W + w] = -(w + 1) - (k + 1) * W
                self.req[g][1] += 1
            tokens.append(trow), parents.append(prow)
        fin = [1 if self._done(r // W) else 0 for r in range(R)]
        return tokens, parents, fin, list(self.scores)

    def retire(self, g, request):
        self.retired.append((request.id, g))


def _sched(n_groups, W, **kw):
    be = FakeBeams(n_groups, W, kw.pop("eos_at", None), kw.pop("stuck", ()))
    return be, G.BeamScheduler(be, n_groups, W, max_len=128, cap_max=8, **kw)


def _chain_ok(hyp, W):
    """The hypothesis' tokens name round i at place i and a row that continues the row before it."""
    rows = [t % 1000 for t in hyp]
    return [t // 1000 for t in hyp] == list(range(len(hyp))) and all(
        rows[i - 1] == (rows[i] + i) % W for i in range(1, len(hyp)))


def test_fifo_group_reuse_and_admission_limits():
    be, s = _sched(2, 3, max_admit=2, max_admit_tokens=20)
    new = [3, 20, 9, 2, 5]
    ids = [s.submit(n, 4, k) for n, k in zip([5, 12, 10, 9, 3], new)]
    out = s.run(EOS)
    assert ids == [0, 1, 2, 3, 4] and sorted(out) == ids
    # requests 0 and 1 at once (17 rows); request 2 takes group 0 at the next look (request 0 done; group 1 is busy with
    # request 1's 20 rounds); both groups end in the third chunk, and request 3 takes group 1, the less recently admitted
    assert be.calls[0] == ([0, 1], [0, 1])
    assert be.calls[1] == ([2], [0])
    assert be.calls[2] == ([3, 4], [1, 0]) and be.chunks == 4
    order = [i for call in be.calls for i in call[0]]
    assert order == ids                                   # nothing overtakes
    assert all(len(c[0]) <= 2 for c in be.calls)
    groups = {i: g for call in be.calls for i, g in zip(*call)}
    assert s.admissions == [list(zip(*c)) for c in be.calls]
    assert sorted(be.retired) == sorted(groups.items())
    for i, k in zip(ids, new):
        (hyp, score), = out[i]
        assert len(hyp) == k and EOS not in hyp and _chain_ok(hyp, 3), (i, hyp)
        assert score == -1 - k * 3                        # row 0 of the group: the best raw sum
    # max_admit_tokens: 12 + 10 rows do not fit one admission of 20
    be, s = _sched(4, 2, max_admit_tokens=20)
    for n in (12, 10, 3):
        s.submit(n, 4, 2)
    s.run(EOS)
    assert [c[0] for c in be.calls] == [[0], [1, 2]] and be.chunks == 1
    with pytest.raises(ValueError):
        s.submit(21, 4, 2)                                # can never be admitted
    with pytest.raises(ValueError):
        s.submit(5, 4, 2, keep=True)
    with pytest.raises(ValueError):
        s.extend(0, 3)
    with pytest.raises(ValueError):
        G.BeamScheduler(be, 4, 9, 128, 8)
    with pytest.raises(ValueError):
        list(s.drain(EOS, num_return=3))


def test_backtracking_cuts_at_the_bound_and_at_eos():
    """max_new 3, 8, 9 and 11: the chunk of 8 runs 5, 0, 7 and 5 rounds past the bound, and none of them reaches the
    hypothesis; a group whose beams all take eos in round 4 ends there with the eos included."""
    W = 4
    be, s = _sched(5, W, eos_at={4: 5})
    new = [3, 8, 9, 11, 30]
    for k in new:
        s.submit(6, 4, k)
    out = s.run(EOS, length_penalty=0.0, num_return=W)
    assert s.steps == 16
    for i, k in enumerate(new[:4]):
        assert len(out[i]) == W
        for rank, (hyp, score) in enumerate(out[i]):
            assert len(hyp) == k and EOS not in hyp and _chain_ok(hyp, W), (i, rank, hyp)
            assert hyp[-1] % 1000 == rank and score == -(rank + 1) - k * W   # penalty 0: ranked by the raw sum, by row
    for rank, (hyp, score) in enumerate(out[4]):
        assert len(hyp) == 5 and hyp[-1] == EOS and EOS not in hyp[:-1] and _chain_ok(hyp[:-1], W)
    # the length penalty acts on the final order only: with it the same hypotheses, best by score / len
    be, s = _sched(1, W)
    s.submit(6, 4, 3)
    (best, sc), = s.run(EOS, length_penalty=1.0)[0]
    assert best == out[0][0][0] and sc == out[0][0][1]


def test_device_flags_that_disagree_with_the_round_count_raise():
    be, s = _sched(2, 2, stuck={1})
    s.submit(5, 4, 3)
    s.submit(5, 4, 8)
    got = []
    with pytest.raises(RuntimeError, match="group 1"):
        for item in s.drain(EOS):
            got.append(item[0])
    assert got == [0]


def _gen_bench():
    spec = importlib.util.spec_from_file_location("gen_bench", os.path.join(ROOT, "tools", "gen_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n_groups,static_want,cont_want", [(8, 1460, 696), (4, 2257, 1368)])
def test_fewer_rounds_than_static_batches_on_the_seeded_list(n_groups, static_want, cont_want):
    """tools/gen_bench.py's 256 requests (4,519 requested tokens), W = 4: static batches of n_groups prompts in arrival
    order each run their largest bound; the scheduler refills a group at every 8-round look."""
    new = _gen_bench().request_lengths(256)
    assert len(new) == 256 and sum(new) == 4519
    static = sum(max(new[i:i + n_groups]) for i in range(0, 256, n_groups))
    be, s = _sched(n_groups, 4)
    for k in new:
        s.submit(64, 8, k)
    out = s.run(EOS)
    print(f"{n_groups} groups: static {static} rounds, continuous {s.steps} rounds, ratio {static / s.steps:.2f}")
    assert [len(out[i][0][0]) for i in range(256)] == new
    assert static == static_want and s.steps == cont_want
    assert s.steps < static
