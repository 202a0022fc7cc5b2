"""Sessions in the continuous-batching policy (ergm_amd.generate.SlotScheduler) against a fake device in the style of
tests/test_continuous_sched.py's, with extend_requests: parked lengths for eos and bound endings, continuations before
admissions under the same per-call limits, drain with sessions parked, the all-parked deadlock, release, the refusals
of extend, and keep=False exactly as before."""
import pytest

import test_continuous_sched as CS
from ergm_amd.generate import SlotScheduler

EOS = CS.EOS


class SessionDevice(CS.FakeDevice):
    """FakeDevice that can continue a slot: a continuation emits 1000·id + 100·turn + i, and the device checks what the
    scheduler tells it about the slot (the request that parked there and the rows its cache holds)."""

    def __init__(self, max_batch, eos_at=None):
        super().__init__(max_batch, eos_at)
        self.rows = [0] * max_batch          # rows in each slot's cache, kept the way the device does
        self.turn = {}
        self.ext_calls = []                  # (slots, ids, new rows) per extend call
        self.order = []                      # "admit" / "extend", in call order

    def admit_requests(self, slots, requests):
        super().admit_requests(slots, requests)
        self.order.append("admit")
        for s, r in zip(slots, requests):
            self.rows[s] = r.n
            self.turn[r.id] = 0

    def extend_requests(self, slots, requests):
        assert len(slots) == len(requests) == len(set(slots))
        for s, r in zip(slots, requests):
            st = self.slots[s]
            assert st is not None and st[2] and st[0].id == r.id, f"slot {s} does not hold a finished request {r.id}"
            assert r.past == self.rows[s], f"slot {s}: the scheduler says {r.past} rows, the device holds {self.rows[s]}"
            assert r.slot == s and r.past + r.n + r.max_new <= 64
            self.rows[s] += r.n
            self.turn[r.id] += 1
            self.slots[s] = [r, 0, False]
        self.ext_calls.append((list(slots), [r.id for r in requests], sum(r.n for r in requests)))
        self.order.append("extend")

    def run_chunk(self, n):
        self.chunks += 1
        rows = []
        for _ in range(n):
            row = []
            for s, st in enumerate(self.slots):
                if st is None or st[2]:
                    row.append(EOS)
                    continue
                r, i, _ = st
                tok = EOS if self.eos_at.get((r.id, self.turn[r.id])) == i else 1000 * r.id + 100 * self.turn[r.id] + i
                st[1] = i + 1
                st[2] = tok == EOS or st[1] == r.max_new
                if tok != EOS:
                    self.rows[s] += 1        # an eos that was drawn is never stepped into the cache
                row.append(tok)
            rows.append(row)
        return rows, [1 if st is None or st[2] else 0 for st in self.slots]


def _sched(max_batch, eos_at=None, **kw):
    dev = SessionDevice(max_batch, eos_at)
    return dev, SlotScheduler(dev, max_batch, max_len=64, cap_max=8, **kw)


def test_parked_length_for_eos_and_bound_endings():
    dev, sch = _sched(2, eos_at={(0, 0): 3, (1, 1): 0})
    a = sch.submit(4, 3, 10, keep=True)      # draws eos as its 4th token
    b = sch.submit(6, 2, 5, keep=True)       # runs to its bound
    out = sch.run(EOS)
    assert out == {a: [0, 1, 2, EOS], b: [1000, 1001, 1002, 1003, 1004]}
    assert sch.parked == {a: (0, 4 + 4 - 1, 3), b: (1, 6 + 5, 2)}
    assert [sch.parked[i][1] for i in (a, b)] == [dev.rows[0], dev.rows[1]]
    # second turns: b draws eos at once, a runs to its bound; the lengths go on from the parked ones
    sch.extend(a, 3, 2)
    sch.extend(b, 5, 9)
    out = sch.run(EOS)
    assert out == {a: [100, 101], b: [EOS]}
    assert sch.parked == {a: (0, 7 + 3 + 2, 3), b: (1, 11 + 5 + 0, 2)}
    assert [sch.parked[i][1] for i in (a, b)] == [dev.rows[0], dev.rows[1]]
    assert dev.ext_calls == [([0, 1], [a, b], 8)] and sch.extensions == [[(a, 0), (b, 1)]]
    # a third turn that is not kept frees the slot
    sch.extend(a, 1, 1, keep=False)
    assert sch.run(EOS) == {a: [200]} and a not in sch.parked and sch.parked.keys() == {b}
    assert sch.submit(4, 3, 2, request_id=a) == a            # the id is free again


def test_continuations_go_first_and_respect_the_limits():
    dev, sch = _sched(4, max_admit=2, max_admit_tokens=10)
    ids = [sch.submit(4, 3, 2, keep=True) for _ in range(3)]
    sch.run(EOS)
    assert dev.calls == [([0, 1], [0, 1], 8), ([2], [2], 4)] and sorted(sch.parked) == ids
    n = len(dev.order)
    new = sch.submit(5, 3, 2)                                # arrives before the continuations are queued ...
    for i, k in zip(ids, (6, 5, 4)):
        sch.extend(i, k, 2)
    out = sch.run(EOS)
    assert dev.order[n:] == ["extend", "extend", "admit"]    # ... and is admitted after them
    assert dev.ext_calls == [([0], [0], 6), ([1, 2], [1, 2], 9)]   # 6 + 5 > 10 rows; then two sequences per call
    assert sch.admissions[-1] == [(new, 3)]
    assert sorted(out) == ids + [new] and out[0] == [100, 101] and out[new] == [3000, 3001]
    assert sch.parked[0] == (0, 4 + 2 + 6 + 2, 3)
    with pytest.raises(ValueError):
        sch.extend(1, 11, 2)                                 # more rows than one call takes
    with pytest.raises(ValueError):
        sch.extend(1, 0, 2)


def test_drain_returns_with_sessions_parked_and_the_deadlock_raises():
    dev, sch = _sched(2)
    a, b = sch.submit(4, 3, 2, keep=True), sch.submit(4, 3, 9, keep=True)
    assert sch.run(EOS).keys() == {a, b}                     # returned, although both slots stay held
    chunks = dev.chunks
    assert sch.run(EOS) == {} and dev.chunks == chunks       # nothing queued, nothing running: no step
    c = sch.submit(4, 3, 2)
    with pytest.raises(RuntimeError):
        sch.run(EOS)                                         # c waits, nothing runs, every slot is parked
    assert dev.chunks == chunks
    # a continuation running keeps the loop alive; c still cannot start, and the loop raises once it is alone again
    sch.extend(a, 2, 3)
    got = []
    with pytest.raises(RuntimeError):
        for rid, toks in sch.drain(EOS):
            got.append((rid, toks))
    assert got == [(a, [100, 101, 102])]
    sch.release(b)
    assert sch.run(EOS) == {c: [2000, 2001]} and dev.calls[-1] == ([1], [c], 4)   # the released slot


def test_release_and_the_refusals_of_extend():
    dev, sch = _sched(2)
    a = sch.submit(4, 3, 2, keep=True)
    with pytest.raises(ValueError):
        sch.extend(a, 2)                                     # queued, not parked
    with pytest.raises(ValueError):
        sch.release(a)
    sch.run(EOS)
    with pytest.raises(ValueError):
        sch.submit(4, 3, 2, request_id=a)                    # a parked id is still in use
    with pytest.raises(ValueError):
        sch.extend(a + 1, 2)                                 # unknown
    with pytest.raises(ValueError):
        sch.extend(a, 58)                                    # 6 + 58 rows: no room for one new token
    with pytest.raises(ValueError):
        sch.extend(a, 2, 57)                                 # 6 + 2 + 57 > 64
    assert sch.extend(a, 57) == a                            # 6 + 57 + 1 == 64: exactly one
    with pytest.raises(ValueError):
        sch.extend(a, 1)                                     # waiting for its look: not parked
    assert sch.run(EOS) == {a: [100]} and sch.parked[a] == (0, 64, 3)
    with pytest.raises(ValueError):
        sch.extend(a, 1)                                     # parked with its cache full
    sch.release(a)
    with pytest.raises(ValueError):
        sch.extend(a, 1)                                     # released
    with pytest.raises(ValueError):
        sch.release(a)
    assert not sch.parked and not sch._held and a not in sch._active
    # a one-token prompt that drew eos at once holds one row: nothing to continue
    dev, sch = _sched(1, eos_at={(0, 0): 0})
    a = sch.submit(1, 3, 5, keep=True)
    assert sch.run(EOS) == {a: [EOS]} and sch.parked[a] == (0, 1, 3)
    with pytest.raises(ValueError):
        sch.extend(a, 2)
    # a backend without extend_requests
    sch = SlotScheduler(CS.FakeDevice(1), 1, max_len=64, cap_max=8)
    a = sch.submit(4, 3, 2, keep=True)
    sch.run(EOS)
    with pytest.raises(ValueError):
        sch.extend(a, 2)


def test_keep_false_is_what_it_was():
    """tests/test_continuous_sched.py's seven requests on two slots through the session device: the same lists, the
    same admissions, nothing parked and no extension call."""
    new = (1, 9, 3, 17, 2, 8, 5)
    old_dev, old_sch, ids, want = CS._run(2, new)
    dev, sch = _sched(2)
    assert [sch.submit(4, 3, k) for k in new] == ids
    assert sch.run(EOS) == want
    assert dev.calls == old_dev.calls and sch.admissions == old_sch.admissions and sch.steps == old_sch.steps
    assert not sch.parked and not sch._held and not sch._active and dev.ext_calls == [] and sch.extensions == []
