"""The session store's policy (ergm_amd.generate.SlotScheduler(store=True)) against a fake device in the style of
tests/test_extend_sched.py's SessionDevice, with save / load / drop / fork: how many sessions are evicted and which, one
save and one load call per look in the order save, load, extend, admit, a stored continuation that waits for a slot and
is not overtaken, three times as many sessions as slots through four turns, the row counts through a round trip,
release / offload / fork with their refusals, the byte cap, and store=False exactly as before."""
from types import SimpleNamespace

import pytest

import test_continuous_sched as CS
import test_extend_sched as XS
from ergm_amd.generate import SlotScheduler

EOS = CS.EOS


class StoreDevice(XS.SessionDevice):
    """SessionDevice whose parked slots can be packed away: a stored session is (rows, turn) under its id; the device
    checks that what is saved is a finished request of that id in that slot and that a load goes into a slot nobody
    runs in.  ``at_chunk``: {chunk number: callable}, requests that arrive while the device runs."""

    def __init__(self, max_batch, eos_at=None, at_chunk=None):
        super().__init__(max_batch, eos_at)
        self.store = {}
        self.save_calls, self.load_calls, self.dropped, self.forks = [], [], [], []
        self.at_chunk = at_chunk or {}

    def save_sessions(self, slots, ids):
        assert len(slots) == len(ids) == len(set(slots)) == len(set(ids))
        for s, i in zip(slots, ids):
            st = self.slots[s]
            assert st is not None and st[2] and st[0].id == i, f"slot {s} does not hold a finished request {i}"
            assert i not in self.store
            self.store[i] = self.rows[s]
            self.slots[s], self.rows[s] = None, 0
        self.save_calls.append((list(slots), list(ids)))
        self.order.append("save")

    def load_sessions(self, slots, ids):
        assert len(slots) == len(ids) == len(set(slots)) == len(set(ids))
        for s, i in zip(slots, ids):
            assert self.slots[s] is None or self.slots[s][2], f"slot {s} is still live"
            self.slots[s] = [SimpleNamespace(id=i), 0, True]
            self.rows[s] = self.store[i]
        self.load_calls.append((list(slots), list(ids)))
        self.order.append("load")

    def drop_session(self, i):
        del self.store[i]
        self.dropped.append(i)

    def fork_session(self, i, new):
        assert new not in self.store
        self.store[new] = self.store[i]
        self.turn[new] = self.turn[i]
        self.forks.append((i, new))

    def session_bytes(self, slot, rows, c):
        return 10 * rows

    def run_chunk(self, n):
        out = super().run_chunk(n)
        hook = self.at_chunk.pop(self.chunks, None)
        if hook is not None:
            hook()
        return out


def _sched(max_batch, eos_at=None, at_chunk=None, store=True, **kw):
    dev = StoreDevice(max_batch, eos_at, at_chunk)
    return dev, SlotScheduler(dev, max_batch, max_len=64, cap_max=8, store=store, **kw)


def _parked_in_turn(sch, new=(2, 10, 18, 26)):
    """One kept session per slot, parked at looks 1, 2, 3, ...: the bounds end them 8 steps apart."""
    ids = [sch.submit(4, 3, k, keep=True) for k in new]
    sch.run(EOS)
    assert sorted(sch.parked) == ids
    return ids


def test_eviction_count_and_least_recently_parked_first():
    dev, sch = _sched(4)
    a, b, c, d = _parked_in_turn(sch)
    x, y = sch.submit(4, 3, 2), sch.submit(4, 3, 2)
    out = sch.run(EOS)
    # two requests wait, no slot is free: exactly the two that were parked longest ago leave, in one call
    assert dev.save_calls == [([0, 1], [a, b])] and sch.saves == [[(a, 0), (b, 1)]]
    assert sorted(out) == [x, y] and sch.admissions[-1] == [(x, 0), (y, 1)]
    assert sch.stored == {a: (6, 3), b: (14, 3)} and sorted(sch.parked) == [c, d] and not dev.load_calls
    assert sch.stored_bytes == 10 * (6 + 14)
    # one waits and two slots are free: nothing is evicted
    z = sch.submit(4, 3, 2)
    assert sch.run(EOS) == {z: [1000 * z, 1000 * z + 1]} and len(dev.save_calls) == 1
    # ties (parked at the same look) go by slot
    dev, sch = _sched(4)
    ids = _parked_in_turn(sch, new=(3, 3, 2, 2))
    sch.submit(4, 3, 2)
    sch.run(EOS)
    assert dev.save_calls == [([0], [ids[0]])]
    # least recently parked, not lowest slot: slot 0's session is continued and parks again last
    dev, sch = _sched(3)
    a, b, c = _parked_in_turn(sch, new=(2, 2, 2))
    sch.extend(a, 2, 2)
    sch.run(EOS)
    sch.submit(4, 3, 2)
    sch.run(EOS)
    assert dev.save_calls == [([1], [b])]


def test_a_session_with_a_waiting_continuation_is_never_evicted():
    dev, sch = _sched(3)
    a, b, c = _parked_in_turn(sch, new=(2, 10, 18))
    sch.extend(a, 2, 2)                                       # a is the least recently parked, and about to continue
    x, y = sch.submit(4, 3, 2), sch.submit(4, 3, 2)
    out = sch.run(EOS)
    assert dev.save_calls[0] == ([1, 2], [b, c])              # a stays
    assert out[a] == [100, 101] and sorted(out) == sorted([a, x, y])
    assert dev.ext_calls[0] == ([0], [a], 2)


def test_one_save_and_one_load_per_look_in_the_order_save_load_extend_admit():
    dev, sch = _sched(3)
    a, b, c = _parked_in_turn(sch, new=(2, 10, 18))
    sch.offload(a)
    assert dev.save_calls == [([0], [a])] and a in sch.stored and a not in sch.parked
    d = sch.submit(4, 3, 2, keep=True)
    sch.run(EOS)
    assert sch.parked[d][0] == 0
    n = len(dev.order)
    sch.extend(a, 2, 2)                                       # stored: it needs a slot first
    sch.extend(c, 3, 2)                                       # parked: continued where it is
    e = sch.submit(4, 3, 2)
    out = sch.run(EOS)
    assert dev.order[n:] == ["save", "load", "extend", "admit"]
    assert dev.save_calls[-1] == ([1, 0], [b, d])             # want 2, free 0: both idle sessions, b parked first
    assert dev.load_calls == [([1], [a])]                     # slot 1 was admitted into longer ago than slot 0
    assert dev.ext_calls[-1] == ([2, 1], [c, a], 5) and sch.admissions[-1] == [(e, 0)]
    assert sch.saves[-1] == [(b, 1), (d, 0)] and sch.loads == [[(a, 1)]] and dev.dropped == [a]
    assert out[a] == [100, 101] and out[c] == [1000 * c + 100, 1000 * c + 101] and out[e] == [1000 * e, 1000 * e + 1]
    assert sorted(sch.stored) == [b, d] and sorted(sch.parked) == [a, c]


def test_a_stored_continuation_waits_for_a_slot_and_is_not_overtaken():
    holder = {}

    def arrive():   # while b runs in the only slot: a queued request first, then a's next turn
        holder["d"] = holder["sch"].submit(4, 3, 2)
        holder["sch"].extend(holder["a"], 2, 2)

    dev, sch = _sched(1, at_chunk={2: arrive})
    holder["sch"] = sch
    a = holder["a"] = sch.submit(4, 3, 2, keep=True)
    sch.run(EOS)
    sch.offload(a)
    b = sch.submit(4, 3, 20)
    order = [rid for rid, _ in sch.drain(EOS)]
    d = holder["d"]
    assert order == [b, a, d]                                 # a's turn goes before d, which arrived before it
    # b ran for three chunks; a's load had to wait for the look at which the slot was free
    assert dev.order == ["admit", "save", "admit", "load", "extend", "save", "admit"]
    assert sch.loads == [[(a, 0)]] and sch.saves[-1] == [(a, 0)] and a in sch.stored
    assert dev.chunks == 1 + 3 + 1 + 1


@pytest.mark.parametrize("eos_at", [None, {(i, t): 3 for i in range(0, 12, 2) for t in (0, 2)}])
def test_three_times_as_many_sessions_as_slots_through_four_turns(eos_at):
    """12 sessions on 4 slots, 4 turns each; with ``eos_at`` half of them end turns 0 and 2 by eos.  The device checks
    at every extension that the rows the scheduler states are the rows the session holds."""
    dev, sch = _sched(4, eos_at=eos_at)
    ids = [sch.submit(4, 3, 5, keep=True) for _ in range(12)]
    for turn in range(4):
        if turn:
            for i in ids:
                sch.extend(i, 2, 5)
        out = sch.run(EOS)
        assert sorted(out) == ids
        for i in ids:
            if eos_at and (i, turn) in eos_at:
                assert out[i] == [1000 * i + 100 * turn + j for j in range(3)] + [EOS], (i, turn)
            else:
                assert out[i] == [1000 * i + 100 * turn + j for j in range(5)], (i, turn)
        assert len(sch.parked) + len(sch.stored) == 12 and len(sch.parked) <= 4
    assert dev.save_calls and dev.load_calls and len(sch.saves) == len(dev.save_calls)
    rows = {i: 4 + sum(2 * (t > 0) + (3 if eos_at and (i, t) in eos_at else 5) for t in range(4)) for i in ids}
    got = {**{i: r for i, (r, _) in sch.stored.items()}, **{i: r for i, (_, r, _) in sch.parked.items()}}
    assert got == rows
    for i in ids:
        sch.release(i)
    assert not sch.stored and not sch.parked and not sch._held and not sch._active and sch.stored_bytes == 0 and not dev.store


def test_rows_survive_a_round_trip_for_eos_and_bound_endings():
    dev, sch = _sched(2, eos_at={(0, 0): 3, (1, 1): 0})
    a = sch.submit(4, 3, 10, keep=True)      # draws eos as its 4th token: 4 + 4 - 1 rows
    b = sch.submit(6, 2, 5, keep=True)       # runs to its bound: 6 + 5 rows
    sch.run(EOS)
    sch.offload(a)
    sch.offload(b)
    assert sch.stored == {a: (7, 3), b: (11, 2)} and dev.store == {a: 7, b: 11} and not sch.parked and not sch._held
    sch.extend(b, 5, 9)
    sch.extend(a, 3, 2)
    out = sch.run(EOS)                       # the device checks past == its rows at the extension
    assert out == {a: [100, 101], b: [EOS]}
    assert dev.load_calls == [([0, 1], [b, a])]                # arrival order of the continuations
    assert sch.parked == {a: (1, 7 + 3 + 2, 3), b: (0, 11 + 5 + 0, 2)}
    with pytest.raises(ValueError):
        sch.extend(a, 64 - 12, 1)            # the same room check as for a parked id
    sch.offload(a)
    with pytest.raises(ValueError):
        sch.extend(a, 64 - 12, 1)
    with pytest.raises(ValueError):
        sch.extend(a, 2, 64 - 12 - 2 + 1)
    assert sch.extend(a, 64 - 12 - 1) == a   # exactly one new token fits


def test_release_offload_and_fork():
    dev, sch = _sched(2)
    a = sch.submit(4, 3, 2, keep=True)
    q = sch.submit(4, 3, 30)
    for op in (sch.offload, sch.fork, sch.release):
        with pytest.raises(ValueError):
            op(a)                            # queued: neither parked nor stored
    it = sch.drain(EOS)
    assert next(it) == (a, [0, 1])           # a is parked while q still runs
    with pytest.raises(ValueError):
        sch.offload(q)                       # live
    sch.offload(a)
    sch.offload(a)                           # stored already: left as it is
    assert dev.save_calls == [([0], [a])] and sch.stored_bytes == 60
    f = sch.fork(a)                          # a stored id: no second save, one shared copy
    assert f == 2 and dev.forks == [(a, f)] and sch.stored[f] == sch.stored[a] == (6, 3) and sch.stored_bytes == 60
    with pytest.raises(ValueError):
        sch.fork(a, new_id=q)                # an id in use
    with pytest.raises(ValueError):
        sch.fork(a, new_id=f)
    with pytest.raises(ValueError):
        sch.fork(77)
    with pytest.raises(ValueError):
        sch.submit(4, 3, 2, request_id=f)    # a stored id is in use
    sch.extend(a, 2, 2)
    for op in (sch.offload, sch.fork, sch.release):
        with pytest.raises(ValueError):
            op(a)                            # its continuation waits
    sch.extend(f, 2, 2)
    out = dict(it)
    assert out[a] == [100, 101] and out[f] == [1000 * f + 100, 1000 * f + 101] and len(out[q]) == 30
    # both were loaded (their stored copy dropped); a parked again and had to leave for f, which is parked now
    assert dev.dropped == [a, f] and sch.stored_bytes == 100 and sorted(sch.stored) == [a] and sorted(sch.parked) == [f]
    # fork of a parked id offloads it first
    g = sch.fork(f, new_id=9)
    assert g == 9 and dev.save_calls[-1][1] == [f] and sorted(sch.stored) == [a, f, g] and sch.stored_bytes == 200
    assert not sch.parked and not sch._held
    sch.release(f)
    assert sch.stored_bytes == 200 and dev.dropped[-1] == f and g in dev.store      # the shared copy lives on
    sch.release(g)
    assert sch.stored_bytes == 100 and g not in sch._active and f not in sch._active and sorted(dev.store) == [a]
    with pytest.raises(ValueError):
        sch.release(g)
    sch.release(a)
    assert sch.stored_bytes == 0 and not sch._active and not dev.store


def test_the_byte_cap_restores_the_deadlock_error():
    dev, sch = _sched(2, store_bytes=100)
    a, b = sch.submit(4, 3, 2, keep=True), sch.submit(4, 3, 9, keep=True)    # 6 and 13 rows: 60 and 130 bytes
    sch.run(EOS)
    with pytest.raises(ValueError, match="store_bytes 100"):
        sch.offload(b)
    c, e = sch.submit(4, 3, 2), sch.submit(4, 3, 2, keep=True)
    assert sch.run(EOS).keys() == {c, e}
    # two waited, a fitted and left, b (130 bytes) was passed over: c and e took a's slot in turn, and e is parked there
    assert dev.save_calls == [([0], [a])] and sch.stored_bytes == 60 and sch.parked.keys() == {b, e}
    d = sch.submit(4, 3, 2)
    chunks = dev.chunks
    with pytest.raises(RuntimeError, match="every slot is parked: release a session \\(store_bytes 100 "):
        sch.run(EOS)                                                         # 60 + 60 and 60 + 130 are above the cap
    assert dev.chunks == chunks and len(dev.save_calls) == 1
    sch.release(a)
    assert sch.run(EOS).keys() == {d} and dev.save_calls[-1] == ([0], [e]) and sch.stored_bytes == 60
    for bad in (-1, True, 1.5):
        with pytest.raises(ValueError):
            SlotScheduler(dev, 2, 64, 8, store=True, store_bytes=bad)
    with pytest.raises(ValueError):
        SlotScheduler(dev, 2, 64, 8, store_bytes=100)                        # a cap without a store
    # without a cap the same load runs through
    dev, sch = _sched(2)
    ids = [sch.submit(4, 3, 2, keep=True) for _ in range(6)]
    assert sorted(sch.run(EOS)) == ids and len(sch.stored) == 4


def test_store_false_reproduces_the_deadlock_and_calls_nothing_new():
    """tests/test_extend_sched.py's deadlock on the store device with store=False, and the default is store=False."""
    for kw in ({"store": False}, {}):
        dev = StoreDevice(2)
        sch = SlotScheduler(dev, 2, max_len=64, cap_max=8, **kw)
        a, b = sch.submit(4, 3, 2, keep=True), sch.submit(4, 3, 9, keep=True)
        assert sch.run(EOS).keys() == {a, b}
        chunks = dev.chunks
        c = sch.submit(4, 3, 2)
        with pytest.raises(RuntimeError) as err:
            sch.run(EOS)
        assert str(err.value) == "1 request(s) wait and every slot is parked: release a session"
        assert dev.chunks == chunks and not dev.save_calls and not dev.load_calls and "save" not in dev.order
        for op in (sch.offload, sch.fork):
            with pytest.raises(ValueError, match="store=True"):
                op(a)
        with pytest.raises(ValueError) as err:
            sch.extend(77, 2)
        assert str(err.value) == "request id 77 is not parked"
        sch.release(b)
        assert sch.run(EOS) == {c: [2000, 2001]} and dev.calls[-1] == ([1], [c], 4)
        assert not sch.stored and not sch.saves and not sch.loads and sch.stored_bytes == 0
