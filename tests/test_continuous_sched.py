"""The continuous-batching policy (ergm_amd.generate.SlotScheduler) against a fake device: FIFO admission, slot reuse,
the per-call admission limits, rejection at submit, and every request's tokens cut at eos or at max_new_tokens."""
import pytest

from ergm_amd.generate import SlotScheduler

EOS = 97


class FakeDevice:
    """Emits, for the request in a slot, the tokens 1000·id + i (i = 0, 1, ...), or eos at position eos_at[id]; keeps
    the finished flag the way the device does (eos drawn, or the admission's bound reached) and emits eos afterwards."""

    def __init__(self, max_batch, eos_at=None):
        self.slots = [None] * max_batch      # [request, tokens drawn, finished]
        self.eos_at = eos_at or {}
        self.calls = []                      # (slots, ids, prompt rows) per admit call
        self.chunks = 0

    def admit_requests(self, slots, requests):
        assert len(slots) == len(requests) == len(set(slots))
        for s, r in zip(slots, requests):
            assert self.slots[s] is None or self.slots[s][2], f"slot {s} is still live"
            self.slots[s] = [r, 0, False]
        self.calls.append((list(slots), [r.id for r in requests], sum(r.n for r in requests)))

    def run_chunk(self, n):
        self.chunks += 1
        rows = []
        for _ in range(n):
            row = []
            for st in self.slots:
                if st is None or st[2]:
                    row.append(EOS)
                    continue
                r, i, _ = st
                tok = EOS if self.eos_at.get(r.id) == i else 1000 * r.id + i
                st[1] = i + 1
                st[2] = tok == EOS or st[1] == r.max_new
                row.append(tok)
            rows.append(row)
        return rows, [1 if st is None or st[2] else 0 for st in self.slots]


def _run(max_batch, new, eos_at=None, prompt=4, **kw):
    dev = FakeDevice(max_batch, eos_at)
    sch = SlotScheduler(dev, max_batch, max_len=64, cap_max=8, **kw)
    ids = [sch.submit(prompt, 3, k) for k in new]
    return dev, sch, ids, sch.run(EOS)


def test_seven_requests_on_two_slots_fifo_and_reuse():
    new = (1, 9, 3, 17, 2, 8, 5)
    dev, sch, ids, out = _run(2, new)
    assert ids == list(range(7))
    admitted = [i for _, call_ids, _ in dev.calls for i in call_ids]
    assert admitted == ids                                   # FIFO admission order
    for i, k in zip(ids, new):
        assert out[i] == [1000 * i + j for j in range(k)]    # stops at exactly max_new_tokens
    used = [s for slots, _, _ in dev.calls for s in slots]
    assert set(used) == {0, 1} and len(used) == 7            # both slots reused
    assert sch.steps == 8 * dev.chunks and not sch.queue and sch.live == [None, None]
    # the slots take turns: two free slots at once go to the one admitted into longer ago
    dev4, sch4, _, _ = _run(4, new, max_admit=1)
    by_req = {i: s for call in sch4.admissions for i, s in call}
    assert [by_req[i] for i in range(4)] == [0, 1, 2, 3]
    assert all(len(call) == 1 for call in sch4.admissions)
    assert by_req[6] == 1                                    # request 6 (5 tokens) takes the slot request 1 (9) left


def test_admission_limits():
    new = (3, 3, 3, 3, 3, 3)
    dev, _, _, out = _run(4, new, max_admit=2)
    assert all(len(ids) <= 2 for _, ids, _ in dev.calls) and [len(c[1]) for c in dev.calls[:2]] == [2, 2]
    assert sorted(out) == list(range(6))
    dev, _, _, _ = _run(4, new, max_admit_tokens=9, prompt=4)   # two prompts of 4 rows fit 9, three do not
    assert all(rows <= 9 for _, _, rows in dev.calls) and [len(c[1]) for c in dev.calls[:2]] == [2, 2]
    dev, _, _, _ = _run(4, new, max_admit_tokens=4)
    assert all(len(ids) == 1 for _, ids, _ in dev.calls)
    with pytest.raises(ValueError):
        SlotScheduler(FakeDevice(2), 2, 64, 8, max_admit=3)
    with pytest.raises(ValueError):
        SlotScheduler(FakeDevice(2), 2, 64, 8, max_admit=0)


def test_rejected_at_submit():
    sch = SlotScheduler(FakeDevice(2), 2, max_len=32, cap_max=8, max_admit_tokens=16)
    for n, c, k in ((32, 3, None), (40, 3, 1), (10, 3, 23), (10, 9, 4), (0, 3, 1), (10, 0, 1), (10, 3, 0), (17, 3, 1)):
        with pytest.raises(ValueError):
            sch.submit(n, c, k)
    assert not sch.queue
    assert sch.submit(10, 3) == 0 and sch.queue[0].max_new == 22        # the default: to the end of the cache
    assert sch.submit(10, 8, 22, request_id=2 ** 32 - 1) == 2 ** 32 - 1
    with pytest.raises(ValueError):
        sch.submit(10, 3, 1, request_id=2 ** 32)
    assert sch.submit(5, 1, 1) == 1                                      # explicit ids do not move the counter
    with pytest.raises(ValueError):
        sch.submit(5, 1, 1, request_id=0)                                # an id still queued


def test_tokens_cut_at_eos_or_bound():
    new = (1, 9, 3, 17, 2, 8, 5)
    eos_at = {1: 0, 3: 8, 5: 7, 6: 9}      # at the first token; on a chunk edge; at the last token; past the bound
    dev, sch, ids, out = _run(2, new, eos_at)
    assert out[1] == [EOS]
    assert out[3] == [3000 + j for j in range(8)] + [EOS]
    assert out[5] == [5000 + j for j in range(7)] + [EOS]
    assert out[6] == [6000 + j for j in range(5)]
    for i in (0, 2, 4):
        assert out[i] == [1000 * i + j for j in range(new[i])]
    # the generator form yields each request when it retires: request 1 (eos at once) leaves before request 0's
    # successor does, and nothing is yielded twice
    dev = FakeDevice(2, eos_at)
    sch = SlotScheduler(dev, 2, 64, 8)
    for k in new:
        sch.submit(4, 3, k)
    order = [i for i, _ in sch.drain(EOS)]
    assert sorted(order) == list(range(7)) and order[:2] == [0, 1]


def test_disagreement_with_the_device_flag_is_an_error():
    class Lying(FakeDevice):
        def run_chunk(self, n):
            rows, fin = super().run_chunk(n)
            return rows, [0] * len(fin)

    sch = SlotScheduler(Lying(2), 2, 64, 8)
    sch.submit(4, 3, 2)
    with pytest.raises(RuntimeError):
        sch.run(EOS)
