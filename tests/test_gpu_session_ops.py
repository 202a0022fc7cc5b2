"""ergm_slots_save and ergm_slots_load (ergm_amd/csrc/session.hip) on the GPU against torch slicing, bitwise, with the
caches, the state and the blobs pre-filled with sentinels: every byte of a blob is what ergm_hip.h's layout says,
nothing outside it is written, the saved slot is idle, a load into another slot gives the source's rows and state
words and leaves every row at or past the row counts, the history at or past n and every other slot alone, and a
device meta that names a slot out of range or sizes above its blob writes nothing.  Row counts: the 64-row chunk edges
and a full cache of 192 rows; caption rows 1 and 16 = cap_max; 1 and 3 layers; rows of 256 B (fewer 16-byte pieces than
lanes) and of 3,072 B (three pieces per lane)."""
import pytest
import torch

from ergm_amd import _lib as L
from ergm_amd import ops

pytestmark = pytest.mark.gpu
MB, MAX_LEN, CAP_MAX, LD_SEEN, BAD_CAP = 4, 192, 16, 17, 7   # a seen row of 68 B and a pool row of 28 B: both padded
CTL, RULES = L.SESSION_CTL, L.SESSION_RULES
ROWS = (1, 2, 63, 64, 65, 128, 191, 192)
SENT, GUARD = 0x5A, 256
NAMES = ("lens", "cap_lens", "stop_lens", "finished", "row_ids", "row_steps", "ctl_vals", "min_step", "seen", "hist",
         "rule_vals", "bad")


class _Slots:
    """The buffers of a generator with controls and rules, random or sentinel-filled, and their ergm_session_state."""

    def __init__(self, gpu, n_layer, row_bytes, seed=None, ctl=True, rules=True):
        g = None if seed is None else torch.Generator().manual_seed(seed)

        def ints(*shape, dtype=torch.int32):
            if g is None:
                return torch.full(shape, SENT * 0x01010101 if dtype != torch.uint8 else SENT, dtype=dtype, device=gpu)
            hi = 2 if dtype == torch.uint8 else 2 ** 31 - 1
            return torch.randint(0, hi, shape, generator=g, dtype=dtype).to(gpu)

        def cache(rows):
            if g is None:
                return torch.full((MB, rows, row_bytes // 2), SENT * 0x0101, dtype=torch.int16, device=gpu)
            return torch.randint(-2 ** 15, 2 ** 15, (MB, rows, row_bytes // 2), generator=g, dtype=torch.int16).to(gpu)

        self.kv = [cache(MAX_LEN) for _ in range(n_layer)]
        self.xkv = [cache(CAP_MAX) for _ in range(n_layer)]
        self.lens, self.cap_lens, self.stop_lens = ints(MB), ints(MB), ints(MB)
        self.finished = ints(MB, dtype=torch.uint8)
        self.row_ids, self.row_steps = ints(MB), ints(MB)
        self.ctl_vals, self.min_step, self.seen = ints(4, MB), ints(MB), ints(MB, LD_SEEN)
        self.hist, self.rule_vals, self.bad = ints(MB, MAX_LEN), ints(2, MB), ints(MB, BAD_CAP)
        f = lambda i: self.ctl_vals[i].view(torch.float32)
        self.ctl = ops.sample_ctl(top_p=f(0), temperature=f(1), rep_penalty=f(2), top_k=self.ctl_vals[3],
                                  min_step=self.min_step, seen=self.seen) if ctl else None
        self.rules = ops.rules_desc(self.hist, start=self.rule_vals[0], ngram=self.rule_vals[1], bad=self.bad) if rules else None
        self.state = ops.SessionState(self.kv, self.xkv, self.lens, self.cap_lens, self.stop_lens, self.finished, self.row_ids,
                                      self.row_steps, ctl=self.ctl, rules=self.rules)
        self.n_layer, self.row_bytes = n_layer, row_bytes

    def snap(self):
        d = {k: getattr(self, k).cpu().clone() for k in NAMES}
        d["kv"], d["xkv"] = [t.cpu().clone() for t in self.kv], [t.cpu().clone() for t in self.xkv]
        return d


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def _pad16(t):
    b = _bytes(t)
    return torch.cat([b, torch.zeros(-b.numel() % 16, dtype=torch.uint8)])


def _blob_ref(s, slot, n, c, flags, n_layer, row_bytes):
    """The blob of ergm_hip.h's layout from a snapshot, on the CPU."""
    secs = [torch.cat([lay[slot, :rows].reshape(-1) for lay in caches]) for caches, rows in ((s["kv"], n), (s["xkv"], c))]
    body = [_bytes(x) for x in secs]
    if flags & CTL:
        body.append(_bytes(torch.cat([s["ctl_vals"][:, slot], s["min_step"][slot:slot + 1], torch.zeros(3, dtype=torch.int32)])))
        body.append(_pad16(s["seen"][slot]))
    if flags & RULES:
        body.append(_bytes(torch.cat([s["rule_vals"][:, slot], torch.zeros(2, dtype=torch.int32)])))
        body.append(_pad16(s["bad"][slot]))
        body.append(_pad16(s["hist"][slot, :n]))
    nbytes = 64 + sum(b.numel() for b in body)
    hdr = torch.tensor([L.SESSION_MAGIC, 1, flags, n_layer, row_bytes, n, c, int(s["row_ids"][slot]), int(s["row_steps"][slot]),
                        LD_SEEN if flags & CTL else 0, BAD_CAP if flags & RULES else 0, 0, nbytes, 0, 0, 0], dtype=torch.int32)
    return torch.cat([_bytes(hdr)] + body)


def _guarded(gpu, nbytes):
    buf = torch.full((nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=gpu)
    return buf, buf[GUARD:GUARD + nbytes]


def _check_saved(src, before, sessions, bufs):
    """After a save of ``sessions`` = [(slot, n, c, flags)]: the blobs byte for byte, the guards, the idle slots and
    everything else as it was."""
    after = src.snap()
    for (slot, n, c, flags), (buf, blob) in zip(sessions, bufs):
        want = _blob_ref(before, slot, n, c, flags, src.n_layer, src.row_bytes)
        assert want.numel() == blob.numel() == src.state.bytes(n, c, flags)
        assert torch.equal(blob.cpu(), want), (slot, n, c, flags)
        host = buf.cpu()
        assert bool((host[:GUARD] == SENT).all()) and bool((host[GUARD + blob.numel():] == SENT).all())
        before["finished"][slot], before["lens"][slot], before["cap_lens"][slot] = 1, 0, 0
        if flags & RULES:   # the next tenant inherits no rule
            before["rule_vals"][:, slot] = 0
            before["bad"][slot] = 0
    for k in NAMES:
        assert torch.equal(after[k], before[k]), k
    for k in ("kv", "xkv"):
        assert all(torch.equal(a, b) for a, b in zip(after[k], before[k])), k


def _check_loaded(dst, src_snap, pairs, ids=None):
    """After a load into the sentinel-filled ``dst`` of ``pairs`` = [(source slot, n, c, flags, destination slot)]: the
    destination's rows and state words are the source's, and everything else is the sentinel."""
    want = _Slots(dst.lens.device, dst.n_layer, dst.row_bytes).snap()
    for b, (s0, n, c, flags, s1) in enumerate(pairs):
        for k, rows in (("kv", n), ("xkv", c)):
            for w, s in zip(want[k], src_snap[k]):
                w[s1, :rows] = s[s0, :rows]
        want["lens"][s1], want["cap_lens"][s1], want["stop_lens"][s1], want["finished"][s1] = n, c, n, 1
        want["row_ids"][s1] = src_snap["row_ids"][s0] if ids is None else ids[b]
        want["row_steps"][s1] = src_snap["row_steps"][s0]
        if flags & CTL:
            want["ctl_vals"][:, s1], want["min_step"][s1] = src_snap["ctl_vals"][:, s0], src_snap["min_step"][s0]
            want["seen"][s1] = src_snap["seen"][s0]
        if flags & RULES:
            want["rule_vals"][:, s1], want["bad"][s1] = src_snap["rule_vals"][:, s0], src_snap["bad"][s0]
            want["hist"][s1, :n] = src_snap["hist"][s0, :n]
        else:   # a blob without rules turns the slot's off; the history is not touched
            want["rule_vals"][:, s1] = 0
            want["bad"][s1] = 0
    got = dst.snap()
    for k in NAMES:
        assert torch.equal(got[k], want[k]), k
    for k in ("kv", "xkv"):
        assert all(torch.equal(a, b) for a, b in zip(got[k], want[k])), k


@pytest.mark.parametrize("n_layer,row_bytes", [(1, 256), (3, 256), (1, 3072)])
def test_one_session_round_trip_at_every_chunk_edge(gpu, n_layer, row_bytes):
    assert L.load().ergm_session_launches(n_layer) == 3
    for i, n in enumerate(ROWS):
        c = (1, CAP_MAX)[i % 2]
        slot, dest = ((0, MB - 1), (MB - 1, 0), (0, 1), (MB - 1, 2))[i % 4]
        flags = CTL | (RULES if i % 3 else 0)
        src = _Slots(gpu, n_layer, row_bytes, seed=100 + i)
        before = src.snap()
        buf, blob = _guarded(gpu, src.state.bytes(n, c, flags))
        ops.slots_save(src.state, [slot], [n], [c], [flags], blobs=[blob])
        _check_saved(src, {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in before.items()},
                     [(slot, n, c, flags)], [(buf, blob)])
        dst = _Slots(gpu, n_layer, row_bytes)
        ops.slots_load(dst.state, [dest], [dst.state.header(n, c, flags)], [blob])
        _check_loaded(dst, before, [(slot, n, c, flags, dest)])
        assert torch.equal(blob.cpu(), _blob_ref(before, slot, n, c, flags, n_layer, row_bytes))   # a load writes no blob


@pytest.mark.parametrize("n_layer,row_bytes", [(3, 256), (1, 3072)])
def test_four_sessions_of_mixed_lengths_in_one_call(gpu, n_layer, row_bytes):
    sessions = [(3, 1, 1, CTL | RULES), (0, 64, CAP_MAX, CTL), (2, 65, CAP_MAX, CTL | RULES), (1, 192, 1, CTL)]
    src = _Slots(gpu, n_layer, row_bytes, seed=7)
    before = src.snap()
    bufs = [_guarded(gpu, src.state.bytes(n, c, f)) for _, n, c, f in sessions]
    cols = list(zip(*sessions))
    ops.slots_save(src.state, cols[0], cols[1], cols[2], cols[3], blobs=[b for _, b in bufs])
    _check_saved(src, {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in before.items()},
                 sessions, bufs)
    # back into other slots, the last two under ids of their own (what a fork does); all four at once
    dests = [0, 1, 3, 2]
    dst = _Slots(gpu, n_layer, row_bytes)
    hdrs = [dst.state.header(n, c, f) for _, n, c, f in sessions]
    ops.slots_load(dst.state, dests, hdrs, [b for _, b in bufs])
    _check_loaded(dst, before, [(s, n, c, f, d) for (s, n, c, f), d in zip(sessions, dests)])
    ids = [11, 12, -5, 2 ** 31 - 1]
    dst = _Slots(gpu, n_layer, row_bytes)
    ops.slots_load(dst.state, dests, hdrs, [b for _, b in bufs], row_ids=torch.tensor(ids, dtype=torch.int32, device=gpu))
    _check_loaded(dst, before, [(s, n, c, f, d) for (s, n, c, f), d in zip(sessions, dests)], ids=ids)
    # two of them only, one blob into two slots (a fork and its origin)
    dst = _Slots(gpu, n_layer, row_bytes)
    ops.slots_load(dst.state, [2, 0], [hdrs[2], hdrs[2]], [bufs[2][1], bufs[2][1]])
    s, n, c, f = sessions[2]
    _check_loaded(dst, before, [(s, n, c, f, 2), (s, n, c, f, 0)])


def test_states_without_controls_or_rules(gpu):
    """flags 0: the caches and the draw counters alone; and a state with controls and no rules."""
    for ctl in (False, True):
        flags = CTL if ctl else 0
        src = _Slots(gpu, 3, 256, seed=21, ctl=ctl, rules=False)
        before = src.snap()
        buf, blob = _guarded(gpu, src.state.bytes(65, 5, flags))
        assert blob.numel() == 64 + 3 * 65 * 256 + 3 * 5 * 256 + ((32 + 80) if ctl else 0)
        ops.slots_save(src.state, [1], [65], [5], [flags], blobs=[blob])
        _check_saved(src, {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in before.items()},
                     [(1, 65, 5, flags)], [(buf, blob)])
        dst = _Slots(gpu, 3, 256, ctl=ctl, rules=False)
        ops.slots_load(dst.state, [2], [dst.state.header(65, 5, flags)], [blob])
        got, want = dst.snap(), _Slots(gpu, 3, 256).snap()
        for k in ("rule_vals", "bad", "hist") + (() if ctl else ("ctl_vals", "min_step", "seen")):
            assert torch.equal(got[k], want[k]), k          # no such section: not touched
        assert torch.equal(got["kv"][2][2, :65], before["kv"][2][1, :65]) and bool((got["kv"][2][2, 65:] == SENT * 0x0101).all())
        assert int(got["lens"][2]) == 65 and int(got["row_ids"][2]) == int(before["row_ids"][1])
        if ctl:
            assert torch.equal(got["seen"][2], before["seen"][1]) and torch.equal(got["ctl_vals"][:, 2], before["ctl_vals"][:, 1])


def test_a_bad_device_meta_writes_nothing(gpu):
    """The host arguments are right and the device meta is not: a slot out of range (either side), a zero blob address,
    and row counts whose blob would be larger than the blob is.  Nothing is written, neither by a save nor by a load."""
    n, c, flags = 65, 5, CTL | RULES
    src = _Slots(gpu, 3, 256, seed=33)
    before = src.snap()
    nbytes = src.state.bytes(n, c, flags)
    good = ops.slots_save(src.state, [0], [n], [c], [flags])[0]
    src = _Slots(gpu, 3, 256, seed=33)
    for slot, rows, cap, addr in ((MB, n, c, None), (-1, n, c, None), (2 ** 40, n, c, None), (1, n, c, 0),
                                  (1, n + 1, c, None), (1, 10 ** 9, c, None), (1, n, CAP_MAX, None)):
        buf, blob = _guarded(gpu, nbytes)
        meta = torch.tensor([[slot], [rows], [cap], [blob.data_ptr() if addr is None else addr], [flags], [nbytes]],
                            dtype=torch.int64).to(gpu)
        ops.slots_save(src.state, [1], [n], [c], [flags], blobs=[blob], meta=meta)
        assert bool((buf.cpu() == SENT).all()), (slot, rows, cap, addr)
        got = src.snap()
        for k in NAMES:
            assert torch.equal(got[k], before[k]), (k, slot, rows, cap, addr)
        dst = _Slots(gpu, 3, 256)
        meta = torch.tensor([[slot], [rows], [cap], [good.data_ptr() if addr is None else addr], [flags], [nbytes]],
                            dtype=torch.int64).to(gpu)
        ops.slots_load(dst.state, [1], [dst.state.header(n, c, flags)], [good], meta=meta)
        got, want = dst.snap(), _Slots(gpu, 3, 256).snap()
        for k in NAMES:
            assert torch.equal(got[k], want[k]), (k, slot, rows, cap, addr)
        for k in ("kv", "xkv"):
            assert all(torch.equal(a, b) for a, b in zip(got[k], want[k])), (k, slot, rows, cap, addr)
    # smaller row counts in the meta than on the host are followed (the host's are the grid's bound): still inside
    buf, blob = _guarded(gpu, nbytes)
    meta = torch.tensor([[1], [3], [2], [blob.data_ptr()], [flags], [nbytes]], dtype=torch.int64).to(gpu)
    ops.slots_save(src.state, [1], [n], [c], [flags], blobs=[blob], meta=meta)
    small = src.state.bytes(3, 2, flags)
    assert torch.equal(blob[:small].cpu(), _blob_ref(before, 1, 3, 2, flags, 3, 256))
    assert bool((blob[small:].cpu() == SENT).all()) and bool((buf[:GUARD].cpu() == SENT).all())
