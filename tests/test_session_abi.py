"""The session store's C ABI without a GPU: the new entry points (ergm_session_bytes, ergm_session_header,
ergm_session_launches, ergm_slots_save, ergm_slots_load) are declared, bound and exported with the ABI still 14;
ergm_session_bytes against a hand count of the layout in ergm_hip.h; and every refusal of a save and a load comes back
as ERGM_EINVAL with a telling message on fake pointers, before anything launches.  Helpers are
tests/test_continuous_abi.py's."""
import ctypes as C
import re

import test_continuous_abi as CA
from ergm_amd import _lib as L

NEW = ["ergm_session_bytes", "ergm_session_header", "ergm_session_launches", "ergm_slots_save", "ergm_slots_load"]
CTL, RULES = L.SESSION_CTL, L.SESSION_RULES
MB, MAX_LEN, CAP_MAX, NL, RB, LD_SEEN, BAD_CAP = 4, 32, 16, 2, 256, 16, 8


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(CA.HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14
    assert int(re.search(r"#define ERGM_ABI_VERSION (\d+)", src).group(1)) == 14
    for name, val in (("CTL", CTL), ("RULES", RULES), ("META_ROWS", L.SESSION_META_ROWS)):
        assert int(re.search(r"#define ERGM_SESSION_%s (\d+)" % name, src).group(1)) == val
    assert int(re.search(r"#define ERGM_SESSION_MAGIC (0x[0-9A-Fa-f]+)u", src).group(1), 16) == L.SESSION_MAGIC
    assert L.SESSION_MAGIC.to_bytes(4, "little") == b"ERGS"
    assert C.sizeof(L.SessionHdr) == 64 and L.SessionHdr.bytes.offset == 48
    assert lib.ergm_session_launches(1) == lib.ergm_session_launches(12) == lib.ergm_session_launches(48) == 3
    assert lib.ergm_session_launches(49) == 5 and lib.ergm_session_launches(0) == L.ERGM_EINVAL


def _up16(x):
    return (x + 15) // 16 * 16


def _hand(n_layer, row_bytes, rows, cap, ld_seen, bad_cap, flags):
    """ergm_hip.h's layout, counted by hand: the header, the two cache sections, 8 control words + the seen row, 4 rule
    words + the pool row + the history; every section padded to 16 bytes."""
    n = 64 + n_layer * rows * row_bytes + n_layer * cap * row_bytes
    if flags & CTL:
        n += 32 + _up16(4 * ld_seen)
    if flags & RULES:
        n += 16 + _up16(4 * bad_cap) + _up16(4 * rows)
    return n


def test_session_bytes_against_a_hand_count():
    size = L.load().ergm_session_bytes
    # GPT-2 small: 128 rows of 2 · 768 bf16 in 12 layers are 12 · 128 · 3,072 B = 4.7 MB of self-attention K | V
    assert 12 * 128 * 3072 == 4718592
    assert size(12, 3072, 128, 64, 0, 0, 0) == 64 + 4718592 + 12 * 64 * 3072 == 7077952
    seen = (50257 + 31) // 32   # 1,571 words: 6,284 bytes, padded to 6,288
    assert size(12, 3072, 128, 64, seen, 64, CTL) == 7077952 + 32 + 6288
    assert size(12, 3072, 128, 64, seen, 64, CTL | RULES) == 7077952 + 32 + 6288 + 16 + 256 + 512
    assert size(12, 3072, 128, 64, seen, 64, RULES) == 7077952 + 16 + 256 + 512
    # flags off: ld_seen and bad_cap do not count
    assert size(12, 3072, 128, 64, seen, 64, 0) == size(12, 3072, 128, 64, 0, 0, 0)
    # 16-byte rounding of hist at 1 and 5 rows (4 and 20 bytes), of a 5-word seen row and a 3-word pool row
    base = lambda rows: 64 + 2 * rows * 256 + 2 * 3 * 256
    assert size(2, 256, 1, 3, 4, 4, RULES) == base(1) + 16 + 16 + 16
    assert size(2, 256, 5, 3, 4, 4, RULES) == base(5) + 16 + 16 + 32
    assert size(2, 256, 4, 3, 4, 4, RULES) == base(4) + 16 + 16 + 16
    assert size(2, 256, 5, 3, 5, 3, CTL | RULES) == base(5) + 32 + 32 + 16 + 16 + 32
    for args in ((1, 16, 1, 1, 1, 1, 3), (3, 256, 63, 16, 16, 64, 3), (3, 256, 192, 1, 17, 7, 1), (1, 3072, 65, 16, 1, 1, 2)):
        got = size(*args)
        assert got == _hand(*args) and got % 16 == 0, args
    # rejected: 0
    for args in ((0, 256, 1, 1, 0, 0, 0), (1, 0, 1, 1, 0, 0, 0), (1, 24, 1, 1, 0, 0, 0), (1, 256, 0, 1, 0, 0, 0),
                 (1, 256, 1, 0, 0, 0, 0), (1, 256, 1, 1, 0, 0, 4), (1, 256, 1, 1, 0, 8, CTL), (1, 256, 1, 1, 8, 0, RULES),
                 (1, 256, 1, 1, 0, 0, -1), (1, -256, 1, 1, 0, 0, 0)):
        assert size(*args) == 0, args
    h = L.SessionHdr()
    assert L.load().ergm_session_header(2, 256, 5, 3, 5, 3, CTL, C.byref(h)) == L.ERGM_OK
    assert (h.magic, h.version, h.flags, h.n_layer, h.row_bytes, h.rows, h.cap_rows) == (L.SESSION_MAGIC, 1, CTL, 2, 256, 5, 3)
    assert (h.ld_seen, h.bad_cap, h.bytes, h.row_id, h.row_steps) == (5, 0, size(2, 256, 5, 3, 5, 3, CTL), 0, 0)
    assert L.load().ergm_session_header(2, 24, 5, 3, 5, 3, CTL, C.byref(h)) == L.ERGM_EINVAL


class _State:
    """An ergm_session_state over fake pointers, with the pieces kept alive."""

    def __init__(self, ctl=True, rules=True, **kw):
        self.keep, self.p = CA._buf()
        p = self.p
        self.ptrs = (C.c_void_p * NL)(*[p.value] * NL)
        self.ctl = L.SampleCtl(p, p, p, p, p, p, LD_SEEN)
        self.rules = L.LogitRules(p, MAX_LEN, p, p, p, BAD_CAP)
        f = dict(kv=self.ptrs, xkv=self.ptrs, n_layer=NL, row_bytes=RB, kv_ld_seq=MAX_LEN * RB, kv_ld_row=RB,
                 xkv_ld_seq=CAP_MAX * RB, xkv_ld_row=RB, max_batch=MB, max_len=MAX_LEN, cap_max=CAP_MAX, lens=p, cap_lens=p,
                 stop_lens=p, finished=p, row_ids=p, row_steps=p, ctl=C.pointer(self.ctl) if ctl else None,
                 rules=C.pointer(self.rules) if rules else None)
        f.update(kw)
        self.c = L.SessionState(**f)
        self.flags = (CTL if ctl else 0) | (RULES if rules else 0)


def _save(st, slots, rows, caps, flags=None, blobs=None, sizes=None, meta="p"):
    n = len(slots)
    p = st.p
    flags = [st.flags] * n if flags is None else flags
    blobs = [p.value + 64 * b for b in range(n)] if blobs is None else blobs
    sizes = [1 << 30] * n if sizes is None else sizes
    return L.load().ergm_slots_save(C.byref(st.c), n, CA._arr(*slots), CA._arr(*rows), CA._arr(*caps),
                                    CA._arr(*flags), (C.c_void_p * n)(*blobs), (C.c_size_t * n)(*sizes),
                                    p if meta == "p" else meta, None)


def _hdr(rows=5, cap=3, flags=CTL | RULES, n_layer=NL, row_bytes=RB, ld_seen=LD_SEEN, bad_cap=BAD_CAP):
    h = L.SessionHdr()
    assert L.load().ergm_session_header(n_layer, row_bytes, rows, cap, ld_seen, bad_cap, flags, C.byref(h)) == L.ERGM_OK
    return h


def _load(st, slots, hdrs, blobs=None, sizes=None, meta="p", row_ids=None):
    n = len(slots)
    p = st.p
    blobs = [p.value] * n if blobs is None else blobs
    sizes = [1 << 30] * n if sizes is None else sizes
    return L.load().ergm_slots_load(C.byref(st.c), n, CA._arr(*slots), (L.SessionHdr * n)(*hdrs), (C.c_void_p * n)(*blobs),
                                    (C.c_size_t * n)(*sizes), row_ids, p if meta == "p" else meta, None)


def _refused(word, rc):
    assert rc == L.ERGM_EINVAL
    assert word in L.last_error(), (word, L.last_error())


def test_save_refusals_without_a_gpu():
    st = _State()
    need = L.load().ergm_session_bytes(NL, RB, 5, 3, LD_SEEN, BAD_CAP, CTL | RULES)
    _refused("slot 4", _save(st, [4], [5], [3]))                                  # a slot out of range
    _refused("slot -1", _save(st, [-1], [5], [3]))
    _refused("named twice", _save(st, [2, 0, 2], [5] * 3, [3] * 3))
    _refused("n_seq", _save(st, [], [], []))                                      # n_seq outside [1, max_batch]
    _refused("n_seq", _save(st, [0, 1, 2, 3, 0], [5] * 5, [3] * 5))
    _refused("rows 0", _save(st, [0], [0], [3]))                                  # rows outside [1, max_len]
    _refused("rows 33", _save(st, [0], [MAX_LEN + 1], [3]))
    _refused("cap_rows 0", _save(st, [0], [5], [0]))                              # cap_rows outside [1, cap_max]
    _refused("cap_rows 17", _save(st, [0], [5], [CAP_MAX + 1]))
    _refused("needs", _save(st, [0], [5], [3], sizes=[need - 16]))                # a blob smaller than the session
    _refused("needs", _save(st, [0, 1], [5, 6], [3, 3], sizes=[need, need]))      # the second one needs more
    _refused("blob 0 null", _save(st, [0], [5], [3], blobs=[None]))
    _refused("aligned", _save(st, [0], [5], [3], blobs=[st.p.value + 8]))
    _refused("blob is named twice", _save(st, [0, 1], [5, 5], [3, 3], blobs=[st.p.value, st.p.value]))
    _refused("flags", _save(st, [0], [5], [3], flags=[4]))
    _refused("flags", _save(st, [0], [5], [3], flags=[RULES]))                    # the state has controls: they travel
    _refused("null", _save(st, [0], [5], [3], meta=None))
    _refused("null state", L.load().ergm_slots_save(None, 1, CA._arr(0), CA._arr(5), CA._arr(3), CA._arr(0),
                                                    (C.c_void_p * 1)(st.p.value), (C.c_size_t * 1)(1 << 30), st.p, None))
    # sections the state lacks
    _refused("flags", _save(_State(ctl=False, rules=False), [0], [5], [3], flags=[CTL]))
    _refused("flags", _save(_State(rules=False), [0], [5], [3], flags=[CTL | RULES]))
    # strides, row_bytes, pointers
    _refused("multiples of 16", _save(_State(row_bytes=RB + 8), [0], [5], [3]))
    _refused("multiples of 16", _save(_State(kv_ld_row=RB + 8), [0], [5], [3]))
    _refused("multiples of 16", _save(_State(xkv_ld_seq=CAP_MAX * RB + 8), [0], [5], [3]))
    _refused("shorter", _save(_State(kv_ld_seq=(MAX_LEN - 1) * RB), [0], [5], [3]))
    _refused("shorter", _save(_State(xkv_ld_row=RB - 16), [0], [5], [3]))
    _refused("null pointer", _save(_State(lens=None), [0], [5], [3]))
    _refused("null pointer", _save(_State(row_steps=None), [0], [5], [3]))
    _refused("null pointer", _save(_State(kv=None), [0], [5], [3]))
    bad = _State()
    bad.ptrs[1] = bad.p.value + 8
    _refused("layer 1", _save(bad, [0], [5], [3]))
    bad.ptrs[1] = None
    _refused("layer 1", _save(bad, [0], [5], [3]))
    bad = _State()
    bad.ctl.seen = None
    _refused("controls", _save(bad, [0], [5], [3]))
    bad = _State()
    bad.rules.ld_hist = MAX_LEN - 1
    _refused("ld_hist", _save(bad, [0], [5], [3]))
    bad = _State()
    bad.rules.bad = None
    _refused("rules", _save(bad, [0], [5], [3]))
    _refused("4-byte aligned", _save(_State(lens=C.c_void_p(st.p.value + 2)), [0], [5], [3]))


def test_load_refusals_without_a_gpu():
    st = _State()
    _refused("slot 4", _load(st, [4], [_hdr()]))
    _refused("named twice", _load(st, [1, 1], [_hdr(), _hdr()]))
    _refused("n_seq", _load(st, [0, 1, 2, 3, 0], [_hdr()] * 5))
    _refused("needs", _load(st, [0], [_hdr()], sizes=[_hdr().bytes - 16]))
    _refused("null", _load(st, [0], [_hdr()], blobs=[None]))
    _refused("aligned", _load(st, [0], [_hdr()], blobs=[st.p.value + 4]))
    _refused("null", _load(st, [0], [_hdr()], meta=None))
    # a header that disagrees with the state
    _refused("n_layer 3", _load(st, [0], [_hdr(n_layer=3)]))
    _refused("row_bytes 512", _load(st, [0], [_hdr(row_bytes=512)]))
    _refused("flags", _load(st, [0], [_hdr(flags=RULES)]))
    _refused("flags", _load(_State(rules=False), [0], [_hdr()]))
    _refused("flags", _load(_State(ctl=False, rules=False), [0], [_hdr(flags=CTL)]))
    _refused("ld_seen", _load(st, [0], [_hdr(ld_seen=LD_SEEN + 1)]))
    _refused("bad_cap", _load(st, [0], [_hdr(bad_cap=BAD_CAP + 4)]))
    _refused("rows 33", _load(st, [0], [_hdr(rows=MAX_LEN + 1)]))
    _refused("cap_rows 17", _load(st, [0], [_hdr(cap=CAP_MAX + 1)]))
    h = _hdr()
    h.magic = 0
    _refused("no session header", _load(st, [0], [h]))
    h = _hdr()
    h.version = 2
    _refused("no session header", _load(st, [0], [h]))
    h = _hdr()
    h.bytes += 16
    _refused("bytes", _load(st, [0], [h]))
    h = _hdr()
    h.rows = 0
    _refused("rows 0", _load(st, [0], [h]))
    _refused("multiples of 16", _load(_State(kv_ld_seq=MAX_LEN * RB + 4), [0], [_hdr()]))
    _refused("null pointer", _load(_State(finished=None), [0], [_hdr()]))
    # a blob without the rule section is accepted by the host checks of a state with rules only as far as its flags go:
    # the remaining checks of this call pass, so it is not sent (it would launch)
    assert _hdr(flags=CTL).bytes == L.load().ergm_session_bytes(NL, RB, 5, 3, LD_SEEN, BAD_CAP, CTL)
