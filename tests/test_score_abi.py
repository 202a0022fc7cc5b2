"""Scoring without a GPU: ergm_lm_score and ergm_decode_score are declared, bound and exported with the ABI still 14;
every bad argument of both comes back as ERGM_EINVAL on fake pointers, before anything launches; the workspace queries
are host-only, monotone and linear in the rows, far below a logits matrix; the dry launch count is the admission's
without its slot launches and with the scoring tail; and the host side of ContinuousGenerator.score (targets, groups,
trimming by ``first``) on a fake backend."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from ergm_amd import _lib as L
from ergm_amd import generate as G

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ergm_hip.h")
NEW = ["ergm_lm_score_workspace_size", "ergm_lm_score", "ergm_decode_score_workspace_size", "ergm_decode_score",
       "ergm_decode_score_launches"]
TINY = dict(vocab=500, vocab_pad=512, n_embd=128, n_layer=2, n_head=2, n_inner=512, n_positions=64, max_batch=4,
            max_len=32, cap_max=32, eps=1e-5)
PW = 512  # columns of a vocabulary partition (lmscore.hip LS_PW)


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14


def _buf(nbytes=1024, align=256):
    """A host buffer and an aligned address inside it (never dereferenced: no call below launches anything)."""
    raw = C.create_string_buffer(nbytes + align)
    return raw, C.c_void_p((C.addressof(raw) + align - 1) & ~(align - 1))


def _arr(*v):
    return (C.c_int * len(v))(*v)


# ---- ergm_lm_score ---------------------------------------------------------------------------------------------------
def test_lm_score_workspace_is_linear_in_the_rows_and_far_below_the_logits():
    ws = L.load().ergm_lm_score_workspace_size
    for V, K in ((500, 128), (50257, 768), (65536, 1024)):
        P = (V + PW - 1) // PW
        sizes = [ws(R, V, K) for R in (1, 2, 63, 64, 65, 512, 2048, 4096)]
        assert all(b > a for a, b in zip(sizes, sizes[1:]))
        for R in (1, 7, 64, 2048):
            assert ws(R, V, K) == (3 * P + 1) * R * 4       # O(R x partitions)
            assert ws(2 * R, V, K) <= 2 * ws(R, V, K) + 256
        assert ws(R, V, 64) == ws(R, V, K)                   # the partition does not depend on the depth
    assert ws(2048, 50257, 768) * 100 < 4 * 2048 * 50257     # 2.4 MB against the 412 MB of f32 logits
    for bad in ((0, 500, 128), (-1, 500, 128), (4, 0, 128), (4, 65537, 128), (4, 500, 0), (4, 500, 96), (4, 500, -64)):
        assert ws(*bad) == 0, bad


def test_lm_score_refusals_without_a_gpu():
    lib = L.load()
    keep, p = _buf()
    big = 1 << 30
    ok = dict(X=p, ldx=128, W=p, ldw=128, targets=p, R=8, V=500, K=128, ws=p, ws_bytes=big)

    def call(**kw):
        a = {**ok, **kw}
        return lib.ergm_lm_score(a["X"], a["ldx"], a["W"], a["ldw"], a["targets"], a["R"], a["V"], a["K"], p, p, p, p, a["ws"],
                                 a["ws_bytes"], None)

    def refused(word, **kw):
        assert call(**kw) == L.ERGM_EINVAL, kw
        assert word in L.last_error(), (word, L.last_error())

    refused("null", X=None)
    refused("null", W=None)
    refused("null", targets=None)
    refused("R 0", R=0)
    refused("R -3", R=-3)
    refused("V 0", V=0)
    refused("V 65537", V=65537)
    refused("K 0", K=0)
    refused("K 96", K=96, ldx=96, ldw=96)
    refused("ldx", ldx=120)
    refused("ldx", ldx=132)
    refused("ldw", ldw=64)
    refused("alignment", X=C.c_void_p(p.value + 8))
    refused("alignment", W=C.c_void_p(p.value + 2))
    refused("workspace", ws=None)
    refused("workspace", ws_bytes=lib.ergm_lm_score_workspace_size(8, 500, 128) - 1)
    refused("workspace", ws_bytes=lib.ergm_lm_score_workspace_size(7, 500, 128))
    refused("workspace", ws=C.c_void_p(p.value + 4))


# ---- ergm_decode_score -----------------------------------------------------------------------------------------------
def _score_ws(rows, cap_rows, **kw):
    return L.load().ergm_decode_score_workspace_size(C.byref(L.DecodeDims(**{**TINY, **kw})), rows, cap_rows)


def test_score_workspace_query_is_host_only_monotone_and_linear():
    rows = (2, 5, 31, 32, 33, 64, 100, 128, 256)
    sizes = [_score_ws(r, 32) for r in rows]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    c = _score_ws(1, 32)   # what does not scale with the token rows: the caption rows, the GEMM scratch, the alignment
    for r in (2, 16, 64, 128):
        assert _score_ws(2 * r, 32) <= 2 * _score_ws(r, 32) + c, r
    # at least the packed activations, and no logits: far below 4·R·V bytes once R is past the fixed part
    assert sizes[-1] > 256 * (128 * 4 + 128 * 2 * 3 + 3 * 128 * 2 + 2 * 512 * 2)
    big = dict(vocab=50257, vocab_pad=50304, n_embd=768, n_layer=12, n_head=12, n_inner=3072, n_positions=1024, max_batch=32,
               max_len=1024, cap_max=64)
    assert _score_ws(2048, 256, **big) * 4 < 4 * 2048 * 50257
    assert _score_ws(64, 64) >= _score_ws(64, 32) and _score_ws(64, 128) > _score_ws(64, 1)
    # rows beyond max_len are fine (scoring binds no cache) up to max_batch · n_positions
    assert _score_ws(4 * 64, 8) > 0
    for r, cap in ((0, 8), (8, 0), (-1, 8), (4 * 64 + 1, 8), (8, 4 * 32 + 1)):
        assert _score_ws(r, cap) == 0, (r, cap)
    assert _score_ws(8, 8, n_head=3) == 0
    assert _score_ws(8, 8, vocab=70000, vocab_pad=70016) == 0
    assert L.load().ergm_decode_score_workspace_size(None, 8, 8) == 0


def _plan(capkv=True, **kw):
    lib = L.load()
    dims = L.DecodeDims(**{**TINY, **kw})
    keep, p = _buf()
    prm = L.ModelParams()
    prm.wte = prm.wte_b = prm.wpe = prm.ln_f_w = prm.ln_f_b = prm.layer_f32 = prm.layer_b16 = p
    if capkv:
        prm.capkv_w_b = prm.capkv_b = p
    plan = C.c_void_p()
    rc = lib.ergm_decode_create(C.byref(dims), C.byref(prm), p, lib.ergm_decode_workspace_size(C.byref(dims)), C.byref(plan))
    assert rc == L.ERGM_OK
    return plan, keep, p


def test_score_refusals_without_a_gpu():
    lib = L.load()
    plan, keep, p = _plan()
    big = 1 << 30
    try:
        def score(lens, caps, ws_bytes=big, ids=p, meta=p, cap_ids=p, targets=p, ws=p, vis=None, aud=None, plan_=plan,
                  lens_=True, caps_=True):
            n = len(lens)
            return lib.ergm_decode_score(plan_, n, _arr(*lens) if lens_ else None, _arr(*caps) if caps_ else None, meta, ids,
                                         p, cap_ids, vis, aud, None, targets, p, p, ws, ws_bytes, None)

        def refused(word, *a, **kw):
            assert score(*a, **kw) == L.ERGM_EINVAL, (a, kw)
            assert word in L.last_error(), (word, L.last_error())

        # no bind is needed and none is looked at: the first refusals are about the arguments
        refused("< 2", [1], [7])                                    # n_b < 2: nothing to score
        refused("< 2", [5, 0], [7, 7])
        refused("n_positions", [65], [7])                           # n_b > n_positions
        refused("caption", [5], [0])                                # c_b < 1
        refused("cap_max", [5], [33])                               # c_b > cap_max
        refused("n_seq", [2] * 5, [1] * 5)                          # more sequences than max_batch
        refused("workspace", [16, 15], [7, 7], ws_bytes=_score_ws(30, 14) - 4096)   # 31 rows > what was sized
        refused("256-byte", [5], [7], ws=C.c_void_p(p.value + 16))
        for name in ("ids", "meta", "cap_ids", "targets", "ws"):
            refused("null", [5], [7], **{name: None})
        refused("null", [5], [7], lens_=False)
        refused("null", [5], [7], caps_=False)
        refused("null plan", [5], [7], plan_=None)
        refused("together", [5], [7], vis=p)
        assert lib.ergm_decode_score(plan, 0, _arr(5), _arr(7), p, p, p, p, None, None, None, p, p, p, p, big, None) == L.ERGM_EINVAL
        assert "n_seq" in L.last_error()
        # a sequence longer than max_len is fine: scoring has no cache to fill (the refusal is the workspace's)
        refused("workspace", [40], [7], ws_bytes=1024)
    finally:
        lib.ergm_decode_destroy(plan)
    plan, keep, p = _plan(capkv=False)
    try:
        assert lib.ergm_decode_score(plan, 1, _arr(5), _arr(7), p, p, p, p, None, None, None, p, p, p, p, big,
                                     None) == L.ERGM_EINVAL and "caption K/V" in L.last_error()
    finally:
        lib.ergm_decode_destroy(plan)


def _head_gemm_launches(n_seq):
    """Launches of the admission's head GEMM at n_seq rows: 2 when ergm_gemm splits K."""
    g = L.GemmDesc(M=n_seq, N=TINY["vocab_pad"], K=TINY["n_embd"], lda=TINY["n_embd"], ldb=TINY["n_embd"], ldc=TINY["vocab_pad"],
                   a_layout=L.MK, b_layout=L.NK, c_dtype=L.F32, epilogue=L.EPI_NONE, alpha=1.0)
    cfg, split, flags = C.c_int(), C.c_int(), C.c_int()
    assert L.load().ergm_gemm_plan(C.byref(g), C.byref(cfg), C.byref(split), C.byref(flags)) == L.ERGM_OK
    return 2 if split.value > 1 else 1


def test_score_launch_count_is_the_admissions_without_the_slots():
    """An admission's dry count, minus its slot launches (two row scatters per block, the gather of the last rows, the
    logits scatter and the slot-state kernel), minus its head GEMM, plus ergm_lm_score's two launches; ln_f is in
    both.  12 per block + 4 when no GEMM splits."""
    lib = L.load()
    plan, keep, p = _plan()
    nl = TINY["n_layer"]
    try:
        for n_seq, rows, cap_rows in ((1, 2, 1), (1, 30, 22), (3, 30, 22), (4, 64, 40), (2, 100, 64), (4, 128, 128)):
            admit = lib.ergm_decode_admit_launches(plan, n_seq, rows, cap_rows)
            score = lib.ergm_decode_score_launches(plan, n_seq, rows, cap_rows)
            assert score == admit - (2 * nl + 3) - _head_gemm_launches(n_seq) + 2, (n_seq, rows, cap_rows, admit, score)
            assert score >= 12 * nl + 4
        assert lib.ergm_decode_score_launches(plan, 1, 200, 22) > 0          # past max_batch · max_len: no cache involved
        assert lib.ergm_decode_score_launches(plan, 0, 30, 22) == L.ERGM_EINVAL
        assert lib.ergm_decode_score_launches(plan, 3, 5, 22) == L.ERGM_EINVAL   # fewer than two rows per sequence
        assert lib.ergm_decode_score_launches(plan, 3, 30, 2) == L.ERGM_EINVAL
        assert lib.ergm_decode_score_launches(None, 1, 30, 22) == L.ERGM_EINVAL
        # the admission's, the extension's and the step's counts are what they were
        assert lib.ergm_decode_admit_launches(plan, 1, 30, 22) >= 14 * nl + 6
        assert lib.ergm_decode_launches(plan, 0) - lib.ergm_decode_launches(plan, 1) == 3 * nl
    finally:
        lib.ergm_decode_destroy(plan)


# ---- the host side of ContinuousGenerator.score ------------------------------------------------------------------------
def test_targets_are_the_shifted_tokens_from_first_on():
    ids = [[10, 11, 12, 13], [20, 21], [30, 31, 32]]
    assert G.score_targets(ids, [1, 1, 1]) == [11, 12, 13, -100, 21, -100, 31, 32, -100]
    assert G.score_targets(ids, [3, 1, 2]) == [-100, -100, 13, -100, 21, -100, -100, 32, -100]
    assert G.score_targets([[7, 8]], [1]) == [8, -100]


def test_groups_follow_the_admission_rule():
    assert G.score_groups([5, 5, 5, 5, 5], 2, 100) == [(0, 2), (2, 4), (4, 5)]
    assert G.score_groups([30, 30, 30, 10, 60], 8, 64) == [(0, 2), (2, 4), (4, 5)]
    assert G.score_groups([64], 8, 64) == [(0, 1)]
    assert G.score_groups([], 8, 64) == []
    with pytest.raises(ValueError, match="fits no group"):
        G.score_groups([10, 65], 8, 64)


class _FakeGen(G.ContinuousGenerator):
    """ContinuousGenerator.score over a backend that records its groups and answers logprob = -(packed row index) / 8,
    top1 = target + 1: no GPU, no model."""

    def __init__(self, max_admit, max_admit_tokens, cap_max=8, n_positions=64):
        self.engine, self.dev = "native", torch.device("cpu")
        self.cfg = types.SimpleNamespace(n_positions=n_positions)
        self.m = types.SimpleNamespace(refresh_bf16=lambda: None)
        self.sched = types.SimpleNamespace(max_admit=max_admit, max_admit_tokens=max_admit_tokens)
        self.cap_max = cap_max
        self._plan = None
        self.calls = []

    def _score_native(self, grp, lens, clens, targets):
        self.calls.append((list(lens), list(clens), targets.tolist()))
        R = sum(lens)
        return -torch.arange(R, dtype=torch.float32) / 8, (targets + 1).int()


def _seq(n, c=3, base=0):
    return (torch.arange(base, base + n), torch.zeros(n, dtype=torch.int64), torch.arange(c), None, None)


def test_score_groups_trims_and_reads_back_once_per_group():
    g = _FakeGen(max_admit=2, max_admit_tokens=12)
    seqs = [_seq(4, base=100), _seq(6, base=200), _seq(7, base=300), _seq(2, base=400)]
    out = g.score(seqs, first=[1, 4, 2, 1])
    assert [c[0] for c in g.calls] == [[4, 6], [7, 2]]          # 4 + 6 + 7 > 12: the third opens a group
    assert g.calls[0][2] == [101, 102, 103, -100, -100, -100, -100, 204, 205, -100]
    assert g.calls[1][2] == [-100, 302, 303, 304, 305, 306, -100, 401, -100]
    assert [len(s.logprobs) for s in out] == [3, 2, 5, 1] == [len(s.top1) for s in out]
    assert out[0].logprobs == [0.0, -0.125, -0.25] and out[0].top1 == [102, 103, 104]
    assert out[1].logprobs == [-(4 + 3) / 8, -(4 + 4) / 8] and out[1].top1 == [205, 206]
    assert out[3].logprobs == [-7 / 8] and out[3].top1 == [402]
    assert out[1].sum == -(7 + 8) / 8 and abs(out[1].ppl - torch.tensor(15 / 16).exp().item()) < 1e-6
    # first trims the lists and changes no value
    full = _FakeGen(2, 12).score(seqs)
    assert full[1].logprobs[3:] == out[1].logprobs and full[2].logprobs[1:] == out[2].logprobs


def test_score_refuses_what_fits_no_group():
    g = _FakeGen(max_admit=2, max_admit_tokens=12)
    with pytest.raises(ValueError, match="fits no scoring group"):
        g.score([_seq(13)])
    with pytest.raises(ValueError, match="fits no scoring group"):
        g.score([_seq(1)])
    with pytest.raises(ValueError, match="fits no scoring group"):
        g.score([_seq(5, c=9)])
    with pytest.raises(ValueError, match="empty caption"):
        g.score([_seq(5, c=0)])
    for f in (0, 5, -1):
        with pytest.raises(ValueError, match="first"):
            g.score([_seq(5)], first=[f])
    with pytest.raises(ValueError, match="one first"):
        g.score([_seq(5)], first=[1, 1])
    assert g.calls == []
