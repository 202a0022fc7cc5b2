"""The logit rules without a GPU: ergm_logit_rules_apply, the history entry points and ergm_decode_set_rules are
declared, bound and exported with the ABI still 14; their argument checks refuse with ERGM_EINVAL on fake pointers
before anything launches; SamplingParams validates the new fields on the host and stays frozen and hashable; the
generator's check refuses rules without controls and lists beyond bad_words_cap, through SlotScheduler too; and the
plain-Python rule of tests/_rules.py agrees with a brute-force enumeration of all n-grams."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import _rules
from ergm_amd import _lib as L
from ergm_amd.generate import (ContinuousGenerator, SamplingParams, SlotScheduler, check_rules, pack_bad_words)

import test_continuous_abi as CA

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ergm_hip.h")
NEW = ["ergm_logit_rules_apply", "ergm_hist_write", "ergm_hist_append", "ergm_hist_follow", "ergm_decode_set_rules"]


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14
    body = re.search(r"typedef struct \{([^}]*)\} ergm_logit_rules;", src).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in L.LogitRules._fields_]
    assert int(re.search(r"#define ERGM_NGRAM_MAX (\d+)", src).group(1)) == L.NGRAM_MAX == _rules.NGRAM_MAX == 8


def _rules_struct(p, ld_hist=64, ld_bad=16, hist=True, bad=True):
    return L.LogitRules(hist=p.value if hist else None, ld_hist=ld_hist, start=p.value, ngram=p.value,
                        bad=p.value if bad else None, ld_bad=ld_bad)


def test_apply_refuses_before_any_launch():
    lib = L.load()
    keep, p = CA._buf()
    V, ldl = 500, 512
    good = _rules_struct(p)

    def apply(logits=p, ldl=ldl, R=4, V=V, rules=good, lens=p, eos=7, max_len=64):
        return lib.ergm_logit_rules_apply(logits, ldl, R, V, None if rules is None else C.byref(rules), lens, None, eos,
                                          max_len, None)

    def refused(word, **kw):
        assert apply(**kw) == L.ERGM_EINVAL
        assert word in L.last_error(), (word, L.last_error())

    refused("null", logits=None)
    refused("null", rules=None)
    refused("null", lens=None)
    refused("ldl", ldl=V - 1)
    refused("V", V=52 * 1024 + 1, ldl=60000)
    refused("V", V=0)
    refused("ld_hist", rules=_rules_struct(p, ld_hist=63))
    refused("hist", rules=_rules_struct(p, hist=False))
    refused("max_len", max_len=0)
    refused("max_len", max_len=1025, rules=_rules_struct(p, ld_hist=2048))
    refused("R", R=0)
    refused("R", R=65536)
    refused("eos_id", eos=-1)
    refused("eos_id", eos=V)
    refused("ld_bad", rules=_rules_struct(p, ld_bad=0))
    # both rules NULL: nothing to do and nothing launched (the pointers are fake)
    off = L.LogitRules(hist=p.value, ld_hist=64)
    assert apply(rules=off) == L.ERGM_OK


def test_history_entry_points_refuse_before_any_launch():
    lib = L.load()
    keep, p = CA._buf()
    E = L.ERGM_EINVAL
    write = lambda ids=p, total=10, slot=p, n_seq=2, n_slots=4, hist=p, ld=64, max_len=64: lib.ergm_hist_write(
        ids, total, slot, p, p, None, n_seq, n_slots, hist, ld, max_len, None)
    assert write(ids=None) == E and write(slot=None) == E and write(hist=None) == E
    assert write(total=0) == E and write(n_seq=0) == E and write(n_slots=0) == E
    assert write(max_len=0) == E and write(ld=63) == E and "ld_hist" in L.last_error()
    append = lambda tok=p, lens=p, R=4, hist=p, ld=64, max_len=64: lib.ergm_hist_append(tok, lens, None, R, hist, ld, max_len, None)
    assert append(tok=None) == E and append(lens=None) == E and append(hist=None) == E
    assert append(R=0) == E and append(max_len=0) == E and append(ld=63) == E
    follow = lambda hist=p, par=p, lens=p, R=8, W=4, ld=64, max_len=64: lib.ergm_hist_follow(hist, ld, par, lens, R, W, max_len, None)
    assert follow(hist=None) == E and follow(par=None) == E and follow(lens=None) == E
    assert follow(W=0) == E and follow(W=9) == E and follow(R=6) == E and follow(R=0) == E
    assert follow(max_len=0) == E and follow(ld=63) == E


def test_set_rules_on_an_unbound_plan():
    lib = L.load()
    plan, keep, p = CA._plan()
    try:
        good = _rules_struct(p, ld_hist=CA.TINY["max_len"])
        assert lib.ergm_decode_set_rules(plan, C.byref(good)) == L.ERGM_OK
        assert lib.ergm_decode_set_rules(plan, None) == L.ERGM_OK
        assert lib.ergm_decode_set_rules(plan, C.byref(_rules_struct(p, ld_hist=CA.TINY["max_len"] - 1))) == L.ERGM_EINVAL
        assert "ld_hist" in L.last_error()
        assert lib.ergm_decode_set_rules(plan, C.byref(_rules_struct(p, hist=False))) == L.ERGM_EINVAL
        assert lib.ergm_decode_set_rules(plan, C.byref(_rules_struct(p, ld_bad=0))) == L.ERGM_EINVAL
        assert lib.ergm_decode_set_rules(None, None) == L.ERGM_EINVAL
        # the step's launch count is what it was, rules set or not
        n0 = lib.ergm_decode_launches(plan, 0)
        assert lib.ergm_decode_set_rules(plan, C.byref(good)) == L.ERGM_OK
        assert lib.ergm_decode_launches(plan, 0) == n0
        # the loops still refuse what they refused
        assert lib.ergm_decode_run_slots_sampled(plan, 8, 0.9, None, 1, 497, 499, p, None, None) == L.ERGM_EINVAL
        assert "slots bound" in L.last_error()
    finally:
        lib.ergm_decode_destroy(plan)


def test_sampling_params_validation():
    sp = SamplingParams()
    assert (sp.no_repeat_ngram_size, sp.no_repeat_scope, sp.bad_words_ids) == (0, "sequence", ())
    assert not sp.has_rules
    for bad in (dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=True),
                dict(no_repeat_ngram_size=2.0), dict(bad_words_ids=[[]]), dict(bad_words_ids=[list(range(9))]),
                dict(bad_words_ids=[[3, -1]]), dict(bad_words_ids=[[True]]), dict(bad_words_ids=[[1.0]]),
                dict(bad_words_ids=[5]), dict(bad_words_ids=5), dict(bad_words_ids="ab"), dict(bad_words_ids=[[2 ** 31]]),
                dict(no_repeat_scope="dialogue"), dict(no_repeat_scope=None)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    a = SamplingParams(no_repeat_ngram_size=8, no_repeat_scope="turn", bad_words_ids=[[1, 2], [7]])
    assert a.bad_words_ids == ((1, 2), (7,)) and a.has_rules
    b = SamplingParams(no_repeat_ngram_size=8, no_repeat_scope="turn", bad_words_ids=((1, 2), (7,)))
    assert a == b and hash(a) == hash(b) and len({a, b, sp}) == 2
    assert SamplingParams(bad_words_ids=[[4]]).has_rules and SamplingParams(no_repeat_ngram_size=1).has_rules
    with pytest.raises(Exception):
        a.no_repeat_ngram_size = 2   # frozen
    assert check_rules(3, "turn", [[1], (2, 3)]) == ((1,), (2, 3))


def test_pool_rows():
    assert pack_bad_words(((1, 2), (7,)), 8) == [2, 1, 2, 1, 7, 0, 0, 0]
    assert pack_bad_words(((1, 2), (7,)), 5) == [2, 1, 2, 1, 7]          # a full row needs no terminator
    assert _rules.parse_pool(pack_bad_words(((1, 2), (7,)), 5)) == [(1, 2), (7,)]
    with pytest.raises(ValueError, match="bad_words_cap"):
        pack_bad_words(((1, 2), (7,)), 4)
    assert pack_bad_words((), 3) == [0, 0, 0]


def _fake(controls, cap=8, max_len=32):
    """What ContinuousGenerator.check_sampling reads of its generator (building one needs a device)."""
    return SimpleNamespace(controls=controls, bad_words_cap=cap, max_len=max_len)


def test_generator_refuses_rules_it_cannot_serve():
    check = ContinuousGenerator.check_sampling
    ruled = SamplingParams(no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="controls=True"):
        check(_fake(False), ruled)
    check(_fake(True), ruled)
    check(_fake(True), None)
    check(_fake(True), SamplingParams(bad_words_ids=[[1, 2, 3], [4, 5, 6]]))       # 8 entries: fits exactly
    with pytest.raises(ValueError, match="bad_words_cap"):
        check(_fake(True), SamplingParams(bad_words_ids=[[1, 2, 3], [4, 5, 6], [7]]))
    with pytest.raises(ValueError, match="max_len"):
        check(_fake(True, max_len=2048), ruled)
    check(_fake(True, max_len=2048), SamplingParams(top_k=3))                       # no rule: no bound


class _Backend:
    """The scheduler's view of a generator: it refuses through check_sampling, like ContinuousGenerator."""

    def __init__(self, controls, cap=8):
        self.controls, self.bad_words_cap, self.max_len = controls, cap, 32

    check_sampling = ContinuousGenerator.check_sampling

    def extend_requests(self, slots, requests):
        pass

    def admit_requests(self, slots, requests):
        self.left = {s: r.max_new for s, r in zip(slots, requests)}

    def run_chunk(self, n):
        rows = [[1, 1] for _ in range(n)]
        done = [0, 0]
        for s in list(self.left):
            self.left[s] -= n
            done[s] = int(self.left[s] <= 0)
        return rows, done


def test_scheduler_refuses_through_the_backend():
    ruled = SamplingParams(no_repeat_ngram_size=3, bad_words_ids=[[5]])
    off = SlotScheduler(_Backend(False), max_batch=2, max_len=32, cap_max=8)
    with pytest.raises(ValueError, match="controls=True"):
        off.submit(4, 3, 6, sampling=ruled)
    assert not off.queue and not off._active
    on = SlotScheduler(_Backend(True), max_batch=2, max_len=32, cap_max=8)
    rid = on.submit(4, 3, 8, sampling=ruled, keep=True)
    with pytest.raises(ValueError, match="bad_words_cap"):
        on.submit(4, 3, 6, sampling=SamplingParams(bad_words_ids=[[1, 2, 3, 4], [5, 6, 7, 8]]))
    assert len(on.queue) == 1
    on.run(eos_id=-1)
    with pytest.raises(ValueError, match="bad_words_cap"):
        on.extend(rid, 2, 3, sampling=SamplingParams(bad_words_ids=[[1, 2, 3, 4], [5, 6, 7, 8]]))
    assert rid in on.parked   # refused: still parked
    on.extend(rid, 2, 3, sampling=ruled)


def test_python_rule_against_brute_force():
    """Random short histories over a 4-token alphabet: the rule's banned set equals the set of tokens whose appending
    would complete an n-gram already present in [s0, L), found by enumerating all n-grams."""
    rng = np.random.default_rng(0)
    seen_nonempty = 0
    for _ in range(4000):
        L_ = int(rng.integers(0, 13))
        h = [int(x) for x in rng.integers(0, 4, L_)]
        n = int(rng.integers(1, 6))
        s0 = int(rng.integers(0, L_ + 1))
        got = _rules.banned(h + [9, 9], L_, 64, 4, -1, n, s0)     # what lies past the length is not history
        want = _rules.brute_force_ngram(h, n, s0)
        assert got == want, (h, n, s0)
        seen_nonempty += bool(want)
        # the property itself: appending an allowed token never repeats an n-gram that ends at the new token
        for j in set(range(4)) - got:
            seq = h[s0:] + [j]
            assert len(seq) < n or tuple(seq[-n:]) not in {tuple(seq[i:i + n]) for i in range(len(seq) - n)}
    assert seen_nonempty > 400   # a tenth of the draws at least ban something: the comparison is not of empty sets
    # eos is exempt, ids outside the vocabulary ban nothing, lengths clamp
    assert _rules.banned([1, 2, 1], 3, 64, 4, 2, 2) == set()
    assert _rules.banned([1, 7, 1], 3, 64, 4, -1, 2) == set()
    assert _rules.banned([1, 2, 1], 99, 3, 4, -1, 2) == {2} and _rules.banned([1, 2, 1], -5, 3, 4, -1, 1) == set()
    assert _rules.banned([3, 1], 2, 64, 4, -1, 0, 0, [(1, 2), (3, 0), (0,)]) == {2, 0}
