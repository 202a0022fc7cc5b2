"""Per-request sampling controls without a GPU: ergm_sample_rows, ergm_sample_mark and
ergm_decode_run_slots_sampled are declared, bound and exported with the ABI still 14; their argument checks refuse with
ERGM_EINVAL on fake pointers before anything launches; SamplingParams validates on the host; and SlotScheduler carries a
request's value to the backend and refuses a minimum length above the bound."""
import ctypes as C
import math
import os
import re

import pytest

from ergm_amd import _lib as L
from ergm_amd.generate import SamplingParams, SlotScheduler

import test_continuous_abi as CA

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ergm_hip.h")
NEW = ["ergm_sample_rows", "ergm_sample_mark", "ergm_decode_run_slots_sampled"]


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14
    # the struct's fields, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} ergm_sample_ctl;", src).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in L.SampleCtl._fields_]


def test_sample_rows_refuses_before_any_launch():
    lib = L.load()
    keep, p = CA._buf()
    V, ldl = 500, 512

    def rows(logits=p, ldl=ldl, B=2, V=V, top_p=0.9, ctl=None, ids=p, steps=p, tokens=p):
        return lib.ergm_sample_rows(logits, ldl, B, V, top_p, ctl, 1, ids, steps, None, 7, tokens, None, None, None, None)

    def refused(word, **kw):
        assert rows(**kw) == L.ERGM_EINVAL
        assert word in L.last_error(), (word, L.last_error())

    refused("null logits", logits=None)
    refused("null logits or tokens", tokens=None)
    refused("row_ids", ids=None)
    refused("row_steps", steps=None)
    refused("outside", V=0)
    refused("outside", V=52 * 1024 + 1, ldl=60000)
    refused("bad shape", B=0)
    refused("bad shape", ldl=V - 1)
    refused("NaN", top_p=float("nan"))
    ctl = L.SampleCtl(seen=p.value, ld_seen=(V + 31) // 32 - 1)
    refused("ld_seen", ctl=C.byref(ctl))
    ctl = L.SampleCtl(seen=p.value, ld_seen=0)
    refused("ld_seen", ctl=C.byref(ctl))


def test_sample_mark_refuses_before_any_launch():
    lib = L.load()
    keep, p = CA._buf()

    def mark(ids=p, total=10, slot=p, start=p, length=p, n_seq=2, V=500, n_slots=4, seen=p, ld_seen=16, steps=p, ms=p):
        return lib.ergm_sample_mark(ids, total, slot, start, length, None, None, n_seq, V, n_slots, seen, ld_seen, steps, ms, None)

    def refused(word, **kw):
        assert mark(**kw) == L.ERGM_EINVAL
        assert word in L.last_error(), (word, L.last_error())

    refused("null", ids=None)
    refused("null", slot=None)
    refused("null", start=None)
    refused("null", length=None)
    refused("neither", seen=None, ms=None, steps=None)
    refused("together", steps=None)
    refused("bad shape", n_seq=0)
    refused("bad shape", total=0)
    refused("bad shape", V=0)
    refused("bad shape", n_slots=0)
    refused("ld_seen", ld_seen=15)


def test_run_slots_sampled_refuses_like_run_slots():
    lib = L.load()
    plan, keep, p = CA._plan()
    try:
        ptrs = (C.c_void_p * 2)(p.value, p.value)
        run = lambda n=8, top_p=0.9, out=p, plan=plan: lib.ergm_decode_run_slots_sampled(plan, n, top_p, None, 1, 497, 499, out,
                                                                                         None, None)
        assert run() == L.ERGM_EINVAL and "slots bound" in L.last_error()
        assert lib.ergm_decode_bind_slots(plan, ptrs, ptrs, p, p, p, p, p, p, p) == L.ERGM_OK
        assert run(n=0) == L.ERGM_EINVAL and "n 0" in L.last_error()
        assert run(top_p=float("nan")) == L.ERGM_EINVAL and "NaN" in L.last_error()
        assert run(out=None) == L.ERGM_EINVAL and "null" in L.last_error()
        assert run(plan=None) == L.ERGM_EINVAL
        # the step's launch count is what it was
        assert lib.ergm_decode_launches(plan, 0) - lib.ergm_decode_launches(plan, 1) == 3 * CA.TINY["n_layer"]
    finally:
        lib.ergm_decode_destroy(plan)


def test_sampling_params_validation():
    sp = SamplingParams()
    assert (sp.top_p, sp.temperature, sp.top_k, sp.repetition_penalty) == (None, 1.0, 0, 1.0)
    assert (sp.min_new_tokens, sp.logprobs) == (0, False)
    SamplingParams(top_p=0.5, temperature=0.7, top_k=50, repetition_penalty=1.2, min_new_tokens=3, logprobs=True)
    with pytest.raises(Exception):
        sp.top_k = 3   # frozen
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf),
                dict(repetition_penalty=0.0), dict(repetition_penalty=-2.0), dict(repetition_penalty=math.nan),
                dict(repetition_penalty=math.inf), dict(top_p=math.nan), dict(top_p=math.inf), dict(top_k=-1),
                dict(top_k=1.5), dict(top_k=2 ** 31), dict(min_new_tokens=-1), dict(min_new_tokens=2.0),
                dict(temperature="1")):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    SamplingParams(min_new_tokens=4).check_bound(4)
    with pytest.raises(ValueError, match="min_new_tokens"):
        SamplingParams(min_new_tokens=5).check_bound(4)


class _Backend:
    """Every request draws token 1 until its bound; records what the scheduler hands over."""

    def __init__(self, max_batch):
        self.left = [0] * max_batch
        self.admitted, self.extended = [], []

    def admit_requests(self, slots, requests):
        self.admitted += [(r.id, r.sampling) for r in requests]
        for s, r in zip(slots, requests):
            self.left[s] = r.max_new

    def extend_requests(self, slots, requests):
        self.extended += [(r.id, r.sampling) for r in requests]
        for s, r in zip(slots, requests):
            self.left[s] = r.max_new

    def run_chunk(self, n):
        rows = []
        for _ in range(n):
            rows.append([1] * len(self.left))
            self.left = [max(0, k - 1) for k in self.left]
        return rows, [int(k == 0) for k in self.left]


def test_scheduler_carries_sampling_to_the_backend():
    be = _Backend(2)
    sched = SlotScheduler(be, max_batch=2, max_len=32, cap_max=8)
    a, b = SamplingParams(top_k=5, min_new_tokens=2), SamplingParams(temperature=0.5)
    ia = sched.submit(4, 3, 6, payload="a", keep=True, sampling=a)
    ib = sched.submit(5, 3, 4, payload="b")
    with pytest.raises(ValueError, match="min_new_tokens"):
        sched.submit(4, 3, 2, sampling=SamplingParams(min_new_tokens=3))
    with pytest.raises(ValueError, match="min_new_tokens"):   # the default bound: to the end of the cache
        sched.submit(30, 3, sampling=SamplingParams(min_new_tokens=3))
    assert len(sched.queue) == 2   # a refused request leaves nothing behind
    out = sched.run(eos_id=-1)
    assert be.admitted == [(ia, a), (ib, None)]
    assert len(out[ia]) == 6 and len(out[ib]) == 4
    with pytest.raises(ValueError, match="min_new_tokens"):
        sched.extend(ia, 2, 3, sampling=SamplingParams(min_new_tokens=4))
    assert ia in sched.parked   # refused: still parked
    sched.extend(ia, 2, 3, payload="t", sampling=b)
    assert len(sched.run(eos_id=-1)[ia]) == 3
    sched.extend(ia, 2, 3, payload="t")
    sched.run(eos_id=-1)
    assert be.extended == [(ia, b), (ia, None)]
