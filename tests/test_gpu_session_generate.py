"""The session store in ContinuousGenerator (session_store=True) on the GPU: a parked session's state survives the trip
through a blob into another slot bit for bit on all three engines, which pack the same state into the same bytes; a
three-turn session that is offloaded after every turn gives the tokens, final logits and log-probabilities of the run
without a store; a fork shares its origin's history and draws under its own id; 12 two-turn sessions are served on 4
slots, which the generator without a store refuses; and where nothing has to leave, nothing is saved.  Model, prompts
and helpers are tests/test_gpu_generate_batched.py's, tests/test_gpu_continuous.py's and tests/test_gpu_extend.py's."""
from dataclasses import replace

import pytest
import torch

import test_gpu_continuous as TC
import test_gpu_extend as XE
import test_gpu_generate_batched as TB
from ergm_amd import _lib as L
from ergm_amd.generate import SamplingParams

pytestmark = pytest.mark.gpu
E, SP2, NO_EOS, ENGINES = TB.E, TB.SP2, TC.NO_EOS, TC.ENGINES
RUN = dict(top_p=0.9, eos_id=NO_EOS, sp2_id=SP2, seed=7)
RUN_EOS = dict(RUN, eos_id=TB.EOS)   # the logit rules need an eos inside the vocabulary; min_new_tokens keeps it away
RULED = SamplingParams(top_p=0.8, temperature=0.9, top_k=40, repetition_penalty=1.2, min_new_tokens=6,
                       no_repeat_ngram_size=2, bad_words_ids=((3, 4), (7,)))
WORDS = ("row_ids", "row_steps", "min_step")


def _slot_state(gen, slot, n, c):
    """What travels of a slot, as CPU copies."""
    s = {k: getattr(gen, k)[slot].cpu().clone() for k in WORDS}
    s["kv"] = [t[slot, :n].cpu().clone() for t in gen.kv]
    s["xkv"] = [t[slot, :c].cpu().clone() for t in gen.xkv]
    s["ctl"], s["seen"] = gen._ctl_vals[:, slot].cpu().clone(), gen.seen[slot].cpu().clone()
    s["rule"], s["bad"], s["hist"] = gen._rule_vals[:, slot].cpu().clone(), gen._bad_pool[slot].cpu().clone(), gen.hist[slot, :n].cpu().clone()
    return s


def _put_slot_state(gen, slot, n, c, s):
    for k in WORDS:
        getattr(gen, k)[slot] = s[k].to(gen.dev)
    for t, x in zip(gen.kv, s["kv"]):
        t[slot, :n] = x.to(gen.dev)
    for t, x in zip(gen.xkv, s["xkv"]):
        t[slot, :c] = x.to(gen.dev)
    gen._ctl_vals[:, slot], gen.seen[slot] = s["ctl"].to(gen.dev), s["seen"].to(gen.dev)
    gen._rule_vals[:, slot], gen._bad_pool[slot], gen.hist[slot, :n] = s["rule"].to(gen.dev), s["bad"].to(gen.dev), s["hist"].to(gen.dev)


def _same_slot_state(a, b, what):
    for k in a:
        if isinstance(a[k], list):
            for l, (x, y) in enumerate(zip(a[k], b[k])):
                assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f"{what}: {k} of layer {l}"
        else:
            assert torch.equal(a[k], b[k]), f"{what}: {k}"


def test_round_trip_state_and_one_blob_on_all_engines(gpu):
    """Per engine: a session with controls and a rule is served to its park beside another request, its slot gets the
    state the "python" engine left (the engines' own caches differ in their last bits, the blob of one state must not),
    it is offloaded, two other requests run through its slot, and it is loaded into a different slot."""
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E, lens=(5, 12, 6, 9), cap_lens=(7, 12, 3, 16), with_feat=1, seed=31), gpu)
    canon = blob0 = None
    for engine in ENGINES:
        gen = XE._gen(model, engine, controls=True, session_store=True)
        a = gen.submit(prompts[1], 6, keep=True, sampling=RULED)
        gen.submit(prompts[0], 3)
        out = gen.run(**RUN_EOS)
        slot, n, c = gen.sched.parked[a]
        assert n == 12 + 6 and c == 12 and len(out[a]) == 6 and gen._slot_ruled[slot]
        if canon is None:
            canon = _slot_state(gen, slot, n, c)
        _put_slot_state(gen, slot, n, c, canon)
        host = (gen._slot_sp[slot], list(gen._hist_host[slot]), gen._cap_host[slot])
        assert gen.session_bytes(slot, n, c) == 64 + 2 * (n + c) * 4 * E + 32 + 64 + 16 + 256 + 80
        gen.offload(a)
        assert gen.save_calls == 1 and gen.sched.stored == {a: (n, c)} and a not in gen.sched.parked
        blob = gen._store[a].blob
        assert blob.dtype == torch.uint8 and blob.numel() == gen.stored_bytes == gen.sched.stored_bytes
        if blob0 is None:
            blob0 = blob.cpu().clone()
        assert torch.equal(blob.cpu(), blob0), f"{engine}: the blob differs from the python engine's"
        hdr = blob0[:64].view(torch.int32).tolist()
        assert hdr[:7] == [L.SESSION_MAGIC, 1, L.SESSION_CTL | L.SESSION_RULES, 2, 4 * E, n, c] and hdr[7] == a
        # the slot is idle, carries no rule and its host records are a new tenant's
        assert (int(gen.finished[slot]), int(gen.lens[slot]), int(gen.cap_lens[slot])) == (1, 0, 0)
        assert not gen._rule_vals[:, slot].any() and not gen._bad_pool[slot].any()
        assert gen._slot_sp[slot] is None and gen._hist_host[slot] == [] and not gen._slot_ruled[slot]
        # other requests run through the slot
        ids = [gen.submit(prompts[i], 4) for i in (2, 3, 0, 2)]
        out = gen.run(**RUN_EOS)
        assert sorted(out) == ids and slot in [s for _, s in gen.sched.admissions[-1]]
        dest = (slot + 2) % 4
        gen.load_sessions([dest], [a])
        assert gen.load_calls == 1
        _same_slot_state(_slot_state(gen, dest, n, c), canon, engine)
        assert [int(getattr(gen, k)[dest]) for k in ("lens", "cap_lens", "stop_lens", "finished")] == [n, c, n, 1]
        assert (gen._slot_sp[dest], gen._hist_host[dest], gen._cap_host[dest]) == host and gen._slot_ruled[dest]
        assert torch.equal(gen._store[a].blob.cpu(), blob0)       # a load writes no blob


def _three_turns(model, gpu, store):
    """A session (request 9, the last admitted of four) through three turns beside other requests; with ``store`` it is
    offloaded after every turn.  Returns per turn its tokens, final logits and log-probabilities, and the generator."""
    prompts = TB._dev(TB._prompts(E, lens=XE.REQ_LENS[:4], cap_lens=XE.REQ_CAPS[:4], with_feat=1, seed=31), gpu)
    gen = XE._gen(model, "fused", max_admit=1, keep_logits=True, controls=True, session_store=store)
    sp = SamplingParams(top_k=60, temperature=0.95, repetition_penalty=1.1, logprobs=True, no_repeat_ngram_size=3,
                        min_new_tokens=5)
    out, slots = [], []
    for turn in range(3):
        if turn == 2:   # a request alone in between takes the slot the session would return to
            gen.submit(prompts[0], 2)
            gen.run(**RUN_EOS)
        for i in (0, 2, 3):
            gen.submit(prompts[i], XE.REQ_NEW[i], request_id=i)
        if turn == 0:
            gen.submit(prompts[1], 5, request_id=9, keep=True, sampling=sp)
        else:
            gen.extend_request(9, *[t.to(gpu) for t in XE._turns((2 + turn,), seed=40 + turn)[0]], 3,
                               sampling=replace(sp, min_new_tokens=3))
        res = gen.run(**RUN_EOS)
        slots.append(gen.sched.parked[9][0])
        out.append((res[9], gen.final_logits[9].clone().cpu(), list(gen.token_logprobs[9])))
        if store:
            gen.offload(9)
    return out, slots, gen


def test_three_turns_through_the_store_are_the_run_without_it(gpu):
    _, _, model = TB._setup(gpu)
    ref, ref_slots, _ = _three_turns(model, gpu, store=False)
    got, slots, gen = _three_turns(model, gpu, store=True)
    assert len(set(ref_slots)) == 1 and slots[0] != slots[1] != slots[2]     # it came back into other slots
    assert gen.save_calls == 3 and gen.load_calls == 2 and [len(c) for c in gen.sched.loads] == [1, 1]
    for turn, ((t0, l0, p0), (t1, l1, p1)) in enumerate(zip(ref, got)):
        assert t0 == t1 and len(t0) == (5, 3, 3)[turn], turn
        assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), turn
        assert torch.tensor(p0).view(torch.int32).tolist() == torch.tensor(p1).view(torch.int32).tolist() and len(p0) == len(t0)
    assert gen.sched.stored[9][0] == XE.REQ_LENS[1] + 5 + 3 + 3 + 4 + 3 == 30


def test_a_fork_shares_the_history_and_draws_under_its_own_id(gpu):
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E, lens=XE.REQ_LENS[:2], cap_lens=XE.REQ_CAPS[:2], with_feat=1, seed=31), gpu)
    gen = XE._gen(model, "fused", max_admit=1, session_store=True)
    a = gen.submit(prompts[1], 6, keep=True)
    gen.run(**RUN)
    n = gen.sched.parked[a][1]
    f = gen.fork_request(a)                                   # parked: offloaded first
    assert f != a and gen.save_calls == 1 and sorted(gen.sched.stored) == [a, f]
    assert gen._store[f].blob is gen._store[a].blob and gen.stored_bytes == gen._store[a].blob.numel()
    with pytest.raises(ValueError):
        gen.fork_request(77)
    ids, tt = (t.to(gpu) for t in XE._turns((4,), seed=51)[0])
    gen.extend_request(a, ids, tt, 8)
    gen.extend_request(f, ids, tt, 8)
    out = gen.run(**RUN)
    assert gen.load_calls == 1 and len(out[a]) == len(out[f]) == 8 and out[a] != out[f]     # another id, other draws
    (sa, na, _), (sf, nf, _) = gen.sched.parked[a], gen.sched.parked[f]
    assert sa != sf and na == nf == n + 4 + 8 and not gen._store
    assert int(gen.row_ids[sa]) == a and int(gen.row_ids[sf]) == f
    for l, t in enumerate(gen.kv):                            # the history both grew from: bitwise one cache
        assert torch.equal(t[sa, :n].view(torch.int16), t[sf, :n].view(torch.int16)), l
    # the origin alone, without a store, continues as the origin did here
    solo = XE._gen(model, "fused", max_admit=1)
    solo.submit(prompts[1], 6, request_id=a, keep=True)
    solo.run(**RUN)
    solo.extend_request(a, ids, tt, 8)
    assert solo.run(**RUN)[a] == out[a]


N_SESS = 12
S_LENS, S_CAPS = (5, 8, 3, 6, 4, 7, 2, 8, 5, 3, 6, 4), (7, 12, 1, 16, 3, 5, 9, 2, 16, 4, 8, 6)


def _serve_sessions(gen, prompts, gpu):
    """Every prompt as a kept session of 4 new tokens, then a second turn of 3 tokens and 4 new ones for each."""
    ids = [gen.submit(p, 4, keep=True) for p in prompts]
    first = gen.run(**RUN)
    for i in ids:
        gen.extend_request(i, *[t.to(gpu) for t in XE._turns((3,), seed=60 + i)[0]], 4)
    return ids, first, gen.run(**RUN)


@pytest.mark.parametrize("engine", ENGINES)
def test_more_sessions_than_slots(gpu, engine):
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E, lens=S_LENS, cap_lens=S_CAPS, with_feat=1, seed=5), gpu)
    gen = XE._gen(model, engine, session_store=True)
    ids, first, second = _serve_sessions(gen, prompts, gpu)
    assert sorted(first) == sorted(second) == ids and all(len(first[i]) == len(second[i]) == 4 for i in ids)
    assert gen.save_calls > 0 and gen.load_calls > 0 and gen.save_calls == len(gen.sched.saves)
    assert len(gen.sched.parked) + len(gen.sched.stored) == N_SESS and len(gen._store) == len(gen.sched.stored)
    rows = {**{i: r for i, (r, _) in gen.sched.stored.items()}, **{i: r for i, (_, r, _) in gen.sched.parked.items()}}
    assert rows == {i: n + 4 + 3 + 4 for i, n in zip(ids, S_LENS)}
    lens = gen.lens.cpu().tolist()
    assert all(lens[s] == r for s, r, _ in gen.sched.parked.values())
    assert gen.stored_bytes == gen.sched.stored_bytes == sum(64 + 2 * (rows[i] + S_CAPS[i]) * 4 * E for i in gen.sched.stored)
    for i in ids:
        gen.release(i)
    assert gen.stored_bytes == 0 and not gen._store
    # the generator without a store cannot serve them
    gen = XE._gen(model, engine)
    for p in prompts:
        gen.submit(p, 4, keep=True)
    with pytest.raises(RuntimeError, match="every slot is parked"):
        gen.run(**RUN)
    for what in (lambda: gen.offload(0), lambda: gen.fork_request(0), lambda: gen.save_sessions([0], [0])):
        with pytest.raises(ValueError, match="session_store=True"):
            what()
    with pytest.raises(ValueError):
        XE._gen(model, engine, session_store=True, num_beams=2)
    with pytest.raises(ValueError):
        XE._gen(model, engine, session_store_bytes=1 << 20)


def test_nothing_is_saved_where_nothing_has_to_leave(gpu):
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E, lens=S_LENS[:4], cap_lens=S_CAPS[:4], with_feat=1, seed=5), gpu)
    runs = []
    for store in (False, True):
        gen = XE._gen(model, "fused", session_store=store)
        runs.append(_serve_sessions(gen, prompts, gpu))
        assert gen.save_calls == gen.load_calls == 0 and not gen.sched.saves and len(gen.sched.parked) == 4
    assert runs[0] == runs[1]
