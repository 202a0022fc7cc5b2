"""no_repeat_ngram_size and bad_words_ids end to end: ContinuousGenerator (sampling, sessions) and BatchedGenerator
(beams) on all three engines.  Model, prompts and sizes are tests/test_gpu_sample_generate.py's, max_len = 48 where 24
new tokens need the room.

The top-two logit gaps of this model go down to 1e-3, so nothing here is compared with the fp64 oracle: a ruled run is
compared with a host-driven loop on a second generator of the same engine and max_batch, which reads the device's own
logits, applies the plain-Python rule (tests/_rules.py), takes the arg-max (lowest id on ties) and steps.  The two share
every kernel, so the token lists are equal exactly.  The preconditions that keep this from passing vacuously are
asserted: unruled greedy decoding repeats a trigram in every request, and with n = 2 the rule overrules the device's
own arg-max in at least one round of every request."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import _rules
import _sample
import test_gpu_generate_batched as TB
import test_gpu_sample_generate as TS
from ergm_amd.generate import BatchedGenerator, ContinuousGenerator, SamplingParams, beam_backtrack

pytestmark = pytest.mark.gpu
V, E, SP1, SP2, EOS = TB.V, TB.E, TB.SP1, TB.SP2, TB.EOS
ENGINES = TS.ENGINES
TOP_P, N_NEW, MAX_LEN = 0.9, 24, 48
GREEDY = SamplingParams(top_k=1)
_ref = {}   # (engine, what) -> lists computed once and shared between tests


def _gen(model, engine, controls=True, max_batch=8, max_len=MAX_LEN, **kw):
    return ContinuousGenerator(model, max_batch=max_batch, max_len=max_len, cap_max=16, engine=engine, controls=controls, **kw)


def _ids(p):
    return [int(t) for t in p[0].reshape(-1).tolist()]


def _idx(ban):
    return np.array(sorted(ban), dtype=np.int64)


def _host_loop(model, engine, prompts, n_new, n=0, scope="sequence", words=None, max_batch=8):
    """Greedy decoding of ``prompts`` with the rule applied on the host to the device's own logits: one admission into
    slots 0 .. (what ``generate`` does with an empty generator), then read logits, ban, arg-max, step.  Returns the token
    lists (each ending at its first eos) and, per request, the rounds in which the unruled arg-max was banned.
    ``words``: one list of bad-word tuples per request."""
    gen = _gen(model, engine, controls=False, max_batch=max_batch)
    k = len(prompts)
    words = [()] * k if words is None else words
    gen.admit(list(range(k)), prompts, [n_new] * k, list(range(k)))
    hist = [_ids(p) for p in prompts]
    s0 = [len(h) if scope == "turn" else 0 for h in hist]
    out, overruled, live = [[] for _ in range(k)], [0] * k, [True] * k
    tt = torch.full((gen.max_batch,), SP2, dtype=torch.int64, device=gen.dev)
    for i in range(n_new):
        x = gen.logits.float().cpu().numpy()
        tok = [0] * gen.max_batch
        for b in range(k):
            if not live[b]:
                continue
            ban = _rules.banned(hist[b], len(hist[b]), MAX_LEN, V, EOS, n, s0[b], words[b])
            overruled[b] += int(int(x[b].argmax()) in ban)
            row = x[b].copy()
            row[_idx(ban)] = -np.inf
            tok[b] = int(row.argmax())
            out[b].append(tok[b])
            hist[b].append(tok[b])
            live[b] = tok[b] != EOS
        if i + 1 < n_new:
            gen.step(torch.tensor(tok, dtype=torch.int64, device=gen.dev), tt)
    return out, overruled


def _six(gpu):
    return TS._six(gpu)


def _unruled(model, engine, prompts):
    key = (engine, "unruled")
    if key not in _ref:
        _ref[key] = _gen(model, engine).generate(prompts, TOP_P, EOS, SP2, seed=7, max_new_tokens=N_NEW, sampling=GREEDY)
    return _ref[key]


@pytest.mark.parametrize("engine", ENGINES)
def test_the_model_repeats_itself_without_the_rule(gpu, engine):
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    out = _unruled(model, engine, prompts)
    host, _ = _host_loop(model, engine, prompts, N_NEW)
    assert out == host   # the host loop is the generator's greedy path when nothing is banned
    for p, o in zip(prompts, out):
        print(f"{engine}: {len(o)} tokens, tail {o[-4:]}")
        assert _rules.repeats(o, 3), o


@pytest.mark.parametrize("scope", ["sequence", "turn"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("engine", ENGINES)
def test_ruled_greedy_is_the_host_loop(gpu, engine, n, scope):
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    sp = SamplingParams(top_k=1, no_repeat_ngram_size=n, no_repeat_scope=scope)
    gen = _gen(model, engine)
    out = gen.generate(prompts, TOP_P, EOS, SP2, seed=7, max_new_tokens=N_NEW, sampling=sp)
    host, overruled = _host_loop(model, engine, prompts, N_NEW, n, scope)
    print(f"{engine} n={n} {scope}: rounds overruled per request {overruled}, lengths {[len(o) for o in out]}")
    assert out == host
    assert min(overruled) >= 1   # the rule changed every request (the issue's CPU runs: 13 to 15 rounds at n = 2)
    for p, o in zip(prompts, out):
        if scope == "sequence":
            assert not _rules.repeats(_ids(p) + o, n)
        else:
            assert not _rules.repeats(o, n)
    assert out != _unruled(model, engine, prompts)
    assert len(gen.sched.admissions) == 1   # one admission of six, as the host loop's


# three of the six requests carry rules, no two alike; three carry none
def _mixed_ruled():
    m = list(TS.MIXED)
    m[0] = replace(m[0], no_repeat_ngram_size=2)
    m[2] = replace(m[2], no_repeat_ngram_size=3, no_repeat_scope="turn", bad_words_ids=[[5, 6], [17]])
    m[4] = replace(m[4], bad_words_ids=[[3], [101, 102, 103], [250]], no_repeat_ngram_size=1)
    return m


RULED = (0, 2, 4)


def _run_mixed(model, engine, prompts, params, **kw):
    gen = _gen(model, engine, max_batch=4, max_len=32, **kw)
    ids = [gen.submit(p, 9, sampling=sp) for p, sp in zip(prompts, params)]
    out = gen.run(TOP_P, EOS, SP2, seed=5)
    return [out[i] for i in ids], gen.token_logprobs, gen


def test_native_is_bitwise_python(gpu):
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    params = _mixed_ruled()
    py, py_lp, _ = _run_mixed(model, "python", prompts, params)
    nat, nat_lp, gen = _run_mixed(model, "native", prompts, params)
    assert nat == py
    assert sorted(py_lp) == sorted(nat_lp) == [i for i, sp in enumerate(params) if sp.logprobs]
    for i, lp in py_lp.items():
        assert len(lp) == len(py[i]) and all(x <= 0.0 for x in lp)
        assert np.array(lp, dtype=np.float32).tobytes() == np.array(nat_lp[i], dtype=np.float32).tobytes()
    assert len(gen.sched.admissions) >= 2   # six requests over four slots: slots were reused behind ruled tenants
    assert len(set(py[4])) == len(py[4])   # n = 1: no token twice
    plain, _, _ = _run_mixed(model, "python", prompts, TS.MIXED)
    assert [py[i] for i in RULED] != [plain[i] for i in RULED]   # the rules took part in the draws


def test_results_do_not_depend_on_the_schedule(gpu):
    """Engine "fused", max_admit = 1 (rows independent of their neighbours): each request alone returns what it returns
    among the others, the unruled requests return what they return when nobody carries a rule, and the slots are reused
    behind ruled tenants without inheriting anything."""
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    params = _mixed_ruled()
    together, lp, _ = _run_mixed(model, "fused", prompts, params, max_admit=1)
    plain, _, _ = _run_mixed(model, "fused", prompts, TS.MIXED, max_admit=1)
    for i in range(6):
        if i not in RULED:
            assert together[i] == plain[i], i
    solo = _gen(model, "fused", max_batch=4, max_len=32, max_admit=1)
    for i in (5, 0, 3, 2, 1, 4):
        rid = solo.submit(prompts[i], 9, request_id=i, sampling=params[i])
        assert solo.run(TOP_P, EOS, SP2, seed=5)[rid] == together[i], i
        if params[i].logprobs:
            assert solo.token_logprobs[i] == lp[i]


@pytest.mark.parametrize("engine", ENGINES)
def test_no_rule_is_the_parent_path(gpu, engine):
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    old = _gen(model, engine, controls=False, max_batch=4, max_len=32).generate(prompts, TOP_P, EOS, SP2, seed=7, max_new_tokens=10)
    gen = _gen(model, engine, max_batch=4, max_len=32)
    assert gen.generate(prompts, TOP_P, EOS, SP2, seed=7, max_new_tokens=10) == old
    assert not any(gen._slot_ruled) and not gen._rules_bound
    assert int(gen.hist.abs().sum().item()) == 0   # no history was written: the launches are the parent's
    with pytest.raises(ValueError, match="controls=True"):
        _gen(model, engine, controls=False).submit(prompts[0], sampling=SamplingParams(no_repeat_ngram_size=2))
    with pytest.raises(ValueError, match="bad_words_cap"):
        _gen(model, engine, bad_words_cap=4).submit(prompts[0], sampling=SamplingParams(bad_words_ids=[[1, 2], [3, 4]]))
    with pytest.raises(ValueError, match="bad_words_cap"):
        _gen(model, engine, bad_words_cap=4).admit([0], prompts[:1], sampling=[SamplingParams(bad_words_ids=[[1, 2], [3, 4]])])


@pytest.mark.parametrize("engine", ["python", "native"])
def test_bad_words(gpu, engine):
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    plain = _unruled(model, engine, prompts)
    one = [SamplingParams(top_k=1, bad_words_ids=[[u[0]]]) for u in plain]
    out = _gen(model, engine).generate(prompts, TOP_P, EOS, SP2, seed=7, max_new_tokens=N_NEW, sampling=one)
    for u, o in zip(plain, out):
        assert u[0] != EOS and u[0] not in o and o != u
    host, overruled = _host_loop(model, engine, prompts, N_NEW, words=[[(u[0],)] for u in plain])
    assert out == host and min(overruled) >= 1
    two = [SamplingParams(top_k=1, bad_words_ids=[[u[3], u[4]]]) for u in plain]
    out = _gen(model, engine).generate(prompts, TOP_P, EOS, SP2, seed=7, max_new_tokens=N_NEW, sampling=two)
    for u, o in zip(plain, out):
        assert all((x, y) != (u[3], u[4]) for x, y in zip(o, o[1:])) and o != u   # u itself holds the word at 3, 4
    host, _ = _host_loop(model, engine, prompts, N_NEW, words=[[(u[3], u[4])] for u in plain])
    assert out == host


@pytest.mark.parametrize("engine", ["python", "fused"])
def test_first_draw_is_the_rules_then_the_sampler(gpu, engine):
    """The first token of every request of the mixed set is tests/_sample.py applied to the slot's logits with the
    tokens tests/_rules.py bans taken out (NaN: the helper's mark for a token that holds no slot)."""
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    params = _mixed_ruled()
    gen = _gen(model, engine, max_batch=4, max_len=32)
    gen._sampling = (TOP_P, EOS, SP2, TS.FIRST_SEED)
    checked = 0
    for half, slots in ((range(0, 4), (2, 0, 3, 1)), (range(4, 6), (1, 3))):
        half = list(half)
        gen.finished.fill_(1)
        gen.admit(slots, [prompts[i] for i in half], request_ids=[10 + i for i in half], sampling=[params[i] for i in half])
        logits = gen.logits.float().cpu().numpy()
        tokens, _ = gen.run_chunk(1)
        for i, s in zip(half, slots):
            sp = params[i]
            h = _ids(prompts[i])
            s0 = len(h) if sp.no_repeat_scope == "turn" else 0
            ban = _rules.banned(h, len(h), 32, V, EOS, sp.no_repeat_ngram_size, s0, sp.bad_words_ids)
            row = logits[s].copy()
            row[_idx(ban)] = np.nan
            top_p = TOP_P if sp.top_p is None else sp.top_p
            proc = dict(seen=h, rep=sp.repetition_penalty, temp=sp.temperature)
            tok, gap, kept, _ = _sample.draw(row, top_p, _sample.uniform(TS.FIRST_SEED, 10 + i, 0), sp.top_k, **proc)
            print(f"request {i} slot {s}: token {tokens[0][s]} (helper {tok}), gap {gap:.2e}, banned {len(ban)}")
            assert tokens[0][s] not in ban
            if gap >= 1e-4:   # the helper's draw is decided in fp64: closer than this to a CDF boundary it may differ
                assert tokens[0][s] == tok, (i, tokens[0][s], tok)
                checked += 1
            assert gen.hist[s, len(h)].item() == tokens[0][s] or tokens[0][s] == EOS   # and the draw was recorded
            assert gen.hist[s, :len(h)].tolist() == h
    assert checked >= 4


@pytest.mark.parametrize("engine", ["python", "native"])
def test_sessions(gpu, engine):
    """Four sessions on one prompt; turn one is 6 greedy tokens t under n = 2, the other speaker's turn j ends in t[j].
    Scope "sequence": the second turn may not follow t[j] with a token that followed it in turn one; scope "turn": it
    may, and does wherever the device's own arg-max says so (asserted to happen for some j)."""
    _, _, model = TB._setup(gpu)
    p = _six(gpu)[3]
    k, n1, n2 = 4, 6, 4
    assert not _rules.repeats(_ids(p), 2)
    # the reference: a host loop for turn one, the extension, and the logits it leaves
    (t1, *same), _ = _host_loop(model, engine, [p] * k, n1, 2, max_batch=k)
    assert all(s == t1 for s in same) and len(t1) == n1 and EOS not in t1
    sep = min(set(range(V)) - set(_ids(p) + t1))   # the other speaker's first token: in no bigram so far
    probe = _gen(model, engine, controls=False, max_batch=k)
    probe.admit(list(range(k)), [p] * k, [n1] * k, list(range(k)))
    tt = torch.full((probe.max_batch,), SP2, dtype=torch.int64, device=gpu)
    for tok in t1:
        probe.step(torch.full((probe.max_batch,), tok, dtype=torch.int64, device=gpu), tt)
    turns = [(torch.tensor([sep, t1[j]], device=gpu), torch.full((2,), SP1, device=gpu)) for j in range(k)]
    past = len(_ids(p)) + n1
    probe.extend(list(range(k)), turns, [n2] * k, [past] * k)
    x = probe.logits.float().cpu().numpy()
    hist = [_ids(p) + t1 + [sep, t1[j]] for j in range(k)]
    assert not any(_rules.repeats(h, 2) for h in hist)
    plain = [int(x[j].argmax()) for j in range(k)]
    ban = [_rules.banned(h, len(h), MAX_LEN, V, EOS, 2, 0) for h in hist]
    first_seq = []
    for j in range(k):
        row = x[j].copy()
        row[_idx(ban[j])] = -np.inf
        first_seq.append(int(row.argmax()))
    differ = [j for j in range(k) if plain[j] in ban[j]]
    print(f"{engine}: turn one {t1}, plain first tokens {plain}, under 'sequence' {first_seq}, overruled at j = {differ}")
    assert differ   # some turn-two arg-max repeats a bigram of turn one: the scopes can be told apart

    def two_turns(scope):
        gen = _gen(model, engine, max_batch=k)
        sp = SamplingParams(top_k=1, no_repeat_ngram_size=2, no_repeat_scope=scope)
        rids = [gen.submit(p, n1, keep=True, sampling=sp) for _ in range(k)]
        out = gen.run(TOP_P, EOS, SP2, seed=2)
        assert all(out[r] == t1 for r in rids)
        for r, (ids, types) in zip(rids, turns):
            gen.extend_request(r, ids, types, n2)     # sampling=None keeps the session's rule
        out = gen.run(TOP_P, EOS, SP2, seed=2)
        return gen, rids, [out[r] for r in rids]

    gen, rids, t2 = two_turns("sequence")
    for j in range(k):
        assert t2[j][0] == first_seq[j]
        assert not _rules.repeats(hist[j] + t2[j], 2)
    gen_t, _, t2t = two_turns("turn")
    for j in range(k):
        assert t2t[j][0] == plain[j]
        assert not _rules.repeats(t2t[j], 2)
    assert all(_rules.repeats(hist[j] + t2t[j][:1], 2) for j in differ)   # "turn" let turn one's bigram back in
    slot = gen_t.sched.parked[0][0]
    assert gen_t._rule_vals[0, slot].item() == past + 2                    # s0 moved to the new turn's first draw
    # release, and two new tenants (one ruled, one not) in the slots the sessions held: nothing is inherited
    for r in rids:
        gen.release(r)
    others = _six(gpu)[:2]
    sps = [SamplingParams(top_k=1, no_repeat_ngram_size=2, bad_words_ids=[[9]]), GREEDY]
    again = gen.generate(others, TOP_P, EOS, SP2, seed=2, max_new_tokens=8, sampling=sps)
    fresh = _gen(model, engine, max_batch=k).generate(others, TOP_P, EOS, SP2, seed=2, max_new_tokens=8, sampling=sps)
    assert again == fresh
    s_plain = gen.sched.admissions[-1][1][1]
    assert gen._rule_vals[1, s_plain].item() == 0 and gen._bad_pool[s_plain, 0].item() == 0


# ---- beams ---------------------------------------------------------------------------------------------------------
LENS2, CAPS2 = (5, 12), (7, 12)


def _beams(model, engine, max_batch=8):
    return BatchedGenerator(model, max_batch=max_batch, max_len=32, engine=engine)


def _two(gpu):
    return _six(gpu)[:2]


def _beam_run(gen, prompts, W, rounds, **rules):
    gen.beam_prefill(prompts, W, EOS, SP2, **rules)
    toks, pars = [], []
    for n in rounds:
        t, p = gen.beam_round(n)
        toks += t
        pars += p
    return toks, pars, gen.beam_scores.cpu().numpy().tobytes()


def _beam_host(model, prompts, W, n_rounds, n=0, words=()):
    """The python engine without rules, its logits banned from the host before every round (beam_round(1) of the python
    engine is ops.beam_select, ops.beam_gather and the step)."""
    gen = _beams(model, "python")
    gen.beam_prefill(prompts, W, EOS, SP2)
    R = gen.B
    hist = [[] for _ in range(R)]
    for g, p in enumerate(prompts):
        hist[g * W] = _ids(p)
    toks, pars, overruled = [], [], 0
    for _ in range(n_rounds):
        fin = gen.finished[:R].cpu().tolist()
        x = gen._logits[:R].float().cpu().numpy()
        for r in range(R):
            if fin[r]:
                continue
            ban = _idx(_rules.banned(hist[r], len(hist[r]), 32, V, EOS, n, 0, words))
            overruled += int(ban.size > 0 and np.isfinite(x[r, :V]).any() and int(x[r, :V].argmax()) in ban)
            x[r, ban] = -np.inf
        gen._logits[:R].copy_(torch.from_numpy(x).to(gen.dev))
        (t,), (p,) = gen.beam_round(1)
        fin = gen.finished[:R].cpu().tolist()
        hist = [hist[p[r]] + ([] if fin[r] else [t[r]]) for r in range(R)]
        toks.append(t), pars.append(p)
    return toks, pars, gen.beam_scores.cpu().numpy().tobytes(), overruled


def _hyps(toks, pars, scores, W):
    return beam_backtrack(toks, pars, np.frombuffer(scores, dtype=np.float32).tolist(), W, EOS, 1.0, W)


def test_beams_native_python_and_the_host_loop_agree(gpu):
    _, _, model = TB._setup(gpu)
    prompts = _two(gpu)
    W = 4
    plain = _beam_run(_beams(model, "python"), prompts, W, (8, 1))
    for rules in (dict(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=2, bad_words_ids=[[plain[0][0][0]]])):
        py = _beam_run(_beams(model, "python"), prompts, W, (8, 1), **rules)
        nat = _beam_run(_beams(model, "native"), prompts, W, (8, 1), **rules)
        assert nat == py
        *host, overruled = _beam_host(model, prompts, W, 9, 2, [tuple(w) for w in rules.get("bad_words_ids", ())])
        print(f"{sorted(rules)}: a beam's arg-max was banned in {overruled} row-rounds")
        assert tuple(host) == py and overruled >= 1 and py != plain
        for g, hyps in enumerate(_hyps(*py, W)):
            assert hyps
            for h, _ in hyps:
                assert not _rules.repeats(_ids(prompts[g]) + h, 2), (g, h)
                assert all(w[0] not in h for w in rules.get("bad_words_ids", ()))
    # "turn": the prompt's bigrams do not count, the hypothesis' own do
    turn = _beam_run(_beams(model, "native"), prompts, W, (8, 1), no_repeat_ngram_size=2, no_repeat_scope="turn")
    for hyps in _hyps(*turn, W):
        assert all(not _rules.repeats(h, 2) for h, _ in hyps)


def test_beams_fused_and_trainer(gpu):
    _, _, model = TB._setup(gpu)
    prompts = _two(gpu)
    gen = _beams(model, "fused")
    plain = gen.beam_search(prompts, 4, EOS, SP2, max_new_tokens=12, num_return=4)
    word = plain[0][0][0][0]
    got = gen.beam_search(prompts, 4, EOS, SP2, max_new_tokens=12, num_return=4, no_repeat_ngram_size=2, bad_words_ids=[[word]])
    assert got != plain
    for p, hyps in zip(prompts, got):
        assert hyps
        for h, _ in hyps:
            assert not _rules.repeats(_ids(p) + h, 2) and word not in h
    assert gen.beam_search(prompts, 4, EOS, SP2, max_new_tokens=12, num_return=4) == plain   # and off again
    for kw in (dict(no_repeat_ngram_size=9), dict(bad_words_ids=[[]]), dict(no_repeat_scope="x")):
        with pytest.raises(ValueError):
            gen.beam_search(prompts, 4, EOS, SP2, **kw)
    from ergm_amd.data import synthetic_batch
    from ergm_amd.train import Trainer
    batch = synthetic_batch(3, 16, n_turns=3, feat_dim=E, seed=40, vocab_lo=0, vocab_hi=490, sp1=SP1, sp2=SP2, eos=EOS)
    tr = Trainer(model, None)
    run = lambda **kw: tr.test([batch], top_p=0.9, eos_id=EOS, sp2_id=SP2, max_batch=4, max_len=32, num_beams=2, **kw)[0]
    hyps = run(no_repeat_ngram_size=2)
    n_in = (batch["input_ids"] != EOS).sum(1).tolist()
    for i, h in enumerate(hyps):
        assert h and not _rules.repeats(batch["input_ids"][i, :n_in[i]].tolist() + h, 2)
    assert hyps != run()
    with pytest.raises(ValueError, match="sampling"):
        tr.test([batch], top_p=0.9, eos_id=EOS, sp2_id=SP2, max_batch=4, max_len=32, no_repeat_ngram_size=2)


def _obeys(before, generated, n, s0, words=()):
    """Every generated token was allowed when it was drawn, given everything in front of it."""
    h = list(before)
    for t in generated:
        if t in _rules.banned(h, len(h), MAX_LEN, V, EOS, n, s0, words):
            return False
        h.append(t)
    return True


@pytest.mark.parametrize("engine", ["python", "native"])
def test_a_rule_may_start_in_a_later_turn(gpu, engine):
    """Turn one runs without a rule (and repeats itself), so the device keeps no history of it; a rule given with the
    second turn covers the whole sequence all the same: the generator writes the slot's earlier tokens from its own
    record.  The slot's history row is then the sequence, and every token of turn two was allowed when it was drawn."""
    _, _, model = TB._setup(gpu)
    p = _six(gpu)[3]
    gen = _gen(model, engine, max_batch=4)
    rid = gen.submit(p, 6, keep=True, sampling=GREEDY)
    t1 = gen.run(TOP_P, EOS, SP2, seed=2)[rid]
    assert _rules.repeats(t1, 2) and EOS not in t1 and int(gen.hist.abs().sum().item()) == 0
    turn = torch.tensor([t1[0], t1[1]], device=gpu)
    sp = SamplingParams(top_k=1, no_repeat_ngram_size=2, bad_words_ids=[[t1[1], t1[0]]])
    gen.extend_request(rid, turn, torch.full((2,), SP1, device=gpu), 8, sampling=sp)
    t2 = gen.run(TOP_P, EOS, SP2, seed=2)[rid]
    before = _ids(p) + t1 + turn.tolist()
    slot = gen.sched.parked[rid][0]
    kept = t2[:-1] if t2[-1] == EOS else t2
    assert gen.hist[slot, :len(before) + len(kept)].tolist() == before + kept
    assert _obeys(before, t2, 2, 0, [(t1[1], t1[0])])
    # the same turn without the rule repeats a bigram of turn one at once (what the rule had to prevent)
    ref = _gen(model, engine, max_batch=4)
    rid = ref.submit(p, 6, keep=True, sampling=GREEDY)
    assert ref.run(TOP_P, EOS, SP2, seed=2)[rid] == t1
    ref.extend_request(rid, turn, torch.full((2,), SP1, device=gpu), 8)
    plain = ref.run(TOP_P, EOS, SP2, seed=2)[rid]
    print(f"{engine}: turn one {t1}, turn two plain {plain}, ruled {t2}")
    assert not _obeys(before, plain, 2, 0, [(t1[1], t1[0])])
    # low level, outside the scheduler, the generated tokens are unknown: the late rule is refused
    low = _gen(model, engine, max_batch=4)
    low._sampling = (TOP_P, EOS, SP2, 2)
    low.admit([0], [p], [6], [0], sampling=[GREEDY])
    low.run_chunk(8)
    with pytest.raises(ValueError, match="earlier tokens"):
        low.extend([0], [(turn, torch.full((2,), SP1, device=gpu))], [8], [len(_ids(p)) + 6], sampling=[sp])
