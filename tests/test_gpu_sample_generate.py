"""Per-request sampling controls in ContinuousGenerator(controls=True): without any the lists are those of the old
path on every engine; "native" is bitwise "python" with mixed parameters, log-probabilities included; a request's
result does not depend on what it runs beside or on the slot's previous tenant; the first token of every request is
the fp64 rule (tests/_sample.py) applied to the slot's logits; the minimum length holds eos back on the device, per
turn in a session; and a session's bitmap covers everything its cache holds.  Model, prompts and sizes are
tests/test_gpu_generate_batched.py's and tests/test_gpu_continuous.py's."""
import numpy as np
import pytest
import torch

import _sample
import test_gpu_generate_batched as TB
from ergm_amd.generate import ContinuousGenerator, SamplingParams

pytestmark = pytest.mark.gpu
V, E, SP1, SP2, EOS = TB.V, TB.E, TB.SP1, TB.SP2, TB.EOS
NO_EOS = -1
ENGINES = ("python", "native", "fused")
LENS6, CAPS6 = (5, 12, 13, 7, 9, 4), (7, 12, 3, 5, 8, 6)
TOP_P = 0.9
# six requests, no two alike; the cuts of those with top_p < 1 lie well inside the renormalised top-k set
MIXED = [
    SamplingParams(top_k=3, top_p=0.5, logprobs=True),
    SamplingParams(top_k=1),
    SamplingParams(temperature=0.7, repetition_penalty=1.3, top_p=1.0, logprobs=True),
    SamplingParams(top_k=5, top_p=1.0, repetition_penalty=1.5, min_new_tokens=2),
    SamplingParams(top_k=8, temperature=1.5, top_p=1.0, logprobs=True),
    SamplingParams(top_k=2, top_p=0.3, temperature=0.5),
]
FIRST_SEED = 1   # with it every request of MIXED has a first-draw gap >= 1e-4 on its slot's logits (asserted below)


def _gen(model, engine, controls=True, **kw):
    return ContinuousGenerator(model, max_batch=4, max_len=32, cap_max=16, engine=engine, controls=controls, **kw)


def _six(gpu):
    return TB._dev(TB._prompts(E, lens=LENS6, cap_lens=CAPS6), gpu)


@pytest.mark.parametrize("engine", ENGINES)
def test_no_sampling_is_the_old_path(gpu, engine):
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    old = _gen(model, engine, controls=False).generate(prompts, TOP_P, EOS, SP2, seed=7, max_new_tokens=10)
    new = _gen(model, engine).generate(prompts, TOP_P, EOS, SP2, seed=7, max_new_tokens=10)
    assert new == old
    off = _gen(model, engine, controls=False)
    with pytest.raises(ValueError, match="controls=True"):
        off.submit(prompts[0], sampling=SamplingParams(top_k=3))
    with pytest.raises(ValueError, match="controls=True"):
        off.admit([0], prompts[:1], sampling=[SamplingParams()])
    assert not off.sched.queue


def _run_mixed(model, engine, prompts, **kw):
    gen = _gen(model, engine, **kw)
    ids = [gen.submit(p, 9, sampling=sp) for p, sp in zip(prompts, MIXED)]
    out = gen.run(TOP_P, EOS, SP2, seed=5)
    return [out[i] for i in ids], gen.token_logprobs, gen


def test_python_and_native_agree(gpu):
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    py, py_lp, _ = _run_mixed(model, "python", prompts)
    nat, nat_lp, gen = _run_mixed(model, "native", prompts)
    assert nat == py
    assert sorted(py_lp) == sorted(nat_lp) == [i for i, sp in enumerate(MIXED) if sp.logprobs]
    for i, lp in py_lp.items():
        assert len(lp) == len(py[i]) and all(x <= 0.0 for x in lp)
        assert np.array(lp, dtype=np.float32).tobytes() == np.array(nat_lp[i], dtype=np.float32).tobytes()
    assert len(gen.sched.admissions) >= 2   # six requests over four slots: slots were reused


def test_results_do_not_depend_on_the_schedule(gpu):
    """Engine "fused", max_admit = 1: each of the six requests returns the same list (and log-probabilities) alone as
    among the others.  The solo runs share one generator, so every slot is reused behind a tenant with other values."""
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    together, lp, _ = _run_mixed(model, "fused", prompts, max_admit=1)
    solo = _gen(model, "fused", max_admit=1)
    for i in (5, 0, 3, 1, 4, 2):
        rid = solo.submit(prompts[i], 9, request_id=i, sampling=MIXED[i])
        assert solo.run(TOP_P, EOS, SP2, seed=5)[rid] == together[i], i
        if MIXED[i].logprobs:
            assert solo.token_logprobs[i] == lp[i]
    assert len(set(s for call in solo.sched.admissions for _, s in call)) == 4   # the slots took turns


@pytest.mark.parametrize("engine", ["python", "fused"])
def test_first_token_is_the_rule_on_the_slots_logits(gpu, engine):
    _, _, model = TB._setup(gpu)
    prompts = _six(gpu)
    gen = _gen(model, engine)
    gen._sampling = (TOP_P, NO_EOS, SP2, FIRST_SEED)
    for half, slots in ((range(0, 4), (2, 0, 3, 1)), (range(4, 6), (1, 3))):
        half = list(half)
        gen.finished.fill_(1)
        gen.admit(slots, [prompts[i] for i in half], request_ids=[10 + i for i in half], sampling=[MIXED[i] for i in half])
        logits = gen.logits.float().cpu().numpy()
        tokens, _ = gen.run_chunk(1)
        for i, s in zip(half, slots):
            sp = MIXED[i]
            top_p = TOP_P if sp.top_p is None else sp.top_p
            proc = dict(seen=prompts[i][0].reshape(-1).tolist(), rep=sp.repetition_penalty, temp=sp.temperature)
            if top_p < 1.0:
                lo, hi = _sample.cut_margin(logits[s], top_p, sp.top_k, **proc)
                assert lo >= 0.008 and hi >= 0.008 and lo + hi >= 0.02, (i, lo, hi)
            tok, gap, kept, _ = _sample.draw(logits[s], top_p, _sample.uniform(FIRST_SEED, 10 + i, 0), sp.top_k, **proc)
            print(f"request {i} slot {s}: token {tokens[0][s]} (helper {tok}), gap {gap:.2e}, kept {kept.size}")
            assert gap >= 1e-4, (i, gap)
            assert tokens[0][s] == tok, (i, tokens[0][s], tok)


@pytest.mark.parametrize("engine", ["python", "native"])
def test_minimum_length_in_the_generator(gpu, engine):
    _, _, model = TB._setup(gpu)
    p = _six(gpu)[2]
    greedy = SamplingParams(top_k=1)
    first = _gen(model, engine).generate([p], TOP_P, NO_EOS, SP2, seed=3, max_new_tokens=1, sampling=greedy)[0]
    eos = first[0]
    assert _gen(model, engine).generate([p], TOP_P, eos, SP2, seed=3, max_new_tokens=6, sampling=greedy) == [[eos]]
    gen = _gen(model, engine)
    out = gen.generate([p], TOP_P, eos, SP2, seed=3, max_new_tokens=6, sampling=SamplingParams(top_k=1, min_new_tokens=3))[0]
    print(f"{engine}: eos {eos}, with min_new_tokens=3: {out}")
    assert len(out) >= 3 and eos not in out[:2]
    assert eos not in out[:3]   # eos is held back while fewer than 3 tokens of the turn exist
    assert gen.finished.cpu().tolist() == [1, 1, 1, 1]   # the device agrees (the scheduler checked it at every look)
    assert gen.min_step.cpu().tolist()[gen.sched.admissions[0][0][1]] == 3
    with pytest.raises(ValueError, match="min_new_tokens"):
        gen.submit(p, 2, sampling=SamplingParams(min_new_tokens=3))


def _bits(gen, slot):
    row = gen.seen[slot].cpu().numpy().view(np.uint32)
    return sorted(int(w) * 32 + b for w in np.flatnonzero(row) for b in range(32) if (row[w] >> np.uint32(b)) & 1)


@pytest.mark.parametrize("engine", ["python", "native"])
def test_sessions_keep_their_bitmap_and_count_the_minimum_per_turn(gpu, engine):
    _, _, model = TB._setup(gpu)
    p = _six(gpu)[3]
    turn = torch.tensor([17, 301, 17, 44], device=gpu)
    tt = torch.full((4,), SP1, device=gpu)
    sp1 = SamplingParams(repetition_penalty=1.3, top_k=4, logprobs=True)

    def two_turns(eos2, sp2, max_new2):
        gen = _gen(model, engine)
        rid = gen.submit(p, 4, keep=True, sampling=sp1)
        t1 = gen.run(TOP_P, NO_EOS, SP2, seed=2)[rid]
        slot = gen.sched.parked[rid][0]
        assert _bits(gen, slot) == sorted(set(p[0].reshape(-1).tolist()) | set(t1))
        gen.extend_request(rid, turn, tt, max_new2, sampling=sp2)
        t2 = gen.run(TOP_P, eos2, SP2, seed=2)[rid]
        return gen, slot, t1, t2

    # what the second turn draws first, greedily and with eos out of the way
    gen, slot, t1, t2 = two_turns(NO_EOS, SamplingParams(top_k=1), 1)
    assert len(t1) == 4 and len(gen.token_logprobs[0]) == 4   # the first turn's: the second asked for none
    eos = t2[0]
    gen, slot, t1b, t2 = two_turns(eos, SamplingParams(top_k=1), 5)
    assert t1b == t1 and t2 == [eos]
    # the first turn left row_steps at 4: a minimum of 2 counts from the turn's first token, not from the admission's
    gen, slot, t1c, t2 = two_turns(eos, SamplingParams(top_k=1, min_new_tokens=2), 5)
    print(f"{engine}: turn 1 {t1c}, eos {eos}, turn 2 with min_new_tokens=2: {t2}")
    assert t1c == t1 and len(t2) >= 2 and eos not in t2[:2]
    assert gen.min_step.cpu().tolist()[slot] == 4 + 2
    assert _bits(gen, slot) == sorted(set(p[0].reshape(-1).tolist()) | set(t1) | set(turn.tolist()) | set(t2))
    # None keeps the session's values, without a minimum
    gen, slot, _, t2 = two_turns(NO_EOS, None, 3)
    assert gen._slot_sp[slot] == SamplingParams(repetition_penalty=1.3, top_k=4, logprobs=True) and len(t2) == 3
    assert len(gen.token_logprobs[0]) == 3 and gen.min_step.cpu().tolist()[slot] == 4


def test_trainer_test_passes_sampling_through(gpu):
    """Trainer.test(sampling=...) serves every sample with that value: greedy hypotheses do not depend on the seed,
    sampled ones do here, and each respects its bound and its minimum length."""
    from ergm_amd.data import synthetic_batch
    from ergm_amd.train import Trainer
    _, _, model = TB._setup(gpu)
    batch = synthetic_batch(3, 16, n_turns=3, feat_dim=E, seed=40, vocab_lo=0, vocab_hi=490, sp1=SP1, sp2=SP2, eos=EOS)
    tr = Trainer(model, None)
    run = lambda seed, sp: tr.test([batch], top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=seed, max_batch=2, max_len=32, sampling=sp)[0]
    greedy = SamplingParams(top_k=1, min_new_tokens=2)
    a, b = run(3, greedy), run(4, greedy)
    assert a == b and len(a) == 3
    for h in a:
        assert 2 <= len(h) < 32 and EOS not in h[:2] and EOS not in h[:-1]
    assert run(3, None) != run(4, None)   # the plain path draws by the seed
