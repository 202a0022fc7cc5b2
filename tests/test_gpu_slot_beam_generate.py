"""Beam search on the continuous batcher's slots (ContinuousGenerator(num_beams=W)): one request alone in one group is
BatchedGenerator.beam_search, bitwise; the executor's rounds (ergm_decode_run_slot_beams behind ergm_decode_admit and
ergm_beam_seed) are bitwise the Python yardstick in every cache, length, flag, score, token and parent; a request's
hypotheses do not depend on the schedule; groups end at eos or at their bound on the device and are served again; and
Trainer.test(beam_batching="continuous").  Model, prompts and helpers are tests/test_gpu_generate_batched.py's and
tests/test_gpu_continuous.py's.  Every comparison is of integers or of float bits."""
import math

import pytest
import torch

import test_gpu_continuous as TC
import test_gpu_generate_batched as TB
from ergm_amd.data import synthetic_batch
from ergm_amd.generate import BatchedGenerator, ContinuousGenerator
from ergm_amd.train import Trainer

pytestmark = pytest.mark.gpu
V, E, SP1, SP2, EOS = TB.V, TB.E, TB.SP1, TB.SP2, TB.EOS
SENT = TC.SENT


def _gen(model, engine, W, max_batch, **kw):
    return TC._gen(model, engine, max_batch=max_batch, num_beams=W, **kw)


def _bits(hyps):
    """Hypotheses with their scores as float bits: equality below is bitwise."""
    return [(tuple(h), torch.tensor(s, dtype=torch.float32).view(torch.int32).item()) for h, s in hyps]


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("engine", ["python", "native"])
def test_one_group_is_the_static_search(gpu, engine, W):
    """One request alone in ContinuousGenerator(max_batch=W, num_beams=W) against BatchedGenerator(max_batch=W)
    .beam_search([prompt], W), all W hypotheses and their scores, max_new_tokens 1, 8 and 9 (below, at and above one
    8-round look), plain and with no_repeat_ngram_size=2.  The two paths issue the same kernels with the same arguments
    (tests/test_gpu_continuous.py::test_one_slot_returns_the_static_generators_list has the argument); the decode
    cross-attention's row bound is cap_max (16) where the static path gives the caption length (9), which only clamps."""
    _, _, model = TB._setup(gpu)
    p = TB._dev(TB._prompts(E, lens=(12,), cap_lens=(9,), with_feat=0), gpu)
    for rules in ({}, dict(no_repeat_ngram_size=2)):
        for k in (1, 8, 9):
            want = BatchedGenerator(model, max_batch=W, max_len=32, engine=engine).beam_search(
                p, W, EOS, SP2, max_new_tokens=k, num_return=W, **rules)[0]
            gen = ContinuousGenerator(model, max_batch=W, max_len=32, cap_max=16, engine=engine, num_beams=W)
            rid = gen.submit(p[0], k, request_id=0, **rules)
            got = gen.run_beams(EOS, SP2, num_return=W)
            assert list(got) == [rid] and _bits(got[rid]) == _bits(want), (rules, k)
            assert len(want) == W and all(len(h) == k or h[-1] == EOS for h, _ in want)
            assert gen.sched.steps == 8 * ((k + 7) // 8) and gen.seed_calls == 1


GROUPS = (2, 0, 3)   # out of order; group 1 stays idle


def _state(gen):
    st = TC._state(gen)
    st["ints"]["beam_scores"] = gen.beam_scores.clone().cpu().view(torch.int32)
    return st


def test_native_is_bitwise_the_python_rounds(gpu):
    """Three ragged prompts into groups (2, 0, 3) of a 4-group generator of W = 2, then 6 rounds one at a time: after the
    seed and after every round the logits, every layer's whole kv and xkv, lens, cap_lens, stop_lens, finished, the
    scores, and the round's tokens and parents are the same bits on "python" and "native".  The idle group's caches keep
    the sentinel, except the row the step appends behind its length 0."""
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E), gpu)
    W = 2
    traces = []
    for engine in ("python", "native"):
        gen = _gen(model, engine, W, 4 * W)
        gen.admit_beams(GROUPS, prompts, max_new_tokens=(4, 9, 12))
        states, rounds = [_state(gen)], []
        for _ in range(6):
            rounds.append(gen.beam_round(1, EOS, SP2))
            states.append(_state(gen))
        traces.append((states, rounds))
    (sa, ra), (sb, rb) = traces
    for i, (a, b) in enumerate(zip(sa, sb)):
        TC._same(a, b, "after the seed" if i == 0 else f"after round {i - 1}")
    assert ra == rb
    seed = sa[0]["ints"]
    for g, n, c, k in zip(GROUPS, TB.LENS, TB.CAP_LENS, (4, 9, 12)):
        r0 = g * W
        assert seed["lens"][r0:r0 + W].tolist() == [n, 0] and seed["cap_lens"][r0:r0 + W].tolist() == [c, c]
        assert seed["stop_lens"][r0:r0 + W].tolist() == [n + k, n + k] and seed["finished"][r0:r0 + W].tolist() == [0, 0]
        assert gen.beam_scores[r0:r0 + W].cpu().tolist() != [0.0, -math.inf]   # the rounds moved them
        assert seed["beam_scores"][r0:r0 + W].view(torch.float32).tolist() == [0.0, -math.inf]
        for l in range(gen.L):   # the captions reached the group's second row
            x = sa[0]["xkv"][l]
            assert torch.equal(x[r0 + 1, :c].view(torch.int16), x[r0, :c].view(torch.int16))
            assert bool((x[r0 + 1, c:].view(torch.int16) == torch.tensor(SENT).bfloat16().view(torch.int16)).all())
    (tok0, par0), = [(t[0], p[0]) for t, p in ra[:1]]
    for g in GROUPS:
        assert par0[g * W:g * W + W] == [g * W] * W          # round 0: every child comes from the prompt's row
    last = sa[-1]
    sent = torch.tensor(SENT).bfloat16().view(torch.int16)
    for l in range(gen.L):
        assert bool((last["kv"][l][W:2 * W, 1:].view(torch.int16) == sent).all())
        assert bool((last["xkv"][l][W:2 * W].view(torch.int16) == sent).all())
    assert last["ints"]["lens"][W:2 * W].tolist() == [0, 0] and last["ints"]["finished"][W:2 * W].tolist() == [1, 1]
    # the request of 4 tokens was finished by the device at its bound: rounds 4 and 5 changed nothing of it
    r0 = GROUPS[0] * W
    assert last["ints"]["finished"][r0:r0 + W].tolist() == [1, 1]
    assert last["ints"]["lens"][r0:r0 + W].tolist() == [TB.LENS[0] + 4] * W
    assert torch.equal(sa[4]["ints"]["beam_scores"][r0:r0 + W], last["ints"]["beam_scores"][r0:r0 + W])
    assert all(ra[i][1][0][r0:r0 + W] == [r0, r0 + 1] for i in (4, 5))


REQ_LENS, REQ_CAPS, REQ_NEW = TC.REQ_LENS, TC.REQ_CAPS, TC.REQ_NEW


def test_results_do_not_depend_on_the_schedule(gpu):
    """Engine "fused", max_admit = 1, W = 2 on 8 slots: seven requests with bounds (1, 9, 3, 17, 2, 8, 5) share four
    groups; every request's W hypotheses and scores are bitwise what it gets alone in a fresh generator, a second run on
    the used generator repeats the first, and groups are reused.  The odd requests carry no_repeat_ngram_size=2, so ruled
    and plain groups run side by side and a plain request follows a ruled one into its group, inheriting nothing."""
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E, lens=REQ_LENS, cap_lens=REQ_CAPS, with_feat=1, seed=31), gpu)
    W = 2
    rules = [dict(no_repeat_ngram_size=2) if i % 2 else {} for i in range(7)]
    gen = _gen(model, "fused", W, 8, max_admit=1)
    runs = []
    for _ in range(2):
        for i, (p, k) in enumerate(zip(prompts, REQ_NEW)):
            assert gen.submit(p, k, request_id=i, **rules[i]) == i
        runs.append({i: _bits(h) for i, h in gen.run_beams(EOS, SP2, num_return=W).items()})
    assert runs[0] == runs[1] and sorted(runs[0]) == list(range(7))
    adm = gen.sched.admissions
    assert all(len(call) == 1 for call in adm) and len(adm) == 14 and gen.seed_calls == 14
    group_of = {i: g for call in adm[:7] for i, g in call}
    assert [group_of[i] for i in range(4)] == [0, 1, 2, 3] and len(set(group_of.values())) == 4   # groups serve again
    for i, k in enumerate(REQ_NEW):
        for h, _ in runs[0][i]:
            assert len(h) == k or (len(h) < k and h[-1] == EOS), (i, h)
        alone = _gen(model, "fused", W, 8, max_admit=1)
        alone.submit(prompts[i], k, request_id=i, **rules[i])
        if rules[i]:   # no 2-gram twice in the prompt and the hypothesis together
            for h, _ in runs[0][i]:
                seq = prompts[i][0].reshape(-1).tolist() + [t for t in h if t != EOS]
                grams = list(zip(seq, seq[1:]))[REQ_LENS[i] - 1:]
                assert len(set(grams)) == len(grams) and not set(grams) & set(zip(seq[:REQ_LENS[i]], seq[1:REQ_LENS[i]])), (i, h)
        assert {j: _bits(h) for j, h in alone.run_beams(EOS, SP2, num_return=W).items()} == {i: runs[0][i]}, i


def test_eos_and_the_bound_end_a_group_on_the_device(gpu):
    """tests/test_gpu_beam_generate.py's construction (eos = the token round 0 takes): with one beam per group, request
    0 is finished by its first select, its group is free at the first look and serves request 2 while request 1 (12
    tokens) runs on beside it.  Then W = 2 with an eos no beam takes: a request that ends at its bound returns
    hypotheses of exactly max_new_tokens tokens, with none of the eos the chunk's later rounds produced."""
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E), gpu)
    probe = _gen(model, "native", 1, 2)
    probe.admit_beams((0, 1), prompts[:2])
    first = probe.logits[:2].float().cpu().argmax(1).tolist()
    assert first[0] != first[1]
    eos = first[0]
    gen = _gen(model, "native", 1, 2)
    looks = []
    chunk = gen.run_beam_chunk

    def watched(n):
        r = chunk(n)
        looks.append((gen.lens.cpu().tolist(), gen.stop_lens.cpu().tolist(), gen.finished.cpu().tolist(),
                      [None if q is None else q.id for q in gen.sched.live]))
        return r

    gen.run_beam_chunk = watched
    ids = [gen.submit(p, k) for p, k in zip((prompts[0], prompts[1], prompts[2]), (10, 12, 3))]
    out = gen.run_beams(eos, SP2)
    assert ids == [0, 1, 2] and sorted(out) == ids
    (h0, s0), = out[0]
    assert h0 == [eos] and s0 < 0.0
    assert gen.sched.admissions == [[(0, 0), (1, 1)], [(2, 0)]]       # group 0 again, at the first look
    lens, stops, fin, live = looks[0]
    assert fin == [1, 0] and lens[0] == TB.LENS[0] and live == [0, 1]   # eos at the first select: nothing advanced
    lens, stops, fin, live = looks[1]
    assert live == [2, 1] and fin == [1, 1]                           # 3 and 12 rounds: both inside the second chunk
    for lens, stops, fin, live in looks:
        assert all(n <= s for n, s in zip(lens, stops))
    (h1, _), = out[1]
    (h2, _), = out[2]
    assert (len(h1) == 12 or h1[-1] == eos) and eos not in h1[:-1] and len(h1) > 1
    assert (len(h2) == 3 or h2[-1] == eos) and eos not in h2[:-1]
    assert len(looks) == 2 and gen.sched.steps == 16
    # the bound alone: an eos far from every beam
    W = 2
    low = int(probe.logits[0].float().cpu().argmin())
    gen = _gen(model, "native", W, 2 * W)
    got = gen.beam_search(prompts[:2], low, SP2, max_new_tokens=[3, 9], num_return=W)
    for hyps, k in zip(got, (3, 9)):
        assert len(hyps) == W
        for h, s in hyps:
            assert len(h) == k and low not in h and math.isfinite(s) and s < 0.0
    assert gen.sched.steps == 16 and gen.finished.cpu().tolist() == [1] * (2 * W)
    assert gen.lens.cpu().tolist() == [TB.LENS[0] + 3] * W + [TB.LENS[1] + 9] * W == gen.stop_lens.cpu().tolist()


def _loader():
    """The 5-sample loader of tests/test_gpu_continuous.py::test_trainer_test."""
    S, pads = 16, (3, 0, 7, 5, 1)
    batches = []
    for k, B in enumerate((3, 2)):
        b = synthetic_batch(B, S, n_turns=3, feat_dim=E, seed=40 + k, vocab_lo=0, vocab_hi=490, sp1=SP1, sp2=SP2, eos=EOS)
        for i in range(B):
            pad = pads[3 * k + i]
            if pad:
                b["input_ids"][i, S - pad:] = EOS
                b["token_type_ids"][i, S - pad:] = EOS
        batches.append(b)
    return batches, [S - p for p in pads]


def test_trainer_test_continuous_beams(gpu):
    """Trainer.test(num_beams=2, beam_batching="continuous"): one hypothesis per sample in loader order, repeated by a
    second call.  With max_batch = 2 both ways serve one sample at a time (no static batch pads, one group), through the
    same kernels at the same row counts: each hypothesis is the static path's.  The default is the static path."""
    _, _, model = TB._setup(gpu)
    batches, n_in = _loader()
    tr = Trainer(model, None)
    kw = dict(top_p=0.9, eos_id=EOS, sp2_id=SP2, max_len=32, num_beams=2)
    cont = tr.test(batches, max_batch=4, beam_batching="continuous", **kw)
    assert tr.test(batches, max_batch=4, seed=9, beam_batching="continuous", **kw) == cont
    hyps, refs, emos, losses = cont
    assert len(hyps) == len(refs) == len(emos) == 5 and len(losses) == 2
    for h, n in zip(hyps, n_in):
        assert 1 <= len(h) <= 32 - n and EOS not in h[:-1] and (h[-1] == EOS or len(h) == 32 - n)
    static = tr.test(batches, max_batch=2, **kw)
    assert tr.test(batches, max_batch=2, beam_batching="static", **kw) == static
    one = tr.test(batches, max_batch=2, beam_batching="continuous", **kw)
    assert one[0] == static[0] and one[1:] == static[1:] and one[1:] == cont[1:]
    with pytest.raises(ValueError):
        tr.test(batches, max_batch=2, beam_batching="paged", **kw)
    with pytest.raises(ValueError):
        tr.test(batches, 0.9, EOS, SP2, max_batch=2, max_len=32, beam_batching="continuous")   # no num_beams


def test_refusals(gpu):
    _, _, model = TB._setup(gpu)
    p = TB._dev(TB._prompts(E), gpu)
    new = lambda **kw: ContinuousGenerator(model, max_batch=4, max_len=32, cap_max=16, **kw)
    for kw in (dict(num_beams=3), dict(num_beams=0), dict(num_beams=9), dict(num_beams=True), dict(num_beams=2, controls=True)):
        with pytest.raises(ValueError):
            new(**kw)
    gen = new(num_beams=2, engine="native")
    gen.submit(p[0], 3)
    sp2 = torch.full((4,), SP2, dtype=torch.long, device=gpu)
    for call in (lambda: gen.run(0.9, EOS, SP2), lambda: gen.generate(p[:1], 0.9, EOS, SP2), lambda: gen.submit(p[0], 3, keep=True),
                 lambda: gen.extend_request(0, p[0][0], p[0][1]), lambda: list(gen.drain(0.9, EOS, SP2)),
                 lambda: gen.run_chunk(8), lambda: gen.submit(p[0], 3, no_repeat_ngram_size=9),
                 lambda: gen.run_beams(V, SP2), lambda: gen.run_beams(EOS, SP2, num_return=3),
                 lambda: gen.admit_beams((0, 2), p[:2]), lambda: gen.admit_beams((0, 0), p[:2])):
        with pytest.raises(ValueError):
            call()
    assert gen.admit_calls == 0 and gen.seed_calls == 0            # nothing reached the device
    (hyp, score), = gen.run_beams(EOS, SP2)[0]                       # and the queued request is served
    assert 1 <= len(hyp) <= 3
    assert len(gen.score(p[:1])[0].logprobs) == TB.LENS[0] - 1       # scoring touches no slot and works as before
    plain = new()
    for call in (lambda: plain.run_beams(EOS, SP2), lambda: plain.beam_round(1, EOS, SP2), lambda: plain.admit_beams((0,), p[:1]),
                 lambda: plain.submit(p[0], 3, no_repeat_ngram_size=2)):
        with pytest.raises(ValueError):
            call()
