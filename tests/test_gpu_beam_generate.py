"""Beam search in BatchedGenerator: W = 1 is greedy decoding on every engine; every round's selection is the numpy rule
(tests/_beam.py) applied to the logits and scores the generator holds; "native" is bitwise "python"; the caches follow
the beams (each row's cache is that of a fresh generator teacher-forced with the row's history); eos freezes a beam; and
the bounds are refused before anything is launched.  Model, prompts and sizes are tests/test_gpu_generate_batched.py's."""
import math

import numpy as np
import pytest
import torch

import _beam
import test_gpu_generate_batched as TB
from ergm_amd.generate import BatchedGenerator, beam_backtrack

pytestmark = pytest.mark.gpu
V, E, SP2, EOS = TB.V, TB.E, TB.SP2, TB.EOS
ENGINES = ("python", "native", "fused")
MARGIN, TOL = 1e-3, 1e-4   # as tests/test_gpu_beam_ops.py
LENS2, CAPS2 = (5, 12), (7, 12)
PROMPT_SEED = 7            # with it every round below has its margin on every engine's own logits (asserted), and a
                           # token new to both beams enters group 0's at round 1 (the eos test)


def _gen(model, engine, max_batch=8):
    return BatchedGenerator(model, max_batch=max_batch, max_len=32, engine=engine)


def _two(gpu):
    return TB._dev(TB._prompts(E, lens=LENS2, cap_lens=CAPS2, seed=PROMPT_SEED), gpu)


@pytest.mark.parametrize("engine", ENGINES)
def test_one_beam_is_greedy(gpu, engine):
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E), gpu)
    n_new = 9
    got = _gen(model, engine).beam_search(prompts, 1, EOS, SP2, max_new_tokens=n_new)
    ref = _gen(model, engine)
    logits = ref.prefill(prompts)
    B = len(prompts)
    sp2 = torch.full((B,), SP2, dtype=torch.long, device=gpu)
    toks, lps = [[] for _ in range(B)], [0.0] * B
    for i in range(n_new):
        x = logits.float().cpu().numpy().astype(np.float64)
        step = x.argmax(1)   # numpy: the lowest id among equals
        lse = x.max(1) + np.log(np.exp(x - x.max(1, keepdims=True)).sum(1))
        for b in range(B):
            if EOS not in toks[b]:
                toks[b].append(int(step[b]))
                lps[b] += x[b, step[b]] - lse[b]
        if i + 1 < n_new:
            logits = ref.step(torch.from_numpy(step).to(gpu), sp2)
    for b in range(B):
        (hyp, score), = got[b]
        assert hyp == toks[b], (engine, b)
        print(f"{engine} row {b}: {len(hyp)} tokens, |sum - fp64| {abs(score - lps[b]):.3e}")
        assert abs(score - lps[b]) <= TOL * len(hyp)


def _state(gen):
    R = gen.B
    return (gen._logits[:R, :V].float().cpu().numpy(), gen.beam_scores.cpu().numpy().copy(),
            gen.finished[:R].cpu().numpy().copy())


def _check_round(gen, W, eos, what):
    """One beam_round(1) against the rule applied to what the generator held before it.  Returns the helper's result and
    the round's (tokens, parents)."""
    logits, scores, fin = _state(gen)
    assert np.abs(logits[scores > -np.inf]).max() < 128
    ref = _beam.select(logits, scores, fin, W, eos)
    margin = min(ref["margin"])
    print(f"{what}: margin {margin:.3e}")
    assert margin >= MARGIN, what
    (tok,), (par,) = gen.beam_round(1)
    dead = np.isneginf(ref["score"])
    for g in range(gen.B // W):
        rows = [r for r in range(g * W, (g + 1) * W) if not dead[r]]
        assert {(par[r], tok[r]) for r in rows} == ref["pairs"][g], (what, g)
    assert _beam.slot_property(par, tok, W)
    assert par == ref["parent"].tolist() and tok == ref["token"].tolist()
    _, sc, fl = _state(gen)
    assert fl.tolist() == ref["finished"].tolist()
    assert np.abs(sc[~dead].astype(np.float64) - ref["score"][~dead]).max() <= TOL
    return ref, tok, par


@pytest.mark.parametrize("engine", ["python", "fused"])
def test_round_by_round(gpu, engine):
    """G = 2, W = 3, 6 rounds; engine "fused" runs them through ergm_decode_run_beams on its own logits."""
    _, _, model = TB._setup(gpu)
    gen = _gen(model, engine)
    gen.beam_prefill(_two(gpu), 3, EOS, SP2)
    assert gen.beam_scores.cpu().tolist() == [0.0, -math.inf, -math.inf] * 2
    assert gen.lens[:6].cpu().tolist() == [LENS2[0], 0, 0, LENS2[1], 0, 0]
    for i in range(6):
        _, tok, par = _check_round(gen, 3, EOS, f"{engine} round {i}")
        if i == 0:   # all children come from beam 0, and the gather fanned the prompt out
            assert par == [0, 0, 0, 3, 3, 3]
    assert gen.lens[:6].cpu().tolist() == [n + 6 for n in LENS2 for _ in range(3)]


def test_native_is_bitwise_python(gpu):
    _, _, model = TB._setup(gpu)
    prompts = _two(gpu)
    runs = []
    for engine in ("python", "native"):
        gen = _gen(model, engine)
        gen.beam_prefill(prompts, 3, EOS, SP2)
        t8, p8 = gen.beam_round(8)
        t1, p1 = gen.beam_round(1)   # behind the look of a search in chunks of 8
        runs.append((t8 + t1, p8 + p1, gen.beam_scores.cpu().numpy().tobytes(), gen.lens.cpu().tolist(),
                     gen.finished.cpu().tolist()))
    assert runs[0] == runs[1]
    # and beam_search is those rounds, backtracked
    got = _gen(model, "native").beam_search(prompts, 3, EOS, SP2, max_new_tokens=9, num_return=3)
    scores = np.frombuffer(runs[0][2], dtype=np.float32).tolist()
    assert got == beam_backtrack(runs[0][0], runs[0][1], scores, 3, EOS, 1.0, 3)


def _histories(tokens, parents, R):
    out = []
    for r in range(R):
        seq, row = [], r
        for i in range(len(tokens) - 1, -1, -1):
            seq.append(tokens[i][row])
            row = parents[i][row]
        out.append(seq[::-1])
    return out


def test_caches_follow_the_beams(gpu):
    """Engine "fused", G = 2, W = 4, 6 rounds: row g·W + w holds, bitwise and in every layer, the cache of sequence g of
    a fresh fused generator that prefilled the same two prompts and was stepped on that row's token history."""
    _, _, model = TB._setup(gpu)
    prompts = _two(gpu)
    W, n = 4, 6
    gen = _gen(model, "fused")
    gen.beam_prefill(prompts, W, EOS, SP2)
    tokens, parents = gen.beam_round(n)
    assert any(p[r] != r for p in parents[1:] for r in range(2 * W))   # beams moved rows after the fan-out
    hist = _histories(tokens, parents, 2 * W)
    lens = gen.lens[:2 * W].cpu().tolist()
    sp2 = torch.full((2,), SP2, dtype=torch.long, device=gpu)
    for w in range(W):
        fresh = _gen(model, "fused", max_batch=2)
        fresh.prefill(prompts)
        for i in range(n):
            fresh.step(torch.tensor([hist[w][i], hist[W + w][i]], device=gpu), sp2)
        for g in range(2):
            r = g * W + w
            assert LENS2[g] < lens[r] <= LENS2[g] + n
            for l in range(gen.L):
                a, b = gen.kv[l][r, :lens[r]], fresh.kv[l][g, :lens[r]]
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (r, l)


def test_eos_freezes_a_beam(gpu):
    _, _, model = TB._setup(gpu)
    prompts = _two(gpu)
    W = 3
    probe = _gen(model, "python")
    probe.beam_prefill(prompts, W, EOS, SP2)
    (t0,), _ = probe.beam_round(1)
    ref = _beam.select(*_state(probe), W, EOS)
    # a token that enters group 0's beam at round 1 and was in nobody's beam at round 0
    enters = sorted(j for r, j in ref["pairs"][0] if j not in t0)
    assert enters
    eos = enters[0]
    gen = _gen(model, "python")
    gen.beam_prefill(prompts, W, eos, SP2)
    gen.beam_round(1)
    ref1, tok1, par1 = _check_round(gen, W, eos, "eos round 1")
    rows = [r for r in range(W) if tok1[r] == eos]
    assert len(rows) == 1
    r = rows[0]
    assert gen.finished[r].item() == 1
    frozen, n_r = gen.beam_scores[r].item(), gen.lens[r].item()
    assert n_r == LENS2[0] + 1   # the eos was stepped without advancing
    toks, pars = [t0, tok1], [[0, 0, 0, 3, 3, 3], par1]
    for i in range(2, 5):
        _, tok, par = _check_round(gen, W, eos, f"eos round {i}")
        toks.append(tok), pars.append(par)
        if gen.finished[r].item() == 1 and par[r] == r and tok[r] == eos:   # still among the best W
            assert [p for p in par[:W]].count(r) == 1   # one candidate per round
            assert gen.beam_scores[r].item() == frozen and gen.lens[r].item() == n_r
        else:
            break
    else:
        hyps = beam_backtrack(toks, pars, gen.beam_scores.cpu().tolist(), W, eos, 0.0, W)[0]
        assert any(h[-1] == eos and len(h) == 2 and s == frozen for h, s in hyps)


def test_search_stops_at_the_first_look(gpu):
    """One prompt, one beam, eos = the token round 0 takes: finished at once, the search ends behind its first chunk of
    8 rounds and the hypothesis is that token."""
    _, _, model = TB._setup(gpu)
    prompt = _two(gpu)[:1]
    gen = _gen(model, "native")
    first = int(gen.beam_prefill(prompt, 1, EOS, SP2)[0].float().cpu().numpy().argmax())
    got = gen.beam_search(prompt, 1, first, SP2)
    (hyp, score), = got[0]
    assert hyp == [first] and score < 0.0
    assert gen.n_max == LENS2[0] + 8 and gen.lens[0].item() == LENS2[0]


def test_trainer_test_serves_the_loader_through_beam_search(gpu):
    """Trainer.test(num_beams=2, max_batch=4): static batches of two prompts, the best hypothesis of each; no seed
    enters, and each list is what beam_search returns for the sample's prompt in its batch."""
    from ergm_amd.data import synthetic_batch
    from ergm_amd.train import Trainer
    _, _, model = TB._setup(gpu)
    batch = synthetic_batch(3, 16, n_turns=3, feat_dim=E, seed=40, vocab_lo=0, vocab_hi=490, sp1=TB.SP1, sp2=SP2, eos=EOS)
    tr = Trainer(model, None)
    run = lambda seed: tr.test([batch], top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=seed, max_batch=4, max_len=32, num_beams=2)
    hyps, refs, emos, losses = run(3)
    assert run(4)[0] == hyps and len(hyps) == len(refs) == len(emos) == 3 and len(losses) == 1
    d = {k: v.to(gpu) for k, v in batch.items()}
    n_in = (d["input_ids"] != EOS).sum(1).tolist()
    prompts = [(d["input_ids"][i, :n], d["token_type_ids"][i, :n], d["caption_ids"][i], d["visual_feat"][i],
                d["audio_feat"][i]) for i, n in enumerate(n_in)]
    gen = _gen(model, "python", max_batch=4)
    want = [h[0][0] for h in gen.beam_search(prompts[:2], 2, EOS, SP2)] + [gen.beam_search(prompts[2:], 2, EOS, SP2)[0][0][0]]
    assert hyps == want
    for h, n in zip(hyps, n_in):
        assert 1 <= len(h) <= 32 - n and EOS not in h[:-1]
    with pytest.raises(ValueError):
        tr.test([batch], 0.9, EOS, SP2, max_batch=4, max_len=32, num_beams=5)


def test_bounds_are_refused_before_anything_is_launched(gpu):
    _, _, model = TB._setup(gpu)
    prompts = _two(gpu)
    gen = _gen(model, "native", max_batch=4)
    for kw in (dict(num_beams=3), dict(num_beams=0), dict(num_beams=9), dict(num_beams=2, max_new_tokens=32 - 12 + 1),
               dict(num_beams=2, max_new_tokens=0), dict(num_beams=2, num_return=3)):
        with pytest.raises(ValueError):
            gen.beam_search(prompts, eos_id=EOS, sp2_id=SP2, **kw)
        assert gen.B == 0 and gen._plan is None   # nothing was prefilled or bound
    with pytest.raises(ValueError):
        gen.beam_prefill(prompts, 3)
    with pytest.raises(ValueError):
        gen.beam_round(1)
    gen.beam_prefill(prompts, 2, EOS, SP2)
    with pytest.raises(ValueError):
        gen.beam_round(32 - 12 + 1)
    gen.beam_round(1)
