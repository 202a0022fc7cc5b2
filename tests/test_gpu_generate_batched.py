"""Batched KV-cache generation (ergm_amd.generate.BatchedGenerator): ragged prompts through one padded prefill and
per-token decode steps match the oracle's full-sequence forward of every sequence alone and the single-sequence
KVCacheGenerator, within the bf16 logits gate of tests/test_gpu_generate.py; a sequence's logits do not depend on its
neighbours; generate() is seeded-deterministic, stops each sequence at its eos and respects the cache bound."""
import pytest
import torch

from ergm_amd.config import ERGMConfig, NO_DROPOUT
from ergm_amd.generate import BatchedGenerator, KVCacheGenerator
from ergm_amd.model import GPT2LMHeadModel
from oracle import gpt2_oracle as O

pytestmark = pytest.mark.gpu
V, E, LYR, H, P = 500, 128, 2, 2, 64
LOGIT_ATOL = 0.06   # the gate of tests/test_gpu_generate.py
SP1, SP2, EOS = 498, 499, 497
LENS, CAP_LENS = (5, 12, 13), (7, 12, 3)


def _setup(gpu, feat_dim=None, seed=11):
    ocfg = O.OracleConfig(vocab_size=V, n_embd=E, n_layer=LYR, n_head=H, n_positions=P, feat_dim=feat_dim)
    P0 = O.init_params(ocfg, seed=seed)
    model = GPT2LMHeadModel(ERGMConfig(vocab_size=V, n_embd=E, n_layer=LYR, n_head=H, n_positions=P,
                                       feat_dim=feat_dim, **NO_DROPOUT), device=gpu)
    model.load_state_dict(P0, strict=True)
    return ocfg, P0, model


def _prompts(Fd, lens=LENS, cap_lens=CAP_LENS, with_feat=1, seed=4):
    """CPU prompts (ids, types, captions, vis, aud); only sequence `with_feat` carries visual / audio vectors."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b, (n, nc) in enumerate(zip(lens, cap_lens)):
        ids = torch.randint(0, 490, (1, n), generator=g)
        tt = torch.full((1, n), SP1)
        tt[:, n // 2:] = SP2
        cap = torch.randint(0, 490, (1, nc), generator=g)
        vis = aud = None
        if b == with_feat:
            vis, aud = 0.1 * torch.randn(1, Fd, generator=g), 0.1 * torch.randn(1, Fd, generator=g)
        out.append((ids, tt, cap, vis, aud))
    return out


def _dev(prompts, gpu):
    return [tuple(None if t is None else t.to(gpu) for t in p) for p in prompts]


def _oracle_logits(P0, ocfg, seq, types, p):
    return O.forward(P0, ocfg, input_ids=seq, token_type_ids=types, caption_ids=p[2], visual_feat=p[3],
                     audio_feat=p[4])["logits"][0, -1]


@pytest.mark.parametrize("feat_dim", [None, 64])
def test_batched_steps_match_oracle_and_single_generator(gpu, feat_dim):
    """Prefill and 6 teacher-forced steps of three ragged sequences (prompt lengths 5 / 12 / 13, captions 7 / 12 / 3,
    sequence 1 with visual / audio vectors; feat_dim = 64: through the config-5 projections) against the oracle on
    each sequence alone and against KVCacheGenerator on each sequence alone.  The forced tokens differ per sequence."""
    ocfg, P0, model = _setup(gpu, feat_dim)
    prompts = _prompts(feat_dim or E)
    dprompts = _dev(prompts, gpu)
    B = len(prompts)
    forced = torch.randint(0, 490, (6, B), generator=torch.Generator().manual_seed(9))
    assert all(len(set(forced[t].tolist())) == B for t in range(6))
    sp2 = torch.full((B,), SP2, dtype=torch.long, device=gpu)
    gen = BatchedGenerator(model, max_batch=4, max_len=32)
    got = [gen.prefill(dprompts).float().cpu()]
    for t in range(6):
        got.append(gen.step(forced[t].to(gpu), sp2).float().cpu())
    assert gen.lens[:B].cpu().tolist() == [n + 6 for n in LENS]
    worst_o = worst_s = 0.0
    for b, p in enumerate(prompts):
        single = KVCacheGenerator(model, max_len=32)
        seq, types = p[0], p[1]
        lg = single.prefill(*dprompts[b])
        for t in range(7):
            ref = _oracle_logits(P0, ocfg, seq, types, p)
            d_o = (got[t][b] - ref).abs().max().item()
            d_s = (got[t][b] - lg.float().cpu()).abs().max().item()
            worst_o, worst_s = max(worst_o, d_o), max(worst_s, d_s)
            assert d_o <= LOGIT_ATOL, (b, t, d_o)
            assert d_s <= LOGIT_ATOL, (b, t, d_s)
            if t == 6:
                break
            tok = forced[t, b].view(1, 1)
            seq = torch.cat([seq, tok], 1)
            types = torch.cat([types, torch.full((1, 1), SP2)], 1)
            lg = single.step(tok.to(gpu), torch.full((1, 1), SP2, device=gpu))
    print(f"feat_dim {feat_dim}: max |logits - oracle| {worst_o:.4f}, max |logits - KVCacheGenerator| {worst_s:.4f}")


def test_batch_of_one_greedy_matches_single_generator(gpu):
    _, _, model = _setup(gpu)
    p = _dev(_prompts(E, lens=(12,), cap_lens=(9,), with_feat=0), gpu)
    single, batched = KVCacheGenerator(model, max_len=32), BatchedGenerator(model, max_batch=1, max_len=32)
    la, lb = single.prefill(*p[0]), batched.prefill(p)
    a, b = [], []
    for _ in range(8):
        ta, tb = int(la.argmax()), int(lb[0].argmax())
        a.append(ta)
        b.append(tb)
        la = single.step(torch.tensor([[ta]], device=gpu), torch.full((1, 1), SP2, device=gpu))
        lb = batched.step(torch.tensor([tb], device=gpu), torch.tensor([SP2], device=gpu))
    assert a == b


def test_padding_isolation(gpu):
    """Prompt A (length 6, caption 5) in slot 0 beside a long and then a short neighbour; a third sequence of length
    13 with a 12-token caption pins the padded batch shape to B = 3, S = 13, Sc = 12 in both runs.  A's logits, at
    prefill and after 3 steps, are bitwise the same."""
    _, _, model = _setup(gpu)
    A, pin = _prompts(E, lens=(6, 13), cap_lens=(5, 12), with_feat=0, seed=21)
    long_n, = _prompts(E, lens=(12,), cap_lens=(11,), with_feat=-1, seed=22)
    short_n, = _prompts(E, lens=(2,), cap_lens=(1,), with_feat=-1, seed=23)
    sp2 = torch.full((3,), SP2, dtype=torch.long, device=gpu)
    runs = []
    for k, nb in enumerate((long_n, short_n)):
        gen = BatchedGenerator(model, max_batch=3, max_len=32)
        logits = [gen.prefill(_dev([A, nb, pin], gpu))[0].clone()]
        for t in range(3):
            toks = torch.tensor([40 + t, 100 + 50 * k + t, 7 + t], device=gpu)   # the neighbour's tokens differ too
            logits.append(gen.step(toks, sp2)[0].clone())
        runs.append(torch.stack(logits).cpu())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))


def test_generate_deterministic_bounded_and_stops_per_sequence(gpu):
    """Seeded generate() repeats; tokens lie in [0, V); each list ends at its first eos or at the bound.  Sequence 0
    is made to finish at once: the position embedding of its last prompt position (4; an inner position of the other
    two prompts) is a large multiple of the eos direction, which then dominates that row of the residual stream, and
    the eos row of the tied LM head has norm 2, so ln_f · wteᵀ puts nearly all probability on eos there (logit
    about sqrt(E) · 2 = 23 against |logits| of a few).  It then emits nothing more while the others go on."""
    _, P0, model = _setup(gpu)
    wte, wpe = P0["transformer.wte.weight"].clone(), P0["transformer.wpe.weight"].clone()
    d = wte[EOS] / wte[EOS].norm()
    wte[EOS], wpe[LENS[0] - 1] = 2.0 * d, 40.0 * d
    model.load_state_dict({**P0, "transformer.wte.weight": wte, "transformer.wpe.weight": wpe}, strict=True)
    dprompts = _dev(_prompts(E, with_feat=-1), gpu)
    gen = BatchedGenerator(model, max_batch=3, max_len=32)
    bound = 32 - max(LENS)
    runs = [gen.generate(dprompts, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7) for _ in range(2)]
    assert runs[0] == runs[1]
    other = gen.generate(dprompts, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=8)
    print("generate:", [len(r) for r in runs[0]], [len(r) for r in other])
    for out in (runs[0], other):
        assert len(out) == 3
        for r in out:
            assert 1 <= len(r) <= bound and all(0 <= t < V for t in r)
            assert EOS not in r[:-1] and (r[-1] == EOS or len(r) == bound)
    assert runs[0][0] == [EOS]                       # finished at its first token ...
    assert max(len(r) for r in runs[0][1:]) > 1      # ... while the others continued
    assert other[1:] != runs[0][1:]                  # another seed, another continuation
    short = gen.generate(dprompts, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7, max_new_tokens=5)
    assert [r[:5] for r in runs[0]] == short
    with pytest.raises(ValueError):
        gen.generate(dprompts, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7, max_new_tokens=bound + 1)
