"""The native decode executor behind BatchedGenerator(engine=...): engine "native" (the existing kernels, launch for
launch) is bitwise the Python path in every buffer it writes and returns the same generate() lists; engine "fused"
(ergm_linear_rows) meets the logits gate of tests/test_gpu_generate_batched.py against the oracle and
KVCacheGenerator, keeps a sequence's logits independent of its neighbours, generates deterministically, and both
refuse a step past the cache before anything is launched.  Model, prompts and helpers are that file's."""
import pytest
import torch

import test_gpu_generate_batched as TB
from ergm_amd.generate import BatchedGenerator, KVCacheGenerator

pytestmark = pytest.mark.gpu
V, E, SP2, EOS, LENS = TB.V, TB.E, TB.SP2, TB.EOS, TB.LENS
SENT = -12288.0   # exact in bf16
FUSED = ("fused",)


def _gen(model, engine, max_batch=4, max_len=32):
    gen = BatchedGenerator(model, max_batch=max_batch, max_len=max_len, engine=engine)
    for t in gen.kv:
        t.fill_(SENT)   # the whole cache is compared: rows nothing wrote keep the sentinel
    return gen


def _state(gen):
    """Everything a prefill or a step writes, as CPU copies."""
    return dict(logits=gen._logits.clone().cpu(), kv=[t.clone().cpu() for t in gen.kv], lens=gen.lens.clone().cpu(),
                finished=gen.finished.clone().cpu())


def _same(a, b, what):
    assert torch.equal(a["logits"].view(torch.int32), b["logits"].view(torch.int32)), f"{what}: logits"
    for l, (x, y) in enumerate(zip(a["kv"], b["kv"])):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f"{what}: KV cache of layer {l}"
    assert torch.equal(a["lens"], b["lens"]) and torch.equal(a["finished"], b["finished"]), f"{what}: lens / finished"


def _forced(B, steps=6):
    f = torch.randint(0, 490, (steps, B), generator=torch.Generator().manual_seed(9))
    assert all(len(set(f[t].tolist())) == B for t in range(steps))
    return f


def _trace(model, engine, dprompts, forced, gpu, max_batch=4):
    gen = _gen(model, engine, max_batch)
    B = len(dprompts)
    sp2 = torch.full((B,), SP2, dtype=torch.long, device=gpu)
    gen.prefill(dprompts)
    states = [_state(gen)]
    for t in range(forced.shape[0]):
        gen.step(forced[t].to(gpu), sp2)
        states.append(_state(gen))
    return states


@pytest.mark.parametrize("feat_dim", [None, 64])
def test_native_is_bitwise_python(gpu, feat_dim):
    """Prefill and 6 teacher-forced steps of the three ragged sequences: logits [B, vocab_pad], every layer's whole
    KV buffer (sentinel-filled before the prefill), lens and finished, after the prefill and after every step."""
    _, _, model = TB._setup(gpu, feat_dim)
    dprompts = TB._dev(TB._prompts(feat_dim or E), gpu)
    forced = _forced(len(dprompts))
    py = _trace(model, "python", dprompts, forced, gpu)
    nat = _trace(model, "native", dprompts, forced, gpu)
    for t, (a, b) in enumerate(zip(py, nat)):
        _same(a, b, f"feat_dim {feat_dim} after {'the prefill' if t == 0 else f'step {t}'}")
    assert nat[-1]["lens"][:3].tolist() == [n + 6 for n in LENS]
    assert (nat[-1]["kv"][0][3] == SENT).all().item()   # the unused fourth slot was never written


def _oracle_gate(model, P0, ocfg, prompts, dprompts, got, forced, gpu):
    """got[t][b] (t = 0: prefill) within LOGIT_ATOL of the oracle's full forward of each sequence alone and of
    KVCacheGenerator; returns the worst of each."""
    worst_o = worst_s = 0.0
    for b, p in enumerate(prompts):
        single = KVCacheGenerator(model, max_len=32)
        seq, types = p[0], p[1]
        lg = single.prefill(*dprompts[b])
        for t in range(len(got)):
            ref = TB._oracle_logits(P0, ocfg, seq, types, p)
            d_o = (got[t][b] - ref).abs().max().item()
            d_s = (got[t][b] - lg.float().cpu()).abs().max().item()
            worst_o, worst_s = max(worst_o, d_o), max(worst_s, d_s)
            assert d_o <= TB.LOGIT_ATOL, (b, t, d_o)
            assert d_s <= TB.LOGIT_ATOL, (b, t, d_s)
            if t == len(got) - 1:
                break
            tok = forced[t, b].view(1, 1)
            seq = torch.cat([seq, tok], 1)
            types = torch.cat([types, torch.full((1, 1), SP2)], 1)
            lg = single.step(tok.to(gpu), torch.full((1, 1), SP2, device=gpu))
    return worst_o, worst_s


@pytest.mark.parametrize("engine", FUSED)
@pytest.mark.parametrize("feat_dim", [None, 64])
def test_fused_steps_meet_the_logits_gate(gpu, feat_dim, engine):
    ocfg, P0, model = TB._setup(gpu, feat_dim)
    prompts = TB._prompts(feat_dim or E)
    dprompts = TB._dev(prompts, gpu)
    B = len(prompts)
    forced = _forced(B)
    sp2 = torch.full((B,), SP2, dtype=torch.long, device=gpu)
    gen = _gen(model, engine)
    got = [gen.prefill(dprompts).float().cpu()]
    for t in range(6):
        got.append(gen.step(forced[t].to(gpu), sp2).float().cpu())
    assert gen.lens[:B].cpu().tolist() == [n + 6 for n in LENS]
    w = _oracle_gate(model, P0, ocfg, prompts, dprompts, got, forced, gpu)
    print(f"{engine} feat_dim {feat_dim}: max |logits - oracle| {w[0]:.4f}, max |logits - KVCacheGenerator| {w[1]:.4f}")


@pytest.mark.parametrize("engine", FUSED)
def test_padding_isolation_fused(gpu, engine):
    """tests/test_gpu_generate_batched.py::test_padding_isolation on the fused engine: A's logits beside a long and a
    short neighbour are bitwise the same (ergm_linear_rows' row independence, seen from the executor)."""
    _, _, model = TB._setup(gpu)
    A, pin = TB._prompts(E, lens=(6, 13), cap_lens=(5, 12), with_feat=0, seed=21)
    long_n, = TB._prompts(E, lens=(12,), cap_lens=(11,), with_feat=-1, seed=22)
    short_n, = TB._prompts(E, lens=(2,), cap_lens=(1,), with_feat=-1, seed=23)
    sp2 = torch.full((3,), SP2, dtype=torch.long, device=gpu)
    runs = []
    for k, nb in enumerate((long_n, short_n)):
        gen = BatchedGenerator(model, max_batch=3, max_len=32, engine=engine)
        logits = [gen.prefill(TB._dev([A, nb, pin], gpu))[0].clone()]
        for t in range(3):
            toks = torch.tensor([40 + t, 100 + 50 * k + t, 7 + t], device=gpu)
            logits.append(gen.step(toks, sp2)[0].clone())
        runs.append(torch.stack(logits).cpu())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))


def _eos_model(gpu):
    """The generate() setup of tests/test_gpu_generate_batched.py: sequence 0 draws eos at its first token."""
    _, P0, model = TB._setup(gpu)
    wte, wpe = P0["transformer.wte.weight"].clone(), P0["transformer.wpe.weight"].clone()
    d = wte[EOS] / wte[EOS].norm()
    wte[EOS], wpe[LENS[0] - 1] = 2.0 * d, 40.0 * d
    model.load_state_dict({**P0, "transformer.wte.weight": wte, "transformer.wpe.weight": wpe}, strict=True)
    return model, TB._dev(TB._prompts(E, with_feat=-1), gpu)


def test_native_generate_returns_the_python_lists(gpu):
    """Seeds 7 and 8, max_new_tokens 1, 8, 9 (below, at and above one 8-sample chunk) and the cache bound; sequence 0
    finishes at once and is stepped on while the others continue, so the lists stop at different steps."""
    model, dprompts = _eos_model(gpu)
    py = BatchedGenerator(model, max_batch=3, max_len=32)
    nat = BatchedGenerator(model, max_batch=3, max_len=32, engine="native")
    for seed in (7, 8):
        for n in (1, 8, 9, None):
            kw = dict(top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=seed, max_new_tokens=n)
            want, got = py.generate(dprompts, **kw), nat.generate(dprompts, **kw)
            assert want == got, (seed, n, want, got)
            assert torch.equal(py.lens.cpu(), nat.lens.cpu()) and py.n_max == nat.n_max, (seed, n)
            if n is None:
                assert want[0] == [EOS] and len({len(r) for r in want}) > 1, want


@pytest.mark.parametrize("engine", FUSED)
def test_fused_generate_deterministic_bounded_and_stops_per_sequence(gpu, engine):
    model, dprompts = _eos_model(gpu)
    gen = BatchedGenerator(model, max_batch=3, max_len=32, engine=engine)
    bound = 32 - max(LENS)
    runs = [gen.generate(dprompts, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7) for _ in range(2)]
    assert runs[0] == runs[1]
    for r in runs[0]:
        assert 1 <= len(r) <= bound and all(0 <= t < V for t in r)
        assert EOS not in r[:-1] and (r[-1] == EOS or len(r) == bound)
    assert runs[0][0] == [EOS] and max(len(r) for r in runs[0][1:]) > 1
    short = gen.generate(dprompts, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7, max_new_tokens=5)
    assert [r[:5] for r in runs[0]] == short


@pytest.mark.parametrize("B", [1, 4])
def test_batch_extremes(gpu, B):
    """B = 1 and B = max_batch = 4: native equals python bitwise, fused is within the gate, prefill + 3 steps."""
    ocfg, P0, model = TB._setup(gpu)
    lens, caps = ((12,), (9,)) if B == 1 else ((5, 12, 13, 9), (7, 12, 3, 6))
    prompts = TB._prompts(E, lens=lens, cap_lens=caps, with_feat=0)
    dprompts = TB._dev(prompts, gpu)
    forced = _forced(B, 3)
    py = _trace(model, "python", dprompts, forced, gpu)
    nat = _trace(model, "native", dprompts, forced, gpu)
    for t, (a, b) in enumerate(zip(py, nat)):
        _same(a, b, f"B {B} step {t}")
    for engine in FUSED:
        fused = _trace(model, engine, dprompts, forced, gpu)
        got = [s["logits"][:B, :V] for s in fused]
        w = _oracle_gate(model, P0, ocfg, prompts, dprompts, got, forced, gpu)
        print(f"B {B} {engine}: max |logits - oracle| {w[0]:.4f}, max |logits - KVCacheGenerator| {w[1]:.4f}")
        assert fused[-1]["lens"][:B].tolist() == [n + 3 for n in lens]


@pytest.mark.parametrize("engine", ("native",) + FUSED)
def test_cache_full_is_refused_before_any_launch(gpu, engine):
    """max_len 16 and a 13-token prompt: three steps fit.  The fourth is refused twice over, by the executor itself
    (ergm_decode_step and ergm_decode_run called directly: ERGM_EINVAL, "cache full") and by BatchedGenerator.step's
    own guard in front of it (ValueError), and every buffer is left as it was."""
    import ctypes as C
    from ergm_amd import _lib as L
    _, _, model = TB._setup(gpu)
    dprompts = TB._dev(TB._prompts(E), gpu)
    gen = _gen(model, engine, max_batch=3, max_len=16)
    sp2 = torch.full((3,), SP2, dtype=torch.long, device=gpu)
    toks = torch.tensor([1, 2, 3], device=gpu)
    gen.prefill(dprompts)
    for _ in range(3):
        gen.step(toks, sp2)
    before = _state(gen)
    lib, stream = L.load(), gen._stream()
    assert lib.ergm_decode_step(gen._plan, C.c_void_p(toks.data_ptr()), C.c_void_p(sp2.data_ptr()), stream) == L.ERGM_EINVAL
    assert "cache full" in L.last_error()
    out = torch.zeros(8, 3, dtype=torch.int64, device=gpu)
    assert lib.ergm_decode_run(gen._plan, 3, 1, 0.9, 7, EOS, SP2, C.c_void_p(out.data_ptr()), stream) == L.ERGM_EINVAL
    assert "cache full" in L.last_error()
    with pytest.raises(ValueError, match="cache full"):
        gen.step(toks, sp2)
    torch.cuda.synchronize()
    _same(before, _state(gen), engine)
    assert gen.n_max == 16 and not out.any().item()
