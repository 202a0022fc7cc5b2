"""Continuous batching (ergm_amd.generate.ContinuousGenerator): the native admission (ergm_decode_admit: packed
embedding, ragged attention, rows to slots) and the slot steps are bitwise the Python yardstick; all engines meet the
logits gate of tests/test_gpu_generate_batched.py; a single request on one slot returns BatchedGenerator's list; a
request's tokens and logits do not depend on the slot it gets or on what it runs beside; requests stop at eos or at
their bound, on the device; and Trainer.test.  Model, prompts and helpers are tests/test_gpu_generate_batched.py's and
tests/test_gpu_decode_exec.py's."""
import pytest
import torch

import test_gpu_decode_exec as DE
import test_gpu_generate_batched as TB
from ergm_amd.data import synthetic_batch
from ergm_amd.generate import BatchedGenerator, ContinuousGenerator
from ergm_amd.train import Trainer

pytestmark = pytest.mark.gpu
V, E, SP1, SP2, EOS, LENS, CAP_LENS = TB.V, TB.E, TB.SP1, TB.SP2, TB.EOS, TB.LENS, TB.CAP_LENS
SENT = DE.SENT
NO_EOS = -1          # never drawn: every list has exactly max_new_tokens tokens
SLOTS = (2, 0, 3)    # out of order; slot 1 stays idle
ENGINES = ("python", "native", "fused")


def _gen(model, engine, max_batch=4, cap_max=16, **kw):
    gen = ContinuousGenerator(model, max_batch=max_batch, max_len=32, cap_max=cap_max, engine=engine, **kw)
    for t in gen.kv + gen.xkv:
        t.fill_(SENT)   # the whole caches are compared: rows nothing wrote keep the sentinel
    return gen


def _state(gen):
    """Everything an admission or a step writes, as CPU copies."""
    return dict(logits=gen._logits.clone().cpu(), kv=[t.clone().cpu() for t in gen.kv],
                xkv=[t.clone().cpu() for t in gen.xkv],
                ints={k: getattr(gen, k).clone().cpu() for k in ("lens", "cap_lens", "finished", "row_steps", "stop_lens",
                                                                 "row_ids")})


def _same(a, b, what):
    assert torch.equal(a["logits"].view(torch.int32), b["logits"].view(torch.int32)), f"{what}: logits"
    for name in ("kv", "xkv"):
        for l, (x, y) in enumerate(zip(a[name], b[name])):
            assert torch.equal(x.view(torch.int16), y.view(torch.int16)), f"{what}: {name} of layer {l}"
    for k, x in a["ints"].items():
        assert torch.equal(x, b["ints"][k]), f"{what}: {k}"


def _forced_slots(forced):
    """forced [steps, 3] per sequence -> [steps, 4] per slot (the idle slot gets a token of its own)."""
    f = torch.full((forced.shape[0], 4), 123, dtype=torch.long)
    for b, s in enumerate(SLOTS):
        f[:, s] = forced[:, b]
    return f


def _trace(model, engine, dprompts, forced, gpu):
    gen = _gen(model, engine)
    sp2 = torch.full((4,), SP2, dtype=torch.long, device=gpu)
    gen.admit(SLOTS, dprompts, request_ids=(5, 6, 7))
    states = [_state(gen)]
    for t in range(forced.shape[0]):
        gen.step(forced[t].to(gpu), sp2)
        states.append(_state(gen))
    return states


@pytest.mark.parametrize("feat_dim", [None, 64])
def test_native_admission_is_bitwise_python(gpu, feat_dim):
    """The three ragged prompts (lengths 5 / 12 / 13, captions 7 / 12 / 3, sequence 1 with features) admitted into slots
    (2, 0, 3) of sentinel-filled caches, then 6 teacher-forced steps over all four slots: logits, every layer's whole
    kv and xkv, and the slot state, after the admission and after every step."""
    _, _, model = TB._setup(gpu, feat_dim)
    dprompts = TB._dev(TB._prompts(feat_dim or E), gpu)
    forced = _forced_slots(DE._forced(3))
    py = _trace(model, "python", dprompts, forced, gpu)
    nat = _trace(model, "native", dprompts, forced, gpu)
    for t, (a, b) in enumerate(zip(py, nat)):
        _same(a, b, f"feat_dim {feat_dim} after {'the admission' if t == 0 else f'step {t}'}")
    first, last = nat[0], nat[-1]
    for b, s in enumerate(SLOTS):
        assert first["ints"]["lens"][s] == LENS[b] and first["ints"]["cap_lens"][s] == CAP_LENS[b]
        assert first["ints"]["stop_lens"][s] == 32 and first["ints"]["row_ids"][s] == 5 + b
        assert last["ints"]["lens"][s] == LENS[b] + 6 and last["ints"]["row_steps"][s] == 6
        for name, n in (("kv", LENS[b]), ("xkv", CAP_LENS[b])):   # the rows past a sequence's own keep the sentinel
            assert (first[name][0][s, n:] == SENT).all().item() and not (first[name][0][s, :n] == SENT).all().item()
    assert first["ints"]["finished"].tolist() == [0, 1, 0, 0] and last["ints"]["finished"].tolist() == [0, 1, 0, 0]
    assert last["ints"]["lens"][1] == 0 and last["ints"]["row_steps"][1] == 0
    assert (first["kv"][0][1] == SENT).all().item() and (first["xkv"][0][1] == SENT).all().item()
    # the idle slot: a step's append lands in its row 0, which nobody reads; nothing else of it is written
    assert (last["kv"][0][1, 1:] == SENT).all().item() and (last["xkv"][0][1] == SENT).all().item()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("feat_dim", [None, 64])
def test_slots_meet_the_logits_gate(gpu, feat_dim, engine):
    ocfg, P0, model = TB._setup(gpu, feat_dim)
    prompts = TB._prompts(feat_dim or E)
    dprompts = TB._dev(prompts, gpu)
    forced = DE._forced(3)
    fs = _forced_slots(forced)
    sp2 = torch.full((4,), SP2, dtype=torch.long, device=gpu)
    gen = _gen(model, engine)
    gen.admit(SLOTS, dprompts)
    got = [gen.logits[list(SLOTS)].float().cpu()]
    for t in range(6):
        got.append(gen.step(fs[t].to(gpu), sp2)[list(SLOTS)].float().cpu())
    w = DE._oracle_gate(model, P0, ocfg, prompts, dprompts, got, forced, gpu)
    print(f"{engine} feat_dim {feat_dim}: max |logits - oracle| {w[0]:.4f}, max |logits - KVCacheGenerator| {w[1]:.4f}")


@pytest.mark.parametrize("engine", ["python", "native"])
def test_one_slot_returns_the_static_generators_list(gpu, engine):
    """ContinuousGenerator(max_batch=1) serving one request with id 0 against BatchedGenerator(max_batch=1).generate:
    seeds 7 and 8, max_new_tokens 1, 8 and 9 (below, at and above one 8-step look).  The two paths issue the same
    kernels with the same arguments, with one exception that changes nothing here: the decode cross-attention is given
    the row bound cap_max (16) where the static path gives the caption length (9).  The bound only clamps lengths and
    picks the automatic split count, which is 1 for every bound below 512 rows, so the launches are the same."""
    _, _, model = TB._setup(gpu)
    p = TB._dev(TB._prompts(E, lens=(12,), cap_lens=(9,), with_feat=0), gpu)
    for seed in (7, 8):
        for k in (1, 8, 9):
            want = BatchedGenerator(model, max_batch=1, max_len=32, engine=engine).generate(
                p, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=seed, max_new_tokens=k)
            gen = ContinuousGenerator(model, max_batch=1, max_len=32, cap_max=16, engine=engine)
            rid = gen.submit(p[0], k, request_id=0)
            got = gen.run(top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=seed)
            assert got == {rid: want[0]}, (seed, k)
            assert len(want[0]) == k or want[0][-1] == EOS


REQ_LENS, REQ_CAPS = (5, 12, 13, 9, 3, 11, 7), (7, 12, 3, 5, 1, 9, 16)
REQ_NEW = (1, 9, 3, 17, 2, 8, 5)


@pytest.mark.parametrize("engine", ["fused", "native"])
def test_results_do_not_depend_on_the_schedule(gpu, engine):
    """Seven requests with max_new_tokens (1, 9, 3, 17, 2, 8, 5) on 4 slots, admitted one sequence per call
    (max_admit = 1, so an admission's GEMMs see the same rows as when the request runs alone).  Slots are reused and
    request 6 (5 tokens) lands in the slot request 1 (9 tokens) left; request 3 (17 tokens, three looks) holds its
    slot until the queue is empty, so that one slot serves one request.  Every request's tokens and final logits row
    are bitwise what the same request with the same id gets alone in a fresh generator of 4 slots (where it takes
    slot 0), and a second full run on the used generator repeats the first."""
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E, lens=REQ_LENS, cap_lens=REQ_CAPS, with_feat=1, seed=31), gpu)
    gen = _gen(model, engine, max_admit=1, keep_logits=True)
    runs = []
    for _ in range(2):
        for i, (p, k) in enumerate(zip(prompts, REQ_NEW)):
            assert gen.submit(p, k, request_id=i) == i
        out = gen.run(top_p=0.9, eos_id=NO_EOS, sp2_id=SP2, seed=7)
        runs.append((out, {i: t.clone().cpu() for i, t in gen.final_logits.items()}))
    slot_of = {i: s for call in gen.sched.admissions[:7] for i, s in call}
    assert all(len(call) == 1 for call in gen.sched.admissions) and len(gen.sched.admissions) == 14
    assert [slot_of[i] for i in range(4)] == [0, 1, 2, 3] and slot_of[6] == slot_of[1]
    assert len({slot_of[i] for i in (4, 5, 6)}) == 3 and slot_of[3] not in (slot_of[4], slot_of[5], slot_of[6])
    out, logits = runs[0]
    assert [len(out[i]) for i in range(7)] == list(REQ_NEW)
    assert runs[1][0] == out
    for i in range(7):
        assert torch.equal(runs[1][1][i].view(torch.int32), logits[i].view(torch.int32)), i
    for i, (p, k) in enumerate(zip(prompts, REQ_NEW)):
        alone = _gen(model, engine, max_admit=1, keep_logits=True)
        alone.submit(p, k, request_id=i)
        assert alone.run(top_p=0.9, eos_id=NO_EOS, sp2_id=SP2, seed=7) == {i: out[i]}, i
        assert torch.equal(alone.final_logits[i].cpu().view(torch.int32), logits[i].view(torch.int32)), i
    other = _gen(model, engine, max_admit=1)
    assert other.generate(prompts[:2], 0.9, NO_EOS, SP2, seed=8, max_new_tokens=[1, 9])[1] != out[1]   # another seed


@pytest.mark.parametrize("engine", ENGINES)
def test_stop_at_eos_and_at_the_bound_on_the_device(gpu, engine):
    """TB's eos construction: the request with the 5-token prompt draws eos at its first token while its neighbour runs
    on; its slot is admitted into again at the next look and its list is [EOS].  A request stops at exactly
    max_new_tokens.  The flags come from the device: the host writes `finished` only at an admission (0), the
    scheduler raises if a flag it reads disagrees with the tokens, and no length ever passes its bound."""
    model, dprompts = DE._eos_model(gpu)
    gen = _gen(model, engine, max_batch=2)
    new = (10, 12, 3, 9)
    reqs = [dprompts[0], dprompts[1], dprompts[2], dprompts[1]]
    looks = []
    run_chunk = gen.run_chunk

    def watched(n):
        r = run_chunk(n)
        looks.append((gen.lens.cpu().tolist(), gen.stop_lens.cpu().tolist(), gen.finished.cpu().tolist(),
                      [None if q is None else q.id for q in gen.sched.live]))
        return r

    gen.run_chunk = watched
    ids = [gen.submit(p, k) for p, k in zip(reqs, new)]
    out = gen.run(top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7)
    assert ids == [0, 1, 2, 3] and sorted(out) == ids
    assert out[0] == [EOS]
    for i, k in enumerate(new):
        assert 1 <= len(out[i]) <= k and EOS not in out[i][:-1] and (out[i][-1] == EOS or len(out[i]) == k), i
        assert all(0 <= t < V for t in out[i])
    assert len(out[1]) > 1                                   # the neighbour ran on
    assert gen.sched.admissions[0] == [(0, 0), (1, 1)]
    assert gen.sched.admissions[1][0] == (2, 0)              # slot 0 again, at the next look
    for lens, stops, fin, live in looks:
        assert all(n <= s for n, s in zip(lens, stops))
    lens, stops, fin, live = looks[0]
    assert fin[0] == 1 and lens[0] == 5                      # eos at the first draw: the length never advanced
    lens, stops, fin, live = looks[1]
    assert live[0] == 2 and fin[0] == 1                      # request 2 (3 tokens) finished inside its first chunk
    if EOS not in out[2]:
        assert len(out[2]) == 3 and lens[0] == stops[0] == 13 + 3
    assert gen.finished.cpu().tolist() == [1, 1]
    # the low-level guards
    with pytest.raises(ValueError):
        gen.admit([0], [dprompts[2]], max_new_tokens=[20])   # 13 + 20 > max_len
    with pytest.raises(ValueError):
        gen.admit([0, 0], dprompts[:2])
    with pytest.raises(ValueError):
        gen.submit(dprompts[2], 20)


def test_trainer_test(gpu):
    """Trainer.test on a 5-sample loader (batches of 3 and 2, eos-padded inputs of different lengths): one hypothesis
    per sample within its bound, the references are labels != -100, the emotion labels are the loader's, the losses
    are the LM losses of the inference forward on the same batches, and seeded runs repeat."""
    _, _, model = TB._setup(gpu)
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
    tr = Trainer(model, None)
    runs = [tr.test(batches, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=3, max_batch=2, max_len=32) for _ in range(2)]
    hyps, refs, emos, losses = runs[0]
    assert runs[1] == runs[0]
    assert len(hyps) == len(refs) == len(emos) == 5 and len(losses) == 2
    n_in = [S - p for p in pads]
    for i, h in enumerate(hyps):
        assert 1 <= len(h) <= 32 - n_in[i] and EOS not in h[:-1] and (h[-1] == EOS or len(h) == 32 - n_in[i])
    flat = [(b, i) for b in batches for i in range(b["input_ids"].shape[0])]
    for (b, i), r in zip(flat, refs):
        assert r == b["labels"][i][b["labels"][i] != -100].tolist()
    assert emos == [int(x) for b in batches for x in b["emotion_labels"]]
    model.eval()
    for b, loss in zip(batches, losses):
        d = {k: v.to(gpu) for k, v in b.items()}
        with torch.no_grad():
            out = model(input_ids=d["input_ids"], token_type_ids=d["token_type_ids"], labels=d["labels"],
                        emotion_labels=d["emotion_labels"], caption_ids=d["caption_ids"], imgs=d["visual_feat"],
                        auds=d["audio_feat"])
        assert float(out.loss_lm) == loss
    assert tr.test(batches, top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=4, max_batch=2, max_len=32)[0] != hyps
    assert tr.test(batches, 0.9, EOS, SP2, seed=3, max_batch=4, max_len=32, engine="native")[1] == refs
