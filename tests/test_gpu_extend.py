"""Continuing live sequences (ContinuousGenerator.extend, ergm_decode_extend): the native and the fused extension are
bitwise the Python yardstick, which runs the attention through ergm_attn_fwd over each whole sequence; all engines meet
the logits gate of tests/test_gpu_generate_batched.py against the oracle's forward of the concatenated sequence and
against KVCacheGenerator; sessions (submit(keep=True), extend_request, release) repeat, do not depend on their
neighbours and park with the length the device holds; and the dry launch count.  Model, prompts and helpers are
tests/test_gpu_generate_batched.py's, tests/test_gpu_decode_exec.py's and tests/test_gpu_continuous.py's."""
import pytest
import torch

import test_extend_abi as XA
import test_gpu_continuous as TC
import test_gpu_decode_exec as DE
import test_gpu_generate_batched as TB
from ergm_amd.config import ERGMConfig, NO_DROPOUT
from ergm_amd.generate import ContinuousGenerator, KVCacheGenerator
from ergm_amd.model import GPT2LMHeadModel
from oracle import gpt2_oracle as O

pytestmark = pytest.mark.gpu
V, E, SP1, SP2, EOS = TB.V, TB.E, TB.SP1, TB.SP2, TB.EOS
SENT, SLOTS, NO_EOS, ENGINES = TC.SENT, TC.SLOTS, TC.NO_EOS, TC.ENGINES
P_LONG = 192
# the tile edges: after 6 steps the pasts are 63, 64 and 11; the middle turn crosses positions 64 and 128
LONG_LENS, LONG_NEW = (57, 58, 5), (2, 70, 1)
SHORT_NEW = (4, 1, 7)


def _setup_long(gpu, seed=11):
    """TB._setup with 192 positions."""
    ocfg = O.OracleConfig(vocab_size=V, n_embd=E, n_layer=TB.LYR, n_head=TB.H, n_positions=P_LONG, feat_dim=None)
    P0 = O.init_params(ocfg, seed=seed)
    model = GPT2LMHeadModel(ERGMConfig(vocab_size=V, n_embd=E, n_layer=TB.LYR, n_head=TB.H, n_positions=P_LONG, feat_dim=None,
                                       **NO_DROPOUT), device=gpu)
    model.load_state_dict(P0, strict=True)
    return ocfg, P0, model


def _gen(model, engine, max_len=32, **kw):
    gen = ContinuousGenerator(model, max_batch=kw.pop("max_batch", 4), max_len=max_len, cap_max=16, engine=engine, **kw)
    for t in gen.kv + gen.xkv:
        t.fill_(SENT)
    return gen


def _turns(new, seed=17):
    """One (ids, types) per sequence: the other speaker's tokens."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 490, (n,), generator=g), torch.full((n,), SP1)) for n in new]


def _forced(steps, seed):
    return TC._forced_slots(torch.randint(0, 490, (steps, 3), generator=torch.Generator().manual_seed(seed)))


def _load(gen, state):
    gen._logits.copy_(state["logits"])
    for name in ("kv", "xkv"):
        for t, x in zip(getattr(gen, name), state[name]):
            t.copy_(x)
    for k, x in state["ints"].items():
        getattr(gen, k).copy_(x)


def _long_trace(model, engine, gpu, before=None):
    """Admit, 6 forced steps, the extension, 6 forced steps; the states from just before the extension on.  ``before``:
    the state to extend from, in place of the generator's own (the fused steps differ from the yardstick's)."""
    dprompts = TB._dev(TB._prompts(E, lens=LONG_LENS), gpu)
    turns = [(i.to(gpu), t.to(gpu)) for i, t in _turns(LONG_NEW)]
    gen = _gen(model, engine, max_len=P_LONG)
    sp2 = torch.full((4,), SP2, dtype=torch.long, device=gpu)
    gen.admit(SLOTS, dprompts, request_ids=(5, 6, 7))
    f1, f2 = _forced(6, 9), _forced(6, 10)
    for t in range(6):
        gen.step(f1[t].to(gpu), sp2)
    if before is not None:
        _load(gen, before)
    states = [TC._state(gen)]
    gen.extend(SLOTS, turns, past=[n + 6 for n in LONG_LENS])
    states.append(TC._state(gen))
    for t in range(6):
        gen.step(f2[t].to(gpu), sp2)
        states.append(TC._state(gen))
    return states


def test_native_and_fused_extension_are_bitwise_python(gpu):
    """Prompts of 57, 58 and 5 tokens (sequence 1 with features) in slots (2, 0, 3) of sentinel-filled caches of 192
    rows, 6 teacher-forced steps, then 2, 70 and 1 more tokens behind pasts of 63, 64 and 11 rows, then 6 more steps.
    Logits, every layer's whole kv and xkv and the six state arrays, after the extension and after every step: native
    against python at every point; fused against python at the extension itself (from the yardstick's state: the same
    kernels), and against its own rerun after the steps."""
    _, _, model = _setup_long(gpu)
    py = _long_trace(model, "python", gpu)
    nat = _long_trace(model, "native", gpu)
    for t, (a, b) in enumerate(zip(py, nat)):
        TC._same(a, b, "before the extension" if t == 0 else "after the extension" if t == 1 else f"step {t - 1} after it")
    fused = [_long_trace(model, "fused", gpu, before=py[0]) for _ in range(2)]
    TC._same(py[1], fused[0][1], "fused, after the extension")
    for t, (a, b) in enumerate(zip(*fused)):
        TC._same(a, b, f"fused rerun, state {t}")
    before, after, last = nat[0], nat[1], nat[-1]
    lens = [n + 6 + k for n, k in zip(LONG_LENS, LONG_NEW)]
    assert lens == [65, 134, 12]
    for b, s in enumerate(SLOTS):
        assert before["ints"]["lens"][s] == LONG_LENS[b] + 6
        assert after["ints"]["lens"][s] == lens[b] and after["ints"]["stop_lens"][s] == P_LONG
        assert after["ints"]["row_ids"][s] == 5 + b and after["ints"]["row_steps"][s] == 6   # the counters go on
        assert after["ints"]["cap_lens"][s] == TB.CAP_LENS[b] and after["ints"]["finished"][s] == 0
        assert last["ints"]["lens"][s] == lens[b] + 6 and last["ints"]["row_steps"][s] == 12
        for l in range(TB.LYR):   # the rows past a sequence's length keep what they held, the rows below the past too
            assert (after["kv"][l][s, lens[b]:] == SENT).all().item()
            assert not (after["kv"][l][s, LONG_LENS[b] + 6:lens[b]] == SENT).all().item()
            assert torch.equal(after["kv"][l][s, :LONG_LENS[b] + 6].view(torch.int16),
                               before["kv"][l][s, :LONG_LENS[b] + 6].view(torch.int16))
    for l in range(TB.LYR):       # the idle slot (the steps' appends land in its row 0), and the captions
        assert torch.equal(after["kv"][l][1].view(torch.int16), before["kv"][l][1].view(torch.int16))
        assert (last["kv"][l][1, 1:] == SENT).all().item()
        assert torch.equal(after["xkv"][l].view(torch.int16), before["xkv"][l].view(torch.int16))
    assert after["ints"]["finished"].tolist() == [0, 1, 0, 0] and after["ints"]["lens"][1] == 0
    assert torch.equal(after["logits"][1].view(torch.int32), before["logits"][1].view(torch.int32))


def _sequences(prompts, f1, turns, f2):
    """Per sequence: all tokens and types of admit + steps + turn + steps, and the lengths at which logits are read."""
    out = []
    for b, p in enumerate(prompts):
        s = SLOTS[b]
        ids = torch.cat([p[0].view(-1), f1[:, s], turns[b][0], f2[:, s]])
        tt = torch.cat([p[1].view(-1), torch.full((f1.shape[0],), SP2), turns[b][1], torch.full((f2.shape[0],), SP2)])
        n_ext = p[0].numel() + f1.shape[0] + turns[b][0].numel()
        out.append((ids, tt, [n_ext + t for t in range(f2.shape[0] + 1)]))
    return out


def _oracle_rows(P0, ocfg, prompts, seqs):
    """The oracle's next-token logits at every checkpoint of every sequence (one forward of the full sequence each)."""
    ref = []
    for p, (ids, tt, cps) in zip(prompts, seqs):
        lg = O.forward(P0, ocfg, input_ids=ids.view(1, -1), token_type_ids=tt.view(1, -1), caption_ids=p[2], visual_feat=p[3],
                       audio_feat=p[4])["logits"][0]
        ref.append([lg[n - 1] for n in cps])
    return ref


def _extension_logits(model, engine, gpu, prompts, f1, turns, f2, max_len):
    dprompts = TB._dev(prompts, gpu)
    gen = _gen(model, engine, max_len=max_len)
    sp2 = torch.full((4,), SP2, dtype=torch.long, device=gpu)
    gen.admit(SLOTS, dprompts)
    for t in range(f1.shape[0]):
        gen.step(f1[t].to(gpu), sp2)
    gen.extend(SLOTS, [(i.to(gpu), t.to(gpu)) for i, t in turns])   # past read from the device
    got = [gen.logits[list(SLOTS)].float().cpu()]
    for t in range(f2.shape[0]):
        got.append(gen.step(f2[t].to(gpu), sp2)[list(SLOTS)].float().cpu())
    return got


@pytest.fixture(scope="module")
def short_refs(gpu):
    """The references of the gate on the 64-position model, computed once: the oracle and KVCacheGenerator."""
    ocfg, P0, model = TB._setup(gpu)
    prompts = TB._prompts(E)
    f1, f2, turns = _forced(3, 9), _forced(3, 10), _turns(SHORT_NEW)
    seqs = _sequences(prompts, f1, turns, f2)
    oracle = _oracle_rows(P0, ocfg, prompts, seqs)
    single = []
    for b, (p, (ids, tt, cps)) in enumerate(zip(TB._dev(prompts, gpu), seqs)):
        g = KVCacheGenerator(model, max_len=32)
        n0 = p[0].numel()
        lg, rows = g.prefill(*p), []
        for n in range(n0, cps[-1] + 1):
            if n in cps:
                rows.append(lg.float().cpu().view(-1))
            if n < cps[-1]:
                lg = g.step(ids[n].view(1, 1).to(gpu), tt[n].view(1, 1).to(gpu))
        single.append(rows)
    return model, prompts, f1, turns, f2, oracle, single


@pytest.mark.parametrize("engine", ENGINES)
def test_extension_meets_the_logits_gate(gpu, short_refs, engine):
    """The 64-position model: admit, 3 forced steps, extend by (4, 1, 7) tokens, 3 forced steps; the logits after the
    extension and after each later step against the oracle's full forward of the concatenated sequence (with the
    admission's captions and features) and against KVCacheGenerator stepped over the same tokens."""
    model, prompts, f1, turns, f2, oracle, single = short_refs
    got = _extension_logits(model, engine, gpu, prompts, f1, turns, f2, 32)
    worst_o = worst_s = 0.0
    for b in range(3):
        for t in range(4):
            d_o = (got[t][b] - oracle[b][t]).abs().max().item()
            d_s = (got[t][b] - single[b][t]).abs().max().item()
            worst_o, worst_s = max(worst_o, d_o), max(worst_s, d_s)
            assert d_o <= TB.LOGIT_ATOL, (b, t, d_o)
            assert d_s <= TB.LOGIT_ATOL, (b, t, d_s)
    print(f"{engine}: max |logits - oracle| {worst_o:.4f}, max |logits - KVCacheGenerator| {worst_s:.4f}")


def test_extension_against_one_shot_at_the_tile_edges(gpu):
    """The 192-position model at the lengths of the bitwise test: the worst deviation from the oracle of the extension
    path and of the one-shot path (the whole concatenation admitted as one prompt), over the logits after the
    extension and after each of 6 later steps.  The extension is within the gate whenever the one-shot path is; where
    the one-shot path itself is outside it at these lengths, the two paths only round differently: extension <=
    1.5 x one-shot.
    Measured (MI355X, engine native): extension 0.0027, one-shot 0.0028, the gate 0.06."""
    ocfg, P0, model = _setup_long(gpu)
    prompts = TB._prompts(E, lens=LONG_LENS)
    f1, f2, turns = _forced(6, 9), _forced(6, 10), _turns(LONG_NEW)
    seqs = _sequences(prompts, f1, turns, f2)
    oracle = _oracle_rows(P0, ocfg, prompts, seqs)
    ext = _extension_logits(model, "native", gpu, prompts, f1, turns, f2, P_LONG)
    whole = [(ids[:cps[0]].view(1, -1), tt[:cps[0]].view(1, -1), p[2], p[3], p[4]) for p, (ids, tt, cps) in zip(prompts, seqs)]
    gen = _gen(model, "native", max_len=P_LONG)
    sp2 = torch.full((4,), SP2, dtype=torch.long, device=gpu)
    gen.admit(SLOTS, TB._dev(whole, gpu))
    one = [gen.logits[list(SLOTS)].float().cpu()]
    for t in range(6):
        one.append(gen.step(f2[t].to(gpu), sp2)[list(SLOTS)].float().cpu())
    w_ext = max((ext[t][b] - oracle[b][t]).abs().max().item() for b in range(3) for t in range(7))
    w_one = max((one[t][b] - oracle[b][t]).abs().max().item() for b in range(3) for t in range(7))
    print(f"192 positions: max |logits - oracle| extension {w_ext:.4f}, one-shot {w_one:.4f}")
    if w_one <= TB.LOGIT_ATOL:
        assert w_ext <= TB.LOGIT_ATOL, (w_ext, w_one)
    else:
        assert w_ext <= 1.5 * w_one, (w_ext, w_one)


# ---- sessions --------------------------------------------------------------------------------------------------
REQ_LENS, REQ_CAPS, REQ_NEW = (5, 12, 13, 9, 3, 11), (7, 12, 3, 5, 1, 9), (4, 9, 3, 10, 2, 8)
TURN2, TURN2_NEW = 5, 6


def _two_turns(gen, prompts, session, seed=7):
    """Every prompt submitted (the session's kept), run; the session continued beside the others submitted again,
    run.  Returns the session's tokens and final logits of both turns, and everything else that came back."""
    ids2, tt2 = _turns((TURN2,), seed=23)[0]
    out = []
    for turn in range(2):
        for i, (p, k) in enumerate(zip(prompts, REQ_NEW)):
            if i == session and turn == 1:
                gen.extend_request(i, ids2, tt2, TURN2_NEW)
            elif i == session:
                assert gen.submit(p, k, request_id=i, keep=True) == i
            else:
                gen.submit(p, k, request_id=i)
        res = gen.run(top_p=0.9, eos_id=NO_EOS, sp2_id=SP2, seed=seed)
        out.append((res, gen.final_logits[session].clone().cpu()))
    return out


def test_sessions_repeat_and_do_not_depend_on_their_neighbours(gpu):
    """Engine "fused" with max_admit = 1: session 1 (a 12-token prompt with features, 9 new tokens, then a turn of 5
    tokens and 6 new ones) beside five other requests on four slots, twice, and alone: the same token lists for both
    turns and bitwise the same final logits."""
    _, _, model = TB._setup(gpu)
    prompts = TB._dev(TB._prompts(E, lens=REQ_LENS, cap_lens=REQ_CAPS, with_feat=1, seed=31), gpu)
    runs = [_two_turns(_gen(model, "fused", max_admit=1, keep_logits=True), prompts, 1) for _ in range(2)]
    alone = _two_turns(_gen(model, "fused", max_admit=1, keep_logits=True), prompts[:2], 1)   # request 0 retires at once
    (r1, l1), (r2, l2) = runs[0]
    assert [len(r1[i]) for i in range(6)] == list(REQ_NEW) and len(r2[1]) == TURN2_NEW
    assert sorted(r1) == sorted(r2) == list(range(6))
    for (a1, b1), (a2, b2) in zip(runs[0], runs[1]):
        assert a1 == a2 and torch.equal(b1.view(torch.int32), b2.view(torch.int32))
    solo = _gen(model, "fused", max_admit=1, keep_logits=True)
    ids2, tt2 = _turns((TURN2,), seed=23)[0]
    solo.submit(prompts[1], REQ_NEW[1], request_id=1, keep=True)
    assert solo.run(top_p=0.9, eos_id=NO_EOS, sp2_id=SP2, seed=7) == {1: r1[1]}
    assert torch.equal(solo.final_logits[1].cpu().view(torch.int32), l1.view(torch.int32))
    solo.extend_request(1, ids2, tt2, TURN2_NEW)
    assert solo.run(top_p=0.9, eos_id=NO_EOS, sp2_id=SP2, seed=7) == {1: r2[1]}
    assert torch.equal(solo.final_logits[1].cpu().view(torch.int32), l2.view(torch.int32))
    assert alone[0][0][1] == r1[1] and alone[1][0][1] == r2[1]
    assert solo.sched.parked[1][1] == REQ_LENS[1] + REQ_NEW[1] + TURN2 + TURN2_NEW == int(solo.lens[0])
    other = _gen(model, "fused", max_admit=1, keep_logits=True)
    assert _two_turns(other, prompts, 1, seed=8)[1][0][1] != r2[1]   # another seed, another continuation


@pytest.mark.parametrize("engine", ENGINES)
def test_parked_lengths_release_and_refusals(gpu, engine):
    """DE's eos construction on two slots: the 5-token prompt draws eos at its first token and parks with 5 rows, the
    eos not among them; its neighbour runs to its bound of 3 and parks with 12 + 3.  Both equal the device's lens.
    The eos-ended session is continued (its new rows overwrite the row the steps appended to), a released slot goes to
    a queued request, and unknown, released and running ids are refused."""
    model, dprompts = DE._eos_model(gpu)
    gen = _gen(model, engine, max_batch=2)
    a = gen.submit(dprompts[0], 10, keep=True)
    b = gen.submit(dprompts[1], 3, keep=True)
    out = gen.run(top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7)
    assert out[a] == [EOS] and gen.sched.parked[a] == (0, 5, TB.CAP_LENS[0])
    lens = gen.lens.cpu().tolist()
    for rid, n in ((a, 5), (b, 12)):
        slot, rows, _ = gen.sched.parked[rid]
        assert rows == n + len(out[rid]) - (1 if out[rid][-1] == EOS else 0) == lens[slot], rid
    if EOS not in out[b]:
        assert len(out[b]) == 3 and gen.sched.parked[b][1] == 15
    # a queued request cannot start while both slots are parked
    c = gen.submit(dprompts[2], 2)
    with pytest.raises(RuntimeError):
        gen.run(top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7)
    with pytest.raises(ValueError):
        gen.extend_request(c, *_turns((2,))[0])          # queued, not parked
    with pytest.raises(ValueError):
        gen.extend_request(77, *_turns((2,))[0])         # unknown
    with pytest.raises(ValueError):
        gen.extend_request(a, *_turns((27,))[0])         # 5 + 27 rows leave no room for a new token
    gen.release(b)
    with pytest.raises(ValueError):
        gen.extend_request(b, *_turns((2,))[0])          # released
    with pytest.raises(ValueError):
        gen.release(b)
    ids, tt = _turns((3,), seed=29)[0]
    gen.extend_request(a, ids, tt, 4)
    out2 = gen.run(top_p=0.9, eos_id=EOS, sp2_id=SP2, seed=7)
    assert sorted(out2) == sorted([a, c]) and gen.sched.admissions[-1] == [(c, 1)]   # c took the released slot
    assert gen.sched.extensions == [[(a, 0)]]
    slot, rows, _ = gen.sched.parked[a]
    assert slot == 0 and rows == 5 + 3 + len(out2[a]) - (1 if out2[a][-1] == EOS else 0) == int(gen.lens[0])
    assert 1 <= len(out2[a]) <= 4 and gen.sched.parked.keys() == {a}
    with pytest.raises(ValueError):
        gen.submit(TB._dev(TB._prompts(E, lens=(1,), cap_lens=(3,), with_feat=0), gpu)[0], 2, keep=True)   # features, 1 token
    # the low-level guards
    with pytest.raises(ValueError):
        gen.extend([0, 0], [(ids, tt), (ids, tt)], past=[8, 8])
    with pytest.raises(ValueError):
        gen.extend([0], [(ids, tt)], past=[1])
    with pytest.raises(ValueError):
        gen.extend([0], [(ids, tt)], max_new_tokens=[30], past=[8])


@pytest.mark.parametrize("engine", ["native", "fused"])
def test_extend_launch_count(gpu, engine):
    """ergm_decode_extend_launches on a live plan equals the launch sequence counted by hand (tests/test_extend_abi.py:
    12 kernels per block + 6, each GEMM that ergm_gemm_plan splits adding its reduction), and is the same for 1 and 3
    sequences."""
    _, _, model = TB._setup(gpu)
    gen = _gen(model, engine)
    for R in (3, 12, 70):
        for n_seq in (1, 3):
            assert gen.extend_launches(n_seq, R) == XA.extend_kernels(R, n_seq, E, gen.F, model.layout.vocab_pad, TB.LYR)
        assert gen.extend_launches(1, R) == gen.extend_launches(3, R) >= 12 * TB.LYR + 6
    with pytest.raises(ValueError):
        gen.extend_launches(3, 2)
