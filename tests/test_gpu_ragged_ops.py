"""The kernels of continuous batching against the kernels they extend, bitwise: ergm_attn_fwd_ragged against
ergm_attn_fwd on every sequence alone, ergm_rows_to_slots against the source rows (and nothing else touched),
ergm_embed_packed against ergm_embed_fwd(B = 1), ergm_topp_sample_rows against ergm_topp_sample."""
import numpy as np
import pytest
import torch

import test_gpu_decode_ops as DO
from ergm_amd import ops

pytestmark = pytest.mark.gpu
H, E = 2, 128
SENT = -12288.0   # exact in bf16
# the edges of the 64-row tiles: one below, at and one above a tile, and the same past two tiles
LENS = (1, 2, 63, 64, 65, 130)
CAP_LENS = (1, 64, 65, 129, 3, 7)
SPARE = 8


def _i32(v, gpu):
    return torch.tensor(v, dtype=torch.int32, device=gpu)


def _starts(lens):
    return [sum(lens[:b]) for b in range(len(lens))]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.fixture(scope="module")
def packed(gpu):
    """The packed operands and, computed once, ergm_attn_fwd's output and LSE of every sequence alone."""
    g = torch.Generator().manual_seed(3)
    R, Rc = sum(LENS), sum(CAP_LENS)
    assert R == 325
    qkv = torch.randn(R, 3 * E, generator=g).to(torch.bfloat16).to(gpu)
    ckv = torch.randn(Rc, 2 * E, generator=g).to(torch.bfloat16).to(gpu)
    want = {}
    for causal in (True, False):
        o = torch.full((R + SPARE, E), SENT, dtype=torch.bfloat16, device=gpu)
        lse = torch.full((H * (R + SPARE),), SENT, dtype=torch.float32, device=gpu)
        for b, (r0, n, c0, c) in enumerate(zip(_starts(LENS), LENS, _starts(CAP_LENS), CAP_LENS)):
            q = qkv[r0:r0 + n, :E]
            if causal:
                ob, lb = ops.attn_fwd(q, qkv[r0:r0 + n, E:2 * E], qkv[r0:r0 + n, 2 * E:], 1, H, n, n, True)
            else:
                ob, lb = ops.attn_fwd(q, ckv[c0:c0 + c, :E], ckv[c0:c0 + c, E:], 1, H, n, c, False)
            o[r0:r0 + n] = ob
            lse[H * r0:H * (r0 + n)] = lb.reshape(-1)
        want[causal] = (o, lse)
    torch.cuda.synchronize()
    return qkv, ckv, want


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("with_lse", [False, True])
def test_attn_fwd_ragged_is_bitwise_attn_fwd_per_sequence(gpu, packed, causal, with_lse):
    """325 packed query rows of six sequences in one launch; the output buffer, sentinel-filled and with spare rows
    behind row 325, is compared whole with the per-sequence ergm_attn_fwd results; two runs give the same bits."""
    qkv, ckv, want = packed
    R = sum(LENS)
    qs, ql = _i32(_starts(LENS), gpu), _i32(LENS, gpu)
    cs, cl = _i32(_starts(CAP_LENS), gpu), _i32(CAP_LENS, gpu)
    runs = []
    for _ in range(2):
        o = torch.full((R + SPARE, E), SENT, dtype=torch.bfloat16, device=gpu)
        lse = torch.full((H * (R + SPARE),), SENT, dtype=torch.float32, device=gpu) if with_lse else None
        q = qkv[:, :E]
        if causal:
            ops.attn_fwd_ragged(q, qkv[:, E:2 * E], qkv[:, 2 * E:], qs, ql, qs, ql, H, max(LENS), max(LENS), True, o=o[:R],
                                lse=lse)
        else:
            ops.attn_fwd_ragged(q, ckv[:, :E], ckv[:, E:], qs, ql, cs, cl, H, max(LENS), max(CAP_LENS), False, o=o[:R],
                                lse=lse)
        runs.append((o, lse))
    wo, wl = want[causal]
    for o, lse in runs:
        assert torch.equal(_bits(o), _bits(wo))
        if with_lse:
            assert torch.equal(_bits(lse), _bits(wl))
    for b, (r0, n) in enumerate(zip(_starts(LENS), LENS)):   # which sequence, should the whole compare ever fail
        assert torch.equal(_bits(runs[0][0][r0:r0 + n]), _bits(wo[r0:r0 + n])), b


def test_attn_fwd_ragged_sequences_in_any_order(gpu, packed):
    """The metadata lists the sequences in another order than they lie in the buffers (and leaves one out): the rows
    of a listed sequence are the same, the rows of the one left out keep the sentinel."""
    qkv, ckv, want = packed
    R = sum(LENS)
    order = [4, 0, 5, 2, 1]   # without sequence 3
    st, cst = _starts(LENS), _starts(CAP_LENS)
    o = torch.full((R + SPARE, E), SENT, dtype=torch.bfloat16, device=gpu)
    ops.attn_fwd_ragged(qkv[:, :E], ckv[:, :E], ckv[:, E:], _i32([st[b] for b in order], gpu),
                        _i32([LENS[b] for b in order], gpu), _i32([cst[b] for b in order], gpu),
                        _i32([CAP_LENS[b] for b in order], gpu), H, max(LENS), max(CAP_LENS), False, o=o[:R])
    wo = want[False][0].clone()
    wo[st[3]:st[3] + LENS[3]] = SENT
    assert torch.equal(_bits(o), _bits(wo))


def test_attn_fwd_ragged_argument_errors(gpu, packed):
    qkv, ckv, _ = packed
    qs, ql = _i32(_starts(LENS), gpu), _i32(LENS, gpu)
    q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    with pytest.raises(ValueError):
        ops.attn_fwd_ragged(q, k, v, qs, ql, qs, ql, H, 0, 130, True)              # no bound to size the grid from
    with pytest.raises(ValueError):
        ops.attn_fwd_ragged(q, k, v, qs, ql, qs, ql, H, 400, 130, True)            # a bound past the packed rows
    with pytest.raises(ValueError):
        ops.attn_fwd_ragged(qkv[:, 4:E + 4], k, v, qs, ql, qs, ql, H, 130, 130, True)   # q not 16-byte aligned
    with pytest.raises(ValueError):
        ops.attn_fwd_ragged(q, k, v, qs, ql, qs, ql, 7, 130, 130, True)            # ld 3E < H·64


def _guarded(shape, dtype, gpu, guard=4096):
    n = int(np.prod(shape))
    big = torch.full((guard + n + guard,), SENT, dtype=dtype, device=gpu)
    return big, big[guard:guard + n].view(*shape)


def test_rows_to_slots(gpu):
    """K | V rows of three packed sequences into slots (2, 0, 3) of a sentinel-filled [4][32][2E] cache with guard
    regions on both sides; then device metadata gone wrong: slots outside the cache write nothing, and a length past
    the slot's rows stops at the slot's last row."""
    lens, slots = (5, 12, 13), (2, 0, 3)
    st = _starts(lens)
    g = torch.Generator().manual_seed(5)
    src = torch.randn(48, 3 * E, generator=g).to(torch.bfloat16).to(gpu)
    big, cache = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    ops.rows_to_slots(src[:, E:], _i32(st, gpu), _i32(lens, gpu), _i32(slots, gpu), max(lens), cache)
    want_big, want = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    for r0, n, s in zip(st, lens, slots):
        want[s, :n] = src[r0:r0 + n, E:]
    assert torch.equal(_bits(big), _bits(want_big))
    assert (cache[1] == SENT).all().item()
    # slots 7 and -1 lie outside the cache: only the first sequence is written
    big, cache = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    ops.rows_to_slots(src[:, E:], _i32(st, gpu), _i32(lens, gpu), _i32((2, 7, -1), gpu), max(lens), cache)
    want_big, want = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    want[2, :5] = src[:5, E:]
    assert torch.equal(_bits(big), _bits(want_big))
    # 40 rows for a slot of 32, and a wild length and start: the copies stop at the slot's and the source's ends
    big, cache = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    ops.rows_to_slots(src[:, E:], _i32((0, 10 ** 9), gpu), _i32((40, 10 ** 9), gpu), _i32((1, 3), gpu), 40, cache)
    want_big, want = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    want[1] = src[:32, E:]
    want[3] = src[16:48, E:]   # the length clamps to 32 rows, the start to the last 32 rows of the source
    assert torch.equal(_bits(big), _bits(want_big))


def test_rows_to_slots_logit_rows(gpu):
    """f32 rows, one per slot: the admission's logits rows."""
    src = torch.randn(3, 512, generator=torch.Generator().manual_seed(6)).to(gpu)
    big, logits = _guarded((4, 512), torch.float32, gpu)
    ones, iota = _i32((1, 1, 1), gpu), _i32((0, 1, 2), gpu)
    ops.rows_to_slots(src, iota, ones, _i32((2, 0, 3), gpu), 1, logits)
    want_big, want = _guarded((4, 512), torch.float32, gpu)
    want[2], want[0], want[3] = src[0], src[1], src[2]
    assert torch.equal(_bits(big), _bits(want_big))
    with pytest.raises(ValueError):
        ops.rows_to_slots(src[:, :510], iota, ones, iota, 1, logits[:, :510])   # rows of 2,040 bytes: not 16-byte pieces


def test_embed_packed_is_bitwise_embed_fwd(gpu):
    """A sequence with features, one without, and one of length 1 (only the visual row applies); ids outside the
    vocabulary add zeros as in ergm_embed_fwd.  Token rows and caption rows, bitwise."""
    V, P = 500, 64
    g = torch.Generator().manual_seed(8)
    wte, wpe = torch.randn(V, E, generator=g).to(gpu), torch.randn(P, E, generator=g).to(gpu)
    lens, caps, has = (5, 12, 1), (7, 12, 3), (1, 0, 1)
    ids = torch.randint(0, V, (sum(lens),), generator=g).to(gpu)
    tt = torch.randint(0, V, (sum(lens),), generator=g).to(gpu)
    cids = torch.randint(0, V, (sum(caps),), generator=g).to(gpu)
    ids[3], tt[7], cids[2], cids[9] = V, -1, -1, V + 5
    vis, aud = torch.randn(3, E, generator=g).to(gpu), torch.randn(3, E, generator=g).to(gpu)
    st, cst = _starts(lens), _starts(caps)
    h, cap = ops.embed_packed(ids, tt, cids, wte, wpe, _i32(st, gpu), _i32(lens, gpu), _i32(cst, gpu), _i32(caps, gpu),
                              max(lens), max(caps), vis, aud, torch.tensor(has, dtype=torch.uint8, device=gpu))
    for b, (r0, n, c0, c) in enumerate(zip(st, lens, cst, caps)):
        i = ids[r0:r0 + n].view(1, -1)
        v, a = (vis[b:b + 1], aud[b:b + 1]) if has[b] else (None, None)
        hb, _ = ops.embed_fwd(i, tt[r0:r0 + n].view(1, -1), i, wte, wpe, v, a)
        ci = cids[c0:c0 + c].view(1, -1)
        _, cb = ops.embed_fwd(ci, None, ci, wte, wpe)
        assert torch.equal(_bits(h[r0:r0 + n]), _bits(hb)), b
        assert torch.equal(_bits(cap[c0:c0 + c]), _bits(cb)), b
    # no features at all, no token types
    h2, cap2 = ops.embed_packed(ids, None, cids, wte, wpe, _i32(st, gpu), _i32(lens, gpu), _i32(cst, gpu), _i32(caps, gpu),
                                max(lens), max(caps))
    i = ids[st[1]:st[1] + lens[1]].view(1, -1)
    hb, _ = ops.embed_fwd(i, None, i, wte, wpe)
    assert torch.equal(_bits(h2[st[1]:st[1] + lens[1]]), _bits(hb)) and torch.equal(_bits(cap2), _bits(cap))


@pytest.mark.parametrize("V", [500, 5000, 50257])
def test_topp_sample_rows(gpu, V):
    """At the identity mapping (row_ids = 0 .. B-1, every row_steps = step) all four outputs are ergm_topp_sample's;
    with permuted row_ids, row b draws what the old kernel draws for row row_ids[b] on the same logits."""
    logits = torch.from_numpy(DO._logits(V)).to(gpu)
    B, seed, EOS = logits.shape[0], DO.SEEDS[V], DO.EOS
    fin0 = [0, 0, 0, 0, 1]

    def outs():
        return (torch.tensor(fin0, dtype=torch.uint8, device=gpu), torch.full((B,), -1, dtype=torch.int32, device=gpu),
                torch.full((B,), -1.0, dtype=torch.float32, device=gpu))

    for top_p in (DO.TOP_P, 1.0):
        for step in (0, 3):
            fa, ka, ma = outs()
            ta = ops.topp_sample(logits, V, top_p, seed, step, EOS, finished=fa, kept=ka, kept_mass=ma)
            fb, kb, mb = outs()
            tb = ops.topp_sample_rows(logits, V, top_p, seed, _i32(range(B), gpu), _i32([step] * B, gpu), EOS, finished=fb,
                                      kept=kb, kept_mass=mb)
            assert torch.equal(ta, tb) and torch.equal(fa, fb) and torch.equal(ka, kb)
            assert torch.equal(_bits(ma), _bits(mb))
            # rows permuted, ids with them: the draw follows the id, not the row; the steps differ per row too
            perm = [3, 0, 4, 1, 2]
            steps = [step + 5 * r for r in range(B)]
            old = []
            for r in range(B):   # the old kernel's draw of row r at step steps[r]
                f = torch.tensor(fin0, dtype=torch.uint8, device=gpu)
                old.append((int(ops.topp_sample(logits, V, top_p, seed, steps[r], EOS, finished=f)[r]), int(f[r])))
            fp = torch.tensor([fin0[r] for r in perm], dtype=torch.uint8, device=gpu)
            tp = ops.topp_sample_rows(logits[perm].contiguous(), V, top_p, seed, _i32(perm, gpu),
                                      _i32([steps[r] for r in perm], gpu), EOS, finished=fp)
            assert tp.tolist() == [old[r][0] for r in perm]
            assert fp.tolist() == [old[r][1] for r in perm]
    # a uint32 id above 2^31 travels as the same bits
    big = _i32([-(2 ** 31) + 5] * B, gpu)   # 0x80000005
    t1 = ops.topp_sample_rows(logits, V, 1.0, seed, big, _i32([0] * B, gpu), EOS)
    t2 = ops.topp_sample_rows(logits, V, 1.0, seed, big, _i32([0] * B, gpu), EOS)
    assert torch.equal(t1, t2)
    with pytest.raises(ValueError):
        from ergm_amd import _lib as L
        L.call("ergm_topp_sample_rows", ops._ptr(logits), logits.stride(0), B, V, 1.0, seed, None, None, None, EOS,
               ops._ptr(t1), None, None, None)
