"""The kernels of an extension against the kernels they extend, bitwise: ergm_attn_fwd_extend (packed new queries over
a cache that holds a past) against rows past .. of ergm_attn_fwd on every sequence alone and against
ergm_attn_fwd_ragged where there is no past; ergm_rows_to_slots_at against the source rows and ergm_rows_to_slots."""
import pytest
import torch

from test_gpu_ragged_ops import E, H, SENT, SPARE, _bits, _guarded, _i32, _starts
from ergm_amd import ops

pytestmark = pytest.mark.gpu
# (past, new): the past one below, at and one above a tile edge (and none, and two tiles), the new rows inside one
# tile, filling one exactly, and crossing one and two edges
PAIRS = ((0, 65), (1, 1), (63, 2), (64, 64), (65, 130), (130, 63))
NEW = tuple(n for _, n in PAIRS)
SLOTS = (5, 2, 7, 0, 3, 6)      # of eight: two caches of [4 slots][256 rows][2E] back to back in one buffer
N_SLOTS, SLOT_ROWS = 8, 256


@pytest.fixture(scope="module")
def cached(gpu):
    """The caches (sentinel-filled, every sequence's K | V rows 0 .. past + new - 1 in its slot), the packed new
    queries, and, computed once, rows past .. of ergm_attn_fwd(B = 1, causal) of every sequence alone."""
    g = torch.Generator().manual_seed(11)
    R = sum(NEW)
    assert R == 325
    cache = torch.full((N_SLOTS, SLOT_ROWS, 2 * E), SENT, dtype=torch.bfloat16, device=gpu)
    q = torch.empty(R, E, dtype=torch.bfloat16, device=gpu)
    want = torch.full((R + SPARE, E), SENT, dtype=torch.bfloat16, device=gpu)
    for (past, n), r0, s in zip(PAIRS, _starts(NEW), SLOTS):
        Lk = past + n
        qf = torch.randn(Lk, E, generator=g).to(torch.bfloat16).to(gpu)      # the rows below `past` are another turn's
        kv = torch.randn(Lk, 2 * E, generator=g).to(torch.bfloat16).to(gpu)
        cache[s, :Lk] = kv
        q[r0:r0 + n] = qf[past:]
        ob, _ = ops.attn_fwd(qf, kv[:, :E], kv[:, E:], 1, H, Lk, Lk, True)
        want[r0:r0 + n] = ob[past:]
    torch.cuda.synchronize()
    return cache, q, want


def _meta(order, gpu):
    st = _starts(NEW)
    return (_i32([st[b] for b in order], gpu), _i32([NEW[b] for b in order], gpu),
            _i32([SLOTS[b] * SLOT_ROWS for b in order], gpu), _i32([sum(PAIRS[b]) for b in order], gpu))


def _run(cache, q, order, gpu):
    R = sum(NEW)
    flat = cache.view(N_SLOTS * SLOT_ROWS, 2 * E)
    o = torch.full((R + SPARE, E), SENT, dtype=torch.bfloat16, device=gpu)
    qs, ql, ks, kl = _meta(order, gpu)
    ops.attn_fwd_extend(q, flat[:, :E], flat[:, E:], qs, ql, ks, kl, H, max(NEW), max(sum(p) for p in PAIRS), o=o[:R])
    return o


def test_attn_fwd_extend_is_bitwise_attn_fwd_rows(gpu, cached):
    """Six sequences in one launch, their slots out of order; the output buffer, sentinel-filled and with spare rows
    behind row 325, is compared whole with rows past .. of the per-sequence ergm_attn_fwd; two runs give equal bits."""
    cache, q, want = cached
    runs = [_run(cache, q, range(len(PAIRS)), gpu) for _ in range(2)]
    for o in runs:
        assert torch.equal(_bits(o), _bits(want))
    for b, (r0, n) in enumerate(zip(_starts(NEW), NEW)):   # which sequence, should the whole compare ever fail
        assert torch.equal(_bits(runs[0][r0:r0 + n]), _bits(want[r0:r0 + n])), PAIRS[b]


def test_attn_fwd_extend_sequences_in_any_order(gpu, cached):
    """The metadata lists the sequences in another order than they lie in the query buffer and leaves one out: the rows
    of a listed sequence are the same, the rows of the one left out keep the sentinel."""
    cache, q, want = cached
    o = _run(cache, q, [4, 0, 5, 2, 1], gpu)   # without sequence 3
    wo = want.clone()
    st = _starts(NEW)
    wo[st[3]:st[3] + NEW[3]] = SENT
    assert torch.equal(_bits(o), _bits(wo))


def test_attn_fwd_extend_without_a_past_is_attn_fwd_ragged(gpu):
    lens = (1, 2, 63, 64, 65, 130)
    R = sum(lens)
    qkv = torch.randn(R, 3 * E, generator=torch.Generator().manual_seed(12)).to(torch.bfloat16).to(gpu)
    qs, ql = _i32(_starts(lens), gpu), _i32(lens, gpu)
    q, k, v = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    o = torch.full((R + SPARE, E), SENT, dtype=torch.bfloat16, device=gpu)
    w = torch.full((R + SPARE, E), SENT, dtype=torch.bfloat16, device=gpu)
    ops.attn_fwd_extend(q, k, v, qs, ql, qs, ql, H, max(lens), max(lens), o=o[:R])
    ops.attn_fwd_ragged(q, k, v, qs, ql, qs, ql, H, max(lens), max(lens), True, o=w[:R])
    assert torch.equal(_bits(o), _bits(w))


def test_attn_fwd_extend_metadata_gone_wrong(gpu):
    """Device metadata the host checks never saw: k_len < q_len, starts past the buffers, lengths of 10^9.  Every value
    is clamped before an address is formed, so only the rows inside the clamped ranges change, guard regions on both
    sides of the output included, and what is written there is the attention over the clamped ranges."""
    Rq, Rk, max_q, max_k = 96, 160, 40, 100
    g = torch.Generator().manual_seed(13)
    q = torch.randn(Rq, E, generator=g).to(torch.bfloat16).to(gpu)
    kv = torch.randn(Rk, 2 * E, generator=g).to(torch.bfloat16).to(gpu)

    def run(qs, ql, ks, kl):
        big, o = _guarded((Rq, E), torch.bfloat16, gpu)
        ops.attn_fwd_extend(q, kv[:, :E], kv[:, E:], _i32(qs, gpu), _i32(ql, gpu), _i32(ks, gpu), _i32(kl, gpu), H, max_q,
                            max_k, o=o)
        return big, o

    def expect(rows):   # (first query row, n, first key row, Sk) after the clamps
        big, o = _guarded((Rq, E), torch.bfloat16, gpu)
        for q0, n, k0, Sk in rows:
            qf = torch.zeros(Sk, E, dtype=torch.bfloat16, device=gpu)
            qf[Sk - n:] = q[q0:q0 + n]
            ob, _ = ops.attn_fwd(qf, kv[k0:k0 + Sk, :E], kv[k0:k0 + Sk, E:], 1, H, Sk, Sk, True)
            o[q0:q0 + n] = ob[Sk - n:]
        return big

    # k_len < q_len: q_len clamps to k_len (10 rows, no past); and a negative length: nothing
    big, _ = run((0, 50), (30, -5), (0, 20), (10, 60))
    assert torch.equal(_bits(big), _bits(expect([(0, 10, 0, 10)])))
    # starts past the buffers (and below them): clamped so that the rows stay inside
    big, _ = run((10 ** 9, -7), (8, 4), (10 ** 9, -(10 ** 9)), (70, 9))
    assert torch.equal(_bits(big), _bits(expect([(Rq - 8, 8, Rk - 70, 70), (0, 4, 0, 9)])))
    # lengths of 10^9: the host bounds max_q / max_k hold
    big, _ = run((20,), (10 ** 9,), (30,), (10 ** 9,))
    assert torch.equal(_bits(big), _bits(expect([(20, max_q, 30, max_k)])))


def test_attn_fwd_extend_argument_errors(gpu, cached):
    cache, q, _ = cached
    flat = cache.view(N_SLOTS * SLOT_ROWS, 2 * E)
    k, v = flat[:, :E], flat[:, E:]
    qs, ql, ks, kl = _meta(range(len(PAIRS)), gpu)
    with pytest.raises(ValueError):
        ops.attn_fwd_extend(q, k, v, qs, ql, ks, kl, H, 0, 195)                     # no bound to size the grid from
    with pytest.raises(ValueError):
        ops.attn_fwd_extend(q, k, v, qs, ql, ks, kl, H, 400, 195)                   # a bound past the packed rows
    with pytest.raises(ValueError):
        ops.attn_fwd_extend(q, flat[:, 4:E + 4], v, qs, ql, ks, kl, H, 130, 195)    # k not 16-byte aligned
    with pytest.raises(ValueError):
        ops.attn_fwd_extend(q, k, v, qs, ql, ks, kl, 5, 130, 195)                   # leading dims below H·64


def test_rows_to_slots_at(gpu):
    """K | V rows of three packed sequences to rows dst_row0 .. of slots (2, 0, 3) of a sentinel-filled [4][32][2E]
    cache with guard regions on both sides; a dst_row0 + len past the slot stops at the slot's last row; a slot outside
    the cache writes nothing; with dst_row0 = 0 the result is ergm_rows_to_slots'."""
    lens, slots, at = (5, 12, 13), (2, 0, 3), (3, 20, 0)
    st = _starts(lens)
    src = torch.randn(48, 3 * E, generator=torch.Generator().manual_seed(14)).to(torch.bfloat16).to(gpu)
    big, cache = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    ops.rows_to_slots_at(src[:, E:], _i32(st, gpu), _i32(lens, gpu), _i32(slots, gpu), _i32(at, gpu), max(lens), cache)
    want_big, want = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    for r0, n, s, d in zip(st, lens, slots, at):
        want[s, d:d + n] = src[r0:r0 + n, E:]
    assert torch.equal(_bits(big), _bits(want_big))
    # 13 rows from row 25 of a slot of 32: 7 land; a first row at, past and below the slot: none, none, from row 0;
    # slots 7 and -1 lie outside the cache
    big, cache = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    ops.rows_to_slots_at(src[:, E:], _i32((0, 13, 13, 26, 0, 0), gpu), _i32((13, 4, 4, 5, 5, 5), gpu),
                         _i32((1, 0, 2, 3, 7, -1), gpu), _i32((25, 32, 10 ** 9, -4, 0, 0), gpu), 13, cache)
    want_big, want = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    want[1, 25:32] = src[0:7, E:]
    want[3, 0:5] = src[26:31, E:]
    assert torch.equal(_bits(big), _bits(want_big))
    # a wild length from row 8: the copy stops at the slot's end, the start clamps to the source's last 24 rows
    big, cache = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    ops.rows_to_slots_at(src[:, E:], _i32((10 ** 9,), gpu), _i32((10 ** 9,), gpu), _i32((2,), gpu), _i32((8,), gpu), 40, cache)
    want_big, want = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    want[2, 8:32] = src[24:48, E:]
    assert torch.equal(_bits(big), _bits(want_big))
    # dst_row0 = 0: ergm_rows_to_slots
    big, cache = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    ops.rows_to_slots_at(src[:, E:], _i32(st, gpu), _i32(lens, gpu), _i32(slots, gpu), _i32((0, 0, 0), gpu), max(lens), cache)
    old_big, old = _guarded((4, 32, 2 * E), torch.bfloat16, gpu)
    ops.rows_to_slots(src[:, E:], _i32(st, gpu), _i32(lens, gpu), _i32(slots, gpu), max(lens), old)
    assert torch.equal(_bits(big), _bits(old_big))
