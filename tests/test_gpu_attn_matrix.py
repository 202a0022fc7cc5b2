"""ergm_attn_fwd / ergm_attn_bwd per element against fp64 (tests/_attn.py) at tile edges, through the C-ABI.

How a case runs (built on the CPU from a seeded generator, independent data per (b, h), operands rounded to bf16):
* q, k, v, dO and o_in are [rows][H*64] views at row 8 of wider NaN-filled buffers: causal cases carve q, k, v out of
  one [rows + 16][3*H*64 + 24] buffer (the fused projection's layout) at columns 8, 8 + H*64, 8 + 2*H*64; the others use
  one buffer each with rows of H*64 + 24 elements at column offsets 0, 8, 16.  A row or column the kernel may read but
  must not use shows up as a NaN in the output;
* O, dQ, dK, dV are [rows][H*64] views at row 8, column 8 of [rows + 16][H*64 + 24] buffers filled with a finite
  sentinel, the view itself NaN before the call; afterwards the surround must hold the sentinel bit for bit and the
  view no NaN (every row written);
* LSE, delta and the dropout keep bits are slices at element 8 of longer sentinel-filled flat buffers whose slack must
  be intact afterwards;
* the backward runs twice (bitwise equal), fed the reference's bf16 O / fp32 LSE and fed the kernel's own, the fp64
  reference recomputed from exactly what it was fed.
"""
import pytest
import torch

import _attn as A
from ergm_amd import _lib as L
from ergm_amd import ops

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -12288.0  # exact in bf16 and f32
SENT64 = 0x5A5A5A5A5A5A5A5A
bf16, f32 = torch.bfloat16, torch.float32


# ---- device-side plumbing -------------------------------------------------------------------------------------------
def _in_view(x, gpu, col):
    """The bf16 [rows][W] matrix x at row 8, column `col` of a NaN buffer with rows of W + 24 elements."""
    rows, W = x.shape
    buf = torch.full((rows + 16, W + 24), NAN, dtype=bf16)
    buf[8:8 + rows, col:col + W] = x
    return buf.to(gpu)[8:8 + rows, col:col + W]


def _out_view(rows, W, gpu):
    buf = torch.full((rows + 16, W + 24), SENT, dtype=bf16, device=gpu)
    view = buf[8:8 + rows, 8:8 + W]
    view.fill_(NAN)
    return buf, view


def _flat(n, gpu, fill=NAN, dtype=f32, sent=SENT):
    """n elements at element 8 of a flat sentinel buffer (24 elements of slack behind)."""
    buf = torch.full((8 + n + 24,), sent, dtype=dtype, device=gpu)
    view = buf[8:8 + n]
    if isinstance(fill, torch.Tensor):
        view.copy_(fill.reshape(-1))
    else:
        view.fill_(fill)
    return buf, view


def _intact(buf, view, sent=SENT):
    b = buf.clone()
    if b.dim() == 1:
        b[8:8 + view.numel()] = sent
    else:
        b[8:8 + view.shape[0], 8:8 + view.shape[1]] = sent
    return bool((b == sent).all().item())


def _bits(t):
    return t.view(torch.int16 if t.dtype == bf16 else torch.int32)


def device_inputs(c, gpu):
    W = c.H * 64
    q, k, v, do = (A.to_rows(t) for t in (c.q, c.k, c.v, c.do))
    if c.causal:  # q, k, v carved from one buffer
        rows = q.shape[0]
        buf = torch.full((rows + 16, 3 * W + 24), NAN, dtype=bf16)
        for i, t in enumerate((q, k, v)):
            buf[8:8 + rows, 8 + i * W:8 + (i + 1) * W] = t
        buf = buf.to(gpu)
        qd, kd, vd = (buf[8:8 + rows, 8 + i * W:8 + (i + 1) * W] for i in range(3))
        dod = _in_view(do, gpu, 0)
    else:
        qd, kd, vd, dod = _in_view(q, gpu, 0), _in_view(k, gpu, 8), _in_view(v, gpu, 16), _in_view(do, gpu, 8)
    drop = ops.dropout_desc(**c.drop) if c.drop else None
    return dict(q=qd, k=kd, v=vd, do=dod, drop=drop)


def run_fwd(c, dv, gpu):
    """ergm_attn_fwd into guarded buffers; returns CPU (O [B,H,Sq,64] bf16, LSE [B,H,Sq] f32, keep-bit slice on the
    GPU or None) and the raw buffers (for bitwise comparisons)."""
    B, H, Sq, Sk = c.B, c.H, c.Sq, c.Sk
    obuf, o = _out_view(B * Sq, H * 64, gpu)
    lbuf, lse = _flat(B * H * Sq, gpu)
    mbuf = bits = None
    if c.drop:
        mbuf, bits = _flat(B * H * Sq * ((Sk + 63) // 64), gpu, fill=0, dtype=torch.int64, sent=SENT64)
    q, k, v = dv["q"], dv["k"], dv["v"]
    L.call("ergm_attn_fwd", ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._ptr(o), ops._ptr(lse), B, H, Sq, Sk,
           q.stride(0), k.stride(0), v.stride(0), o.stride(0), int(c.causal), ops._dp(dv["drop"]), ops._ptr(bits),
           ops._stream(gpu))
    assert _intact(obuf, o), f"{c.name}: wrote outside O[:, :H*64]"
    assert _intact(lbuf, lse), f"{c.name}: wrote outside LSE[B, H, Sq]"
    assert mbuf is None or _intact(mbuf, bits, SENT64), f"{c.name}: wrote outside the keep bits"
    return A.from_rows(o.cpu(), B, H), lse.cpu().view(B, H, Sq), bits, (obuf, lbuf)


def run_bwd(c, dv, gpu, o_in, lse_in, bits=None):
    """ergm_attn_bwd on guarded buffers, fed o_in [B,H,Sq,64] bf16 / lse_in [B,H,Sq] f32 (CPU); returns CPU dQ, dK, dV
    [B,H,S,64], delta [B,H,Sq] (NaN where the short kernel keeps it in LDS) and the raw buffers."""
    B, H, Sq, Sk = c.B, c.H, c.Sq, c.Sk
    od = _in_view(A.to_rows(o_in), gpu, 16 if not c.causal else 8)
    lbuf, lse = _flat(B * H * Sq, gpu, fill=lse_in.to(gpu))
    dbuf, delta = _flat(B * H * Sq, gpu)
    qb, dq = _out_view(B * Sq, H * 64, gpu)
    kb, dk = _out_view(B * Sk, H * 64, gpu)
    vb, dvv = _out_view(B * Sk, H * 64, gpu)
    ops.attn_bwd(dv["q"], dv["k"], dv["v"], od, dv["do"], lse, B, H, Sq, Sk, c.causal, dq=dq, dk=dk, dv=dvv,
                 dropout=dv["drop"], keep_bits=bits, delta=delta)
    for what, buf, view in (("dQ", qb, dq), ("dK", kb, dk), ("dV", vb, dvv), ("delta", dbuf, delta)):
        assert _intact(buf, view), f"{c.name}: wrote outside {what}"
    assert torch.equal(lse.cpu(), lse_in.reshape(-1)) and _intact(lbuf, lse), f"{c.name}: the backward wrote to LSE"
    return (A.from_rows(dq.cpu(), B, H), A.from_rows(dk.cpu(), B, H), A.from_rows(dvv.cpu(), B, H),
            delta.cpu().view(B, H, Sq), (qb, kb, vb))


def same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def check_bwd(what, c, got, rb, bb, family, tiled):
    for n, g in zip(("dQ", "dK", "dV"), got[:3]):
        A.check(what, n, g, getattr(rb, n), bb[n], family, gate=n not in A.ungated(c))
    if tiled:  # the tiled kernels leave delta in memory
        A.check(what, "delta", got[3], rb.delta, bb["delta"], family)


def backward_both_ways(c, dv, gpu, O, LSE, fed, family, tiled, bits=None, twice=True):
    """The backward fed the reference's O / LSE (`fed` = case_bwd_ref_fed) and fed the kernel's own, each within its own
    reference's bound and, run twice, bitwise the same; `tiled`: the tiled kernels run (they leave delta in memory).
    Returns the raw buffers of both."""
    raws = []
    feeds = (("fed the reference", fed), ("fed its own O, LSE", (O, LSE) + A.case_bwd(c, O, LSE)))
    for tag, (o_in, lse_in, rb, bb) in feeds:
        got = run_bwd(c, dv, gpu, o_in, lse_in, bits)
        check_bwd(f"{c.name} backward {tag}", c, got, rb, bb, family, tiled)
        if twice:
            again = run_bwd(c, dv, gpu, o_in, lse_in, bits)
            assert same_bits(got[4], again[4]), f"{c.name} {tag}: not bitwise repeatable"
        raws.append(got[4])
    return raws


def _short(c):
    """ergm_attn_bwd takes attn_bwd_short_kernel for this case unless ergm_attn_tune forces the tiled pair."""
    return c.Sq <= 128 and c.Sk <= 128


@pytest.fixture
def tune():
    """ergm_attn_tune for the test, reset to the defaults afterwards."""
    def force(v):
        L.call("ergm_attn_tune", v)
    try:
        yield force
    finally:
        L.load().ergm_attn_tune(0)


def _ids(cases):
    return [A.case_id(*x) for x in cases]


# ---- every length, benign inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk,causal,bh", A.LENGTHS, ids=_ids(A.LENGTHS))
def test_lengths(gpu, tune, Sq, Sk, causal, bh):
    """Forward and backward at every length around the 16-row wave, the 64-row tile and the 128 / 129 switch between
    the short backward and the tiled pair (one of Sq, Sk crossing it alone included), Sq = 1 and Sk = 1, with B*H
    rotating over 1, 6 and the two XCD-remapped 8s; for Sq, Sk <= 128 the tiled backward too, bitwise the short one."""
    c, r, bf = A.case_fwd(Sq, Sk, causal, bh)
    fed = A.case_bwd_ref_fed(Sq, Sk, causal, bh)
    dv = device_inputs(c, gpu)
    O, LSE, _, _ = run_fwd(c, dv, gpu)
    A.check(c.name, "O", O, r.O, bf["O"], "benign")
    A.check(c.name, "LSE", LSE, r.LSE, bf["LSE"], "benign")
    raws = backward_both_ways(c, dv, gpu, O, LSE, fed, "benign", tiled=not _short(c))
    if _short(c):
        tune(1)
        forced = backward_both_ways(c, dv, gpu, O, LSE, fed, "benign, tiled forced", tiled=True, twice=False)
        for a, b in zip(raws, forced):
            assert same_bits(a, b), f"{c.name}: the tiled backward differs from the short kernel's"


# ---- ring stages ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk,causal,bh", A.RING_SHAPES, ids=_ids(A.RING_SHAPES))
def test_ring_stages(gpu, tune, Sq, Sk, causal, bh):
    """2, 3 and 4 ring stages of the three tiled kernels on 5-tile loops (a 4-stage ring wraps): within the bound and
    bitwise the same O, LSE, dQ, dK, dV (the stage count does not enter the arithmetic)."""
    c, r, bf = A.case_fwd(Sq, Sk, causal, bh)
    fed = A.case_bwd_ref_fed(Sq, Sk, causal, bh)
    dv = device_inputs(c, gpu)
    seen = []
    for ns in (2, 3, 4):
        tune(1 | ns << 4)
        O, LSE, _, fraw = run_fwd(c, dv, gpu)
        A.check(f"{c.name} ns {ns}", "O", O, r.O, bf["O"], "ring stages")
        A.check(f"{c.name} ns {ns}", "LSE", LSE, r.LSE, bf["LSE"], "ring stages")
        got = run_bwd(c, dv, gpu, fed[0], fed[1])
        check_bwd(f"{c.name} ns {ns}", c, got, fed[2], fed[3], "ring stages", True)
        seen.append(fraw + got[4])
    for ns, s in zip((3, 4), seen[1:]):
        assert same_bits(seen[0], s), f"{c.name}: {ns} ring stages differ from 2"


def test_ring_stage_count_is_validated(gpu, tune):
    for ns in (1, 5):
        with pytest.raises(ValueError):
            tune(1 | ns << 4)


# ---- input families -------------------------------------------------------------------------------------------------
FAMILY_CASES = [s + (f,) for s in A.FAMILY_SHAPES for f in A.FAMILIES]


@pytest.mark.parametrize("Sq,Sk,causal,bh,family", FAMILY_CASES, ids=_ids(FAMILY_CASES))
def test_input_families(gpu, Sq, Sk, causal, bh, family):
    """Peaked softmax (q, k x4, x8), a maximum that arrives in the last key tile / sits at key 0, a flat softmax
    (Q = 0: LSE = log(visible keys), O the running mean of V) and one-hot routing (O[i] = V[pi(i)] exactly)."""
    c, r, bf = A.case_fwd(Sq, Sk, causal, bh, family)
    fed = A.case_bwd_ref_fed(Sq, Sk, causal, bh, family)
    dv = device_inputs(c, gpu)
    O, LSE, _, _ = run_fwd(c, dv, gpu)
    A.check(c.name, "O", O, r.O, bf["O"], family)
    A.check(c.name, "LSE", LSE, r.LSE, bf["LSE"], family)
    if family == "routing":
        want = torch.gather(c.v, 2, c.pi[..., None].expand(c.B, c.H, Sq, 64))
        assert torch.equal(_bits(O.contiguous()), _bits(want.contiguous())), f"{c.name}: O[i] != V[pi(i)]"
    backward_both_ways(c, dv, gpu, O, LSE, fed, family, tiled=not _short(c), twice=False)


# ---- dropout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk,causal,bh", A.DROP_SHAPES, ids=_ids(A.DROP_SHAPES))
def test_dropout(gpu, tune, Sq, Sk, causal, bh):
    """p = 0.1 with a non-zero site and offset: the stored keep bits are the Philox mask on every visible pair, the
    forward and both backward feeds fit the bound; S = 1024 is the limit of the keep-bit staging in LDS."""
    args = (Sq, Sk, causal, bh, "benign", 1.0, True)
    c, r, bf = A.case_fwd(*args)
    fed = A.case_bwd_ref_fed(*args)
    dv = device_inputs(c, gpu)
    O, LSE, bits, _ = run_fwd(c, dv, gpu)
    stored = ops.unpack_bits(bits.cpu().view(c.B * c.H * Sq, -1), Sk, 64).view(c.B, c.H, Sq, Sk)
    vis = c.vis.expand(c.B, c.H, Sq, Sk)
    assert torch.equal(stored[vis], c.keep[vis]), f"{c.name}: stored keep bits differ from the Philox mask"
    A.check(c.name, "O", O, r.O, bf["O"], "dropout")
    A.check(c.name, "LSE", LSE, r.LSE, bf["LSE"], "dropout")
    raws = backward_both_ways(c, dv, gpu, O, LSE, fed, "dropout", tiled=not _short(c), bits=bits, twice=False)
    if _short(c):
        tune(1)
        forced = backward_both_ways(c, dv, gpu, O, LSE, fed, "dropout, tiled forced", tiled=True, bits=bits,
                                    twice=False)
        for a, b in zip(raws, forced):
            assert same_bits(a, b), f"{c.name}: the tiled backward differs from the short kernel's"


@pytest.mark.parametrize("Sq,Sk,causal", [(1025, 1025, True), (1025, 64, False), (64, 1025, False)])
def test_dropout_past_the_limit_is_rejected(gpu, Sq, Sk, causal):
    """Sq or Sk = 1025 with dropout: ValueError from attn_fwd and attn_bwd (nothing is launched); fine without."""
    d = ops.dropout_desc(**A.DROP)
    q = torch.zeros(Sq, 64, dtype=bf16, device=gpu)
    k = torch.zeros(Sk, 64, dtype=bf16, device=gpu)
    with pytest.raises(ValueError):
        ops.attn_fwd(q, k, k, 1, 1, Sq, Sk, causal, dropout=d)
    o, lse = ops.attn_fwd(q, k, k, 1, 1, Sq, Sk, causal)
    bits = torch.zeros(Sq, (Sk + 63) // 64, dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError):
        ops.attn_bwd(q, k, k, o, q, lse, 1, 1, Sq, Sk, causal, dropout=d, keep_bits=bits)


def test_worst_ratios(gpu):
    """Prints the worst err/bound per family and output that this session's tests saw."""
    for fam in sorted(A.WORST):
        A.report(fam)
