"""ergm_lm_score per element against fp64 (tests/_lmscore.py: cases, reference, bounds), through the C-ABI.

Buffers.  X is a [R, K] slice of a NaN-filled [R + 2, K + 8] buffer (rows at or past R and the pad columns hold NaN)
and W a [rows of W, K] slice of a NaN-filled buffer with ld = K + 8 whose rows at or past V hold 1e4 or NaN (the
vocabulary pad), so anything the kernel may not use shows up as NaN.  Every output and the workspace sit in sentinel
buffers that must be intact around the slice afterwards; the outputs hold NaN (top1: the sentinel) before the call and
nothing of the kind after it.  No element is excluded from any comparison.

What runs what: every case launches lm_score_kernel on a grid of ceil(R / BM) row tiles x ceil(V / PW) partitions and
lm_score_combine_kernel once.  V = 203: one partition of two column tiles, the second ragged; V = BN: one full tile;
BN + 1: a second tile of one column; PW + 1: a second partition of one column; 50257: 99 partitions, the last of 81
columns.  R = 1 .. 2*BM + 3 walks one ragged row tile to three, a ragged wave (15, 17, 33) and a ragged lane group.
"""
import ctypes as C

import pytest
import torch

import _lmscore as S
from ergm_amd import _lib as L
from ergm_amd import ops

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -12288.0
bf16, f32, i32, i64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
OUTS = ("logprob", "lse", "top1_logit", "top1")


class Out:
    """[n] of ``dtype`` at element 8 of a sentinel buffer, 24 elements of slack behind."""

    def __init__(self, n, dtype, gpu, init):
        self.n = n
        self.buf = torch.full((8 + n + 24,), SENT, dtype=dtype, device=gpu)
        self.view = self.buf[8:8 + n]
        self.view.fill_(init)

    def intact(self):
        b = self.buf.clone()
        b[8:8 + self.n] = SENT
        return bool((b == SENT).all().item())

    @property
    def ptr(self):
        return C.c_void_p(self.view.data_ptr())


def _operands(c, gpu):
    xb = torch.full((c.R + 2, c.K + 8), NAN, dtype=bf16, device=gpu)
    xb[:c.R, :c.K] = c.X.to(gpu)
    wb = torch.full((c.wrows, c.K + 8), NAN, dtype=bf16, device=gpu)
    wb[:, :c.K] = c.W.to(gpu)
    return xb, wb, c.targets.to(gpu)


def _launch(c, gpu, dev=None, rows=None, skip=()):
    """One call on rows ``rows`` (a slice; default all) of case ``c``.  Returns the CPU outputs by name (None for a
    name in ``skip``, passed as NULL)."""
    xb, wb, tg = dev or _operands(c, gpu)
    r0, r1 = (0, c.R) if rows is None else rows
    n = r1 - r0
    x, t = xb[r0:], tg[r0:r1].contiguous()
    outs = {k: None if k in skip else Out(n, i32 if k == "top1" else f32, gpu, SENT + 1 if k == "top1" else NAN)
            for k in OUTS}
    need = L.load().ergm_lm_score_workspace_size(n, c.V, c.K)
    assert need == (3 * S.parts(c.V) + 1) * n * 4
    ws = Out(need // 4, f32, gpu, NAN)
    L.call("ergm_lm_score", C.c_void_p(x.data_ptr()), x.stride(0), C.c_void_p(wb.data_ptr()), wb.stride(0),
           C.c_void_p(t.data_ptr()), n, c.V, c.K, *[outs[k].ptr if outs[k] else None for k in OUTS], ws.ptr, need,
           ops._stream(gpu))
    torch.cuda.synchronize()
    for k, o in list(outs.items()) + [("the workspace", ws)]:
        assert o is None or o.intact(), f"{c.name}: wrote outside {k}"
    return {k: None if o is None else o.view.cpu() for k, o in outs.items()}


def _check(c, got):
    r = S.ref(c)
    b = S.bounds(c, r)
    for k in ("logprob", "lse", "top1_logit"):
        assert torch.isfinite(got[k]).all().item(), f"{c.name}: NaN or inf in {k}"
    res = S.judge(c, r, b, got["logprob"], got["lse"], got["top1_logit"], got["top1"])
    print(f"{c.name}: err/bound " + "  ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert max(res.values()) <= 1.0, (c.name, res)
    unscored = ~r.valid
    assert (got["logprob"][unscored] == 0.0).all().item(), f"{c.name}: an unscored row's logprob is not exactly 0"
    return res


def _same(a, b):
    return all(torch.equal(a[k].view(i32), b[k].view(i32)) for k in OUTS if a[k] is not None and b[k] is not None)


@pytest.mark.parametrize("K", S.DEPTHS)
def test_matrix(gpu, K):
    """Every R x V of the matrix at depth K, benign data: all four outputs within their bounds on every row."""
    for R in S.ROWS:
        for vw in S.VOCABS:
            c = S.case(R, K, vw)
            _check(c, _launch(c, gpu))


@pytest.mark.parametrize("R", S.BIG_ROWS)
def test_gpt2_vocabulary(gpu, R):
    c = S.case(R, S.BIG_K, S.BIG)
    _check(c, _launch(c, gpu))


@pytest.mark.parametrize("args", list(S.family_cases()), ids=lambda a: f"{a[3]}{a[4]}-R{a[0]}-K{a[1]}-V{a[2][0]}")
def test_families(gpu, args):
    """wide (a missing rescale shows), peaked, edge (a maximum on every tile and partition boundary column, the target
    on the next) and tie (two identical rows of W: the lower column) at both family shapes."""
    c = S.case(*args)
    got = _launch(c, gpu)
    _check(c, got)
    for row, col in c.planted.items():
        assert int(got["top1"][row]) == col, (c.name, row, col, int(got["top1"][row]))


def test_unscored_targets_still_get_lse_and_top1(gpu):
    c = S.case(17, 192, (203, 208))
    kinds = {int(t) for t in c.targets if not 0 <= int(t) < c.V}
    assert kinds == {-100, c.V, c.V + 7}
    _check(c, _launch(c, gpu))  # lse and top1 of those rows are judged like every other row's


def test_same_bits_twice_and_null_outputs(gpu):
    for args in ((2 * S.BM + 3, 192, (S.PW + 1, S.PW + 8)), (33, S.BIG_K, S.BIG)):
        c = S.case(*args)
        dev = _operands(c, gpu)
        a = _launch(c, gpu, dev)
        assert _same(a, _launch(c, gpu, dev)), f"{c.name}: a second run differs"
        for skip in (("logprob",), ("lse", "top1"), ("top1_logit", "lse", "logprob"), OUTS):
            assert _same(a, _launch(c, gpu, dev, skip=skip)), f"{c.name}: NULL {skip} changed another output"


@pytest.mark.parametrize("K,vw", [(192, (S.PW + 1, S.PW + 8)), (768, (203, 208)), (1024, (S.BN + 1, S.BN + 8))])
def test_a_row_does_not_depend_on_its_neighbours(gpu, K, vw):
    """Row r of an R = 2*BM + 3 call is bitwise the R = 1 call on that row."""
    c = S.case(2 * S.BM + 3, K, vw)
    dev = _operands(c, gpu)
    full = _launch(c, gpu, dev)
    for r in (0, S.BM - 1, S.BM, 2 * S.BM + 2):
        one = _launch(c, gpu, dev, rows=(r, r + 1))
        for k in OUTS:
            assert torch.equal(full[k][r:r + 1].view(i32), one[k].view(i32)), (c.name, r, k)
