"""LayerNorm, cross-entropy, the emotion head, ergm_loss_finalize and ergm_colsum per element against fp64
(tests/_rows.py: cases, references, bounds), through the C-ABI.

Buffers.  Every float input is a slice at element 8 of a NaN-filled buffer (a column slice of a wider NaN matrix where
the entry point takes a leading dimension): a row or column the kernel may read but must not use shows up as NaN.  Every
output is a slice of a buffer filled with a finite sentinel, the slice itself NaN (or the in/out value) before the
call; afterwards the surround holds the sentinel bit for bit and the slice no NaN where the operation must write.  The
offsets keep 16-byte alignment (8 bytes for the bf16x4 rows of ergm_colsum); no test passes a misaligned or undersized
pointer, and arguments that must be refused are given buffers large enough for the shape they name.

Which case launches which instantiation:
* ln_fwd_kernel<NV> / ln_bwd_kernel<NV, false> (f32 dy: "f32", "f32-drop", "f32-nob") / ln_bwd_kernel<NV, true> (bf16
  dy: "bf16", "bf16-drop", "bf16-dropres"): test_layernorm[E] with NV = 1 at E = 4, 64, 252, 256; NV = 2 at 260, 512;
  NV = 3 at 516, 768; NV = 4 at 772, 1024 (252, 260, 516, 772: a ragged last column group).  "bf16-dropres" is
  drop_res = 1 with no dres_bf16 (the embedding slot's form), test_layernorm_long runs ln_param_reduce_kernel's second
  round (258 partial rows), ergm_layernorm_fwd_ld runs in every case with ldy = E + 8.
* xent_kernel<N, false> (ergm_xent_fwd_bwd) and xent_kernel<N, true> (ergm_xent_compact), both in every test_xent case:
  N = 2 at ldl = 208, 4096; 4 at 8200 (3 chunk sets, the last one thread wide); 8 at 16392 (5 sets) and 32768; 13 at
  50304; 16 at 53256 (14 sets) and 65536.  Every shape runs benign logits in both label layouts and the ``edge`` parts,
  which put a scored row's maximum on every column of xe_edges(V): V-1, 0 and both sides of every 4096-column stripe
  boundary below V-1 (5 columns at V = 8193, 28 at 53250, 32 at 65536: every chunk set of xent_kernel<16>).
* emotion_row_kernel / emotion_dw_kernel: test_emotion_head, every B = 1, 15, 16, 17, 33 x C = 1, 7, 16 x E = 64, 100,
  768, 1024 x S = 1, 8; loss_finalize_kernel: test_loss_finalize, T = 1, 255, 256, 257, 2049.
* colsum_partial_kernel<false / true> direct (rows <= 64) and with colsum_final_kernel (65, 130): test_colsum.
"""
import ctypes as C

import pytest
import torch

import _rows as R
from ergm_amd import _lib as L
from ergm_amd import ops

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -12288.0  # exact in bf16, f32 and int32
bf16, f32, i32, i64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
P, ST = ops._ptr, ops._stream


class Guard:
    """[rows, cols] with row stride ``ld`` at element ``off`` of a flat sentinel buffer (24 elements of slack behind);
    the slice holds ``init`` (a value or a CPU tensor) before the call."""

    def __init__(self, rows, cols, dtype, gpu, init=NAN, ld=None, off=8, fill=SENT):
        self.ld = cols if ld is None else ld
        self.rows, self.cols, self.off, self.fill = rows, cols, off, fill
        self.buf = torch.full((off + rows * self.ld + 24,), fill, dtype=dtype, device=gpu)
        self.view = self._slice(self.buf)
        if isinstance(init, torch.Tensor):
            self.view.copy_(init.reshape(rows, cols))
        else:
            self.view.fill_(init)

    def _slice(self, buf):
        return buf[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def intact(self):
        b = self.buf.clone()
        self._slice(b).fill_(self.fill)
        return bool((b == self.fill).all().item())

    def cpu(self):
        return self.view.cpu()

    @property
    def ptr(self):
        return C.c_void_p(self.view.data_ptr())


def _in(t, gpu, ld=None, off=8):
    """The CPU tensor ``t`` ([rows, cols] or 1-D) inside a NaN-filled buffer; returns the device view."""
    t2 = t.reshape(1, -1) if t.dim() == 1 else t
    g = Guard(t2.shape[0], t2.shape[1], t.dtype, gpu, init=t2, ld=ld, off=off, fill=NAN)
    return g.view.view(-1) if t.dim() == 1 and ld is None else g.view


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dev_int(v, gpu):
    return torch.tensor([v], dtype=i32, device=gpu)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
def _ln_forward(c, dv, gpu, ldy=None):
    rows, E = c.rows, c.E
    y = Guard(rows, E, bf16, gpu, ld=ldy)
    mean, rstd = Guard(1, rows, f32, gpu), Guard(1, rows, f32, gpu)
    if ldy is None:
        L.call("ergm_layernorm_fwd", P(dv["x"]), P(dv["gamma"]), P(dv["beta"]), y.ptr, mean.ptr, rstd.ptr, rows, E, c.eps,
               ST(gpu))
    else:
        ops.layernorm_fwd_ld(dv["x"], dv["gamma"], dv["beta"], y.view, c.eps, mean=mean.view[0], rstd=rstd.view[0])
    for n, g in (("y", y), ("mean", mean), ("rstd", rstd)):
        assert g.intact(), f"{c.name}: wrote outside {n}" + (" (the pad columns of ldy = E + 8)" if ldy else "")
    return y.cpu(), mean.cpu()[0], rstd.cpu()[0]


def _ln_backward(c, dv, gpu, var, m_in, r_in, entry):
    """One backward launch of variant ``var`` through ``entry`` ("abi": ergm_layernorm_bwd, "ex": the new entry point, "ops": the same through ops.py),
    fed the CPU fp32 m_in / r_in.  Returns CPU dres, dres_bf16 (or None), dgamma, dbeta."""
    dyb, drop, drop_res, has_b = R.LN_BWD[var]
    rows, E = c.rows, c.E
    dres = Guard(rows, E, f32, gpu, init=c.dres0)
    db = Guard(rows, E, bf16, gpu) if has_b else None
    dg, dbe = Guard(1, E, f32, gpu), Guard(1, E, f32, gpu)
    md, rd = _in(m_in, gpu), _in(r_in, gpu)
    d = ops.dropout_desc(**R.LN_DROP) if drop else None
    wsb = L.load().ergm_layernorm_bwd_workspace_size(rows, E)
    ws = Guard(1, wsb // 4, f32, gpu)
    dy = dv["dyb"] if dyb else dv["dy"]
    if entry == "ops":  # the keyword wrapper (its own workspace)
        ops.layernorm_bwd_ex(dy, dv["x"], md, rd, dv["gamma"], dres.view, dres_bf16=db.view if has_b else None,
                             dgamma=dg.view[0], dbeta=dbe.view[0], dropout=d, drop_res=drop_res)
    elif entry == "abi":
        assert not dyb and not drop_res and has_b
        L.call("ergm_layernorm_bwd", P(dy), P(dv["x"]), P(md), P(rd), P(dv["gamma"]), dres.ptr, db.ptr, dg.ptr, dbe.ptr,
               ws.ptr, wsb, rows, E, ops._dp(d), ST(gpu))
    else:
        L.call("ergm_layernorm_bwd_ex", P(dy), L.BF16 if dyb else L.F32, P(dv["x"]), P(md), P(rd), P(dv["gamma"]), dres.ptr,
               db.ptr if has_b else None, dg.ptr, dbe.ptr, ws.ptr, wsb, rows, E, ops._dp(d), int(drop_res), ST(gpu))
    for n, g in (("dres", dres), ("dres_bf16", db), ("dgamma", dg), ("dbeta", dbe), ("the workspace", ws)):
        assert g is None or g.intact(), f"{c.name} {var}: wrote outside {n}"
    return dres.cpu(), db.cpu() if has_b else None, dg.cpu()[0], dbe.cpu()[0]


def _ln_run(c, gpu, key, variants=tuple(R.LN_BWD)):
    x64, g64, b64 = c.x.double(), c.gamma.double(), c.beta.double()
    r = R.ln_fwd_ref(x64, g64, b64, c.eps)
    bf = R.ln_fwd_bounds(x64, g64, b64, r)
    dv = {n: _in(getattr(c, n), gpu) for n in ("x", "gamma", "beta", "dy", "dyb")}
    y, mean, rstd = _ln_forward(c, dv, gpu)
    for n, got in (("y", y), ("mean", mean), ("rstd", rstd)):
        R.check(c.name, n, got, getattr(r, n), bf[n], key)
    again, wide = _ln_forward(c, dv, gpu), _ln_forward(c, dv, gpu, ldy=c.E + 8)
    for a, b, w in zip((y, mean, rstd), again, wide):
        assert _same(a, b), f"{c.name}: the forward is not bitwise repeatable"
        assert _same(a, w), f"{c.name}: ergm_layernorm_fwd_ld with ldy = E + 8 differs from ergm_layernorm_fwd"
    for var in variants:
        dyb, drop, drop_res, has_b = R.LN_BWD[var]
        dy64 = (c.dyb if dyb else c.dy).double()
        for tag, (m_in, r_in) in (("fed the reference", (r.mean.float(), r.rstd.float())), ("fed its own", (mean, rstd))):
            rb = R.ln_bwd_ref(c, dy64, m_in.double(), r_in.double(), drop, drop_res)
            bb = R.ln_bwd_bounds(c, dy64, rb, drop, drop_res)
            got = _ln_backward(c, dv, gpu, var, m_in, r_in, "ex")
            for n, gt in zip(("dres", "dres_bf16", "dgamma", "dbeta"), got):
                if gt is not None:
                    R.check(f"{c.name} {var} {tag}", n, gt, getattr(rb, n), bb[n], key)
            if tag == "fed its own":
                other = _ln_backward(c, dv, gpu, var, m_in, r_in, "abi" if var in ("f32", "f32-drop") else "ops")
                for a, b in zip(got, other):
                    assert a is None or _same(a, b), (f"{c.name} {var}: ergm_layernorm_bwd_ex is not bitwise "
                                                      "ergm_layernorm_bwd / not repeatable")


@pytest.mark.parametrize("E", R.LN_E)
def test_layernorm(gpu, E):
    """Every E x rows on benign inputs: forward (y, mean, rstd; ldy = E and E + 8; twice), and the six backward
    variants fed the reference's mean / rstd and the kernel's own.  The f32 variants through ergm_layernorm_bwd_ex are
    bitwise ergm_layernorm_bwd (the two calls share one code path since ergm_layernorm_bwd forwards to it, so this
    holds by construction and checks repeatability); the others run twice, once through the ops.py wrapper."""
    for rows in R.LN_ROWS:
        _ln_run(R.ln_case(E, rows), gpu, ("layernorm", "benign"))


def test_layernorm_long(gpu):
    """2057 rows at E = 64: 258 partial rows, so ln_param_reduce_kernel runs a second round."""
    _ln_run(R.ln_case(*R.LN_LONG), gpu, ("layernorm", "benign"), ("f32", "bf16-drop"))


LN_FAM = [(E, rows, fam, "randn") for E, rows in R.LN_FAMILY_SHAPES for fam in R.LN_FAMILIES if fam != "benign"] + \
         [(E, rows, "benign", "single") for E, rows in R.LN_FAMILY_SHAPES]


@pytest.mark.parametrize("E,rows,family,dyfam", LN_FAM, ids=[f"{f}-{d}-E{E}" for E, _, f, d in LN_FAM])
def test_layernorm_families(gpu, E, rows, family, dyfam):
    """Large mean with small spread, variance far below eps, constant rows, a single outlier, and a dy with a single
    non-zero row."""
    _ln_run(R.ln_case(E, rows, family, dyfam), gpu, ("layernorm", family if dyfam == "randn" else "single-dy"))


# ---- cross-entropy --------------------------------------------------------------------------------------------------
def _xe_dense(c, lg, labels, nv, gpu):
    rl, dl = Guard(1, c.T, f32, gpu), Guard(c.T, c.ldl, bf16, gpu)
    L.call("ergm_xent_fwd_bwd", P(lg), c.ldl, P(labels), P(nv), rl.ptr, dl.ptr, c.B, c.S, c.V, 1.0, ST(gpu))
    assert rl.intact() and dl.intact(), f"{c.name}: wrote outside row_loss / dlogits"
    return rl.cpu()[0], dl.cpu()


XE_CASES = R.xe_matrix()


@pytest.mark.parametrize("V,ldl,bs,family,pad", XE_CASES, ids=[f"{f}-V{V}-ld{ld}-b{bs[0]}s{bs[1]}-{pad}" for V, ld, bs, f, pad in XE_CASES])
def test_xent(gpu, V, ldl, bs, family, pad):
    """Dense and compact: per-row loss and dlogits over all ldl columns per element, the compact list equal to the
    reference's, the compact rows bitwise the dense ones, zero pad rows, untouched rows."""
    c = R.xe_case(V, ldl, bs, family, pad)
    r = R.xe_ref(c)
    b = R.xe_bounds(c, r)
    key = ("xent", family.rstrip("0123456789"))  # the parts of ``edge`` report as one family
    lg, labels, nv = _in(c.logits, gpu), c.labels.to(gpu), _dev_int(c.n_valid, gpu)
    loss, dl = _xe_dense(c, lg, labels, nv, gpu)
    R.check(c.name, "loss", loss, r.loss, b["loss"], key)
    R.check(c.name, "dlogits", dl, r.dlogits, b["dlogits"], key)
    loss2, dl2 = _xe_dense(c, lg, labels, nv, gpu)
    assert _same(loss, loss2) and _same(dl, dl2), f"{c.name}: not bitwise repeatable"
    # compact
    T, T64 = c.T, (c.T + 63) // 64 * 64
    assert int(r.counts[1]) == T64 or not int(r.counts[0])
    rows, pos, counts = (Guard(1, n, i32, gpu, init=-7777) for n in (T, T, 2))
    L.call("ergm_lm_rows", P(labels), c.B, c.S, V, rows.ptr, pos.ptr, counts.ptr, ST(gpu))
    for n, g in (("rows", rows), ("pos", pos), ("counts", counts)):
        assert g.intact() and torch.equal(g.cpu()[0], getattr(r, n)), f"{c.name}: {n} {g.cpu()[0].tolist()}"
    rl, dc = Guard(1, T, f32, gpu), Guard(T64 + 8, ldl, bf16, gpu, init=SENT)  # 8 rows more than the list can fill
    L.call("ergm_xent_compact", P(lg), ldl, P(labels), P(nv), rl.ptr, dc.ptr, pos.ptr, counts.ptr, c.B, c.S, V, ST(gpu))
    assert rl.intact() and dc.intact(), f"{c.name}: the compact form wrote outside row_loss / dlogits_c"
    assert _same(rl.cpu()[0], loss), f"{c.name}: the compact row losses differ from the dense ones"
    dcc, n = dc.cpu(), int(r.counts[0])
    R.check(f"{c.name} compact", "dlogits", dcc[:n], r.dlogits[r.rows[:n].long()], b["dlogits"][r.rows[:n].long()], key)
    assert _same(dcc[:n], dl[r.rows[:n].long()]), f"{c.name}: compact rows differ from the dense rows"
    assert not dcc[n:int(r.counts[1])].float().abs().sum().item(), f"{c.name}: the pad rows are not zero"
    assert bool((dcc[int(r.counts[1]):].float() == SENT).all().item()), f"{c.name}: rows past counts[1] were written"


@pytest.mark.parametrize("V,ldl", [(203, 208), (8193, 8200)])
def test_xent_nothing_scored(gpu, V, ldl):
    """Every label ignored, n_valid = 0: every loss and every gradient is exactly 0."""
    c = R.xe_case(V, ldl, (2, 5), "benign", "nan")
    lg, nv = _in(c.logits, gpu), _dev_int(0, gpu)
    labels = torch.full((c.B, c.S), -100, dtype=i64, device=gpu)
    loss, dl = _xe_dense(c, lg, labels, nv, gpu)
    assert not loss.abs().sum().item() and not dl.float().abs().sum().item()
    assert torch.isfinite(dl.float()).all().item()


# ---- emotion head, loss finalisation --------------------------------------------------------------------------------
def _emo_call(c, dv, gpu, labels=True, grads=True):
    B, Cn, E, S = c.B, c.C, c.E, c.S
    lg, ls = Guard(B, Cn, f32, gpu), Guard(1, 1, f32, gpu, init=5.0 if not labels else NAN)
    dW = Guard(Cn, E, f32, gpu) if grads else None
    dh = Guard(B * S, E, f32, gpu, init=c.dh0) if grads else None
    sc = Guard(1, B * (Cn + 1), f32, gpu)
    L.call("ergm_emotion_head", P(dv["h"]), P(dv["W"]), P(dv["labels"]) if labels else None, lg.ptr, ls.ptr,
           dW.ptr if grads else None, dh.ptr if grads else None, sc.ptr, B, S, E, Cn,
           P(dv["nv"]), P(dv["gs"]), ST(gpu))
    for n, g in (("logits", lg), ("loss_sum", ls), ("dW", dW), ("dh", dh), ("scratch", sc)):
        assert g is None or g.intact(), f"{c.name}: wrote outside {n}"
    return lg.cpu(), ls.cpu()[0], dW.cpu() if grads else None, dh.cpu() if grads else None


EMO = R.emo_matrix()


@pytest.mark.parametrize("B,Cn,E,S,family", EMO, ids=[f"{f}-B{B}-C{Cn}-E{E}-S{S}" for B, Cn, E, S, f in EMO])
def test_emotion_head(gpu, B, Cn, E, S, family):
    """Logits, loss_sum, dW and the dh rows S-1 (added in place) per element; the other dh rows intact; without
    gradients and without labels the logits (and loss_sum) are bitwise the same and nothing else is written."""
    c = R.emo_case(B, Cn, E, S, family)
    r = R.emo_ref(c)
    b = R.emo_bounds(c, r)
    key = ("emotion", family)
    dv = dict(h=_in(c.h, gpu), W=_in(c.W, gpu), labels=c.labels.to(gpu), nv=_dev_int(c.n_valid, gpu),
              gs=torch.tensor([c.gs], dtype=f32, device=gpu))
    lg, ls, dW, dh = _emo_call(c, dv, gpu)
    for n, got in (("logits", lg), ("loss_sum", ls), ("dW", dW), ("dh", dh)):
        R.check(c.name, n, got, getattr(r, n), b[n], key)
    others = torch.ones(B, S, dtype=torch.bool)
    others[:, S - 1] = False
    assert _same(dh.view(B, S, E)[others], c.dh0.view(B, S, E)[others]), f"{c.name}: a dh row other than S-1 changed"
    lg2, ls2, _, _ = _emo_call(c, dv, gpu, grads=False)
    lg3, ls3, _, _ = _emo_call(c, dv, gpu, labels=False, grads=False)
    assert _same(lg, lg2) and _same(ls, ls2) and _same(lg, lg3), f"{c.name}: the forms differ"
    assert ls3.item() == 5.0, f"{c.name}: loss_sum written without labels"


@pytest.mark.parametrize("T", R.FIN_T)
@pytest.mark.parametrize("emo", [True, False], ids=["emo", "lm"])
def test_loss_finalize(gpu, T, emo):
    c = R.fin_case(T, emo)
    ref = R.fin_ref(c)
    out = Guard(1, 3, f32, gpu)
    rl, nv, ne = _in(c.row_loss, gpu), _dev_int(c.n_valid, gpu), _dev_int(c.n_emo, gpu)
    es = c.emo_sum.to(gpu) if emo else None
    L.call("ergm_loss_finalize", P(rl), T, P(nv), P(es), P(ne) if emo else None, out.ptr, ST(gpu))
    assert out.intact()
    R.check(c.name, "out", out.cpu()[0], ref, R.fin_bounds(c, ref), ("finalize", "emo" if emo else "lm"))


def test_loss_finalize_nothing_scored(gpu):
    """n_valid = 0: 0/0 = NaN for the LM mean and the total, as documented; the emotion mean is unaffected."""
    c = R.fin_case(257, True)
    out = Guard(1, 3, f32, gpu)
    rl, nv, ne, es = _in(torch.zeros(257), gpu), _dev_int(0, gpu), _dev_int(c.n_emo, gpu), c.emo_sum.to(gpu)
    L.call("ergm_loss_finalize", P(rl), 257, P(nv), P(es), P(ne), out.ptr, ST(gpu))
    assert out.intact()
    o = out.cpu()[0]
    assert torch.isnan(o[0]).item() and torch.isnan(o[2]).item()
    assert abs(o[1].item() - R.fin_ref(c)[1].item()) <= R.fin_bounds(c, R.fin_ref(c))[1].item()


# ---- column sums ----------------------------------------------------------------------------------------------------
CS = R.cs_matrix()


@pytest.mark.parametrize("rows,cols,dtype", CS, ids=[f"{dt}-r{rows}-c{cols}" for rows, cols, dt in CS])
def test_colsum(gpu, rows, cols, dtype):
    """ldx = cols and a column slice (at column 4) of a NaN matrix cols + 8 wide; plain and accumulating; twice."""
    c = R.cs_case(rows, cols, dtype)
    wsb = L.load().ergm_colsum_workspace_size(rows, cols)
    for ldx in (cols, cols + 8):
        Xd = _in(c.X, gpu, ld=ldx, off=8 + (4 if ldx > cols else 0))
        for acc in (False, True):
            ref, b = R.cs_ref(c, acc), R.cs_bounds(c, acc)
            seen = []
            for _ in range(2):
                out = Guard(1, cols, f32, gpu, init=c.out0 if acc else NAN)
                ws = Guard(1, max(wsb // 4, 4), f32, gpu)
                L.call("ergm_colsum", P(Xd), L.BF16 if dtype == "bf16" else L.F32, rows, cols, ldx, out.ptr, int(acc), ws.ptr,
                       wsb, ST(gpu))
                assert out.intact() and ws.intact(), f"{c.name}: wrote outside out / the workspace"
                seen.append(out.cpu()[0])
            R.check(f"{c.name} ldx {ldx} accumulate {acc}", "colsum", seen[0], ref, b, ("colsum", dtype))
            assert _same(seen[0], seen[1]), f"{c.name}: not bitwise repeatable"


# ---- refused arguments (host path: nothing is launched) -------------------------------------------------------------
def test_refused_arguments(gpu):
    """E % 4 != 0, E > 1024, ldl % 8 != 0, ldl < V, ldl > 65536, C > 16, cols % 4 != 0, and drop_res with a dres_bf16:
    ERGM_EINVAL before any launch.  Every buffer is large enough for the shape named."""
    lib = L.load()
    big = torch.zeros(1 << 18, dtype=f32, device=gpu)  # 1 MiB: any argument below fits
    lab = torch.zeros(64, dtype=i64, device=gpu)
    one = _dev_int(1, gpu)
    p, s = P(big), ST(gpu)
    for E in (6, 1028):
        assert lib.ergm_layernorm_fwd(p, p, p, p, p, p, 1, E, 1e-5, s) == L.ERGM_EINVAL
        assert lib.ergm_layernorm_fwd_ld(p, p, p, p, E + 8, p, p, 1, E, 1e-5, s) == L.ERGM_EINVAL
        assert lib.ergm_layernorm_bwd(p, p, p, p, p, p, p, p, p, p, 1 << 20, 1, E, None, s) == L.ERGM_EINVAL
        assert lib.ergm_layernorm_bwd_ex(p, L.F32, p, p, p, p, p, p, p, p, p, 1 << 20, 1, E, None, 0, s) == L.ERGM_EINVAL
    d = ops.dropout_desc(**R.LN_DROP)
    assert lib.ergm_layernorm_bwd_ex(p, L.BF16, p, p, p, p, p, p, p, p, p, 1 << 20, 1, 64, C.byref(d), 1, s) == L.ERGM_EINVAL
    assert lib.ergm_layernorm_fwd_ld(p, p, p, p, 60, p, p, 1, 64, 1e-5, s) == L.ERGM_EINVAL  # ldy < E
    for V, ldl in ((16, 20), (16, 8), (65540, 65544)):
        assert lib.ergm_xent_fwd_bwd(p, ldl, P(lab), P(one), p, p, 1, 2, V, 1.0, s) == L.ERGM_EINVAL
        assert lib.ergm_xent_compact(p, ldl, P(lab), P(one), p, p, P(one), P(one), 1, 2, V, s) == L.ERGM_EINVAL
    assert lib.ergm_emotion_head(p, p, P(lab), p, p, p, p, p, 2, 1, 64, 17, P(one), None, s) == L.ERGM_EINVAL
    assert lib.ergm_colsum(p, L.F32, 4, 6, 8, p, 0, p, 1 << 20, s) == L.ERGM_EINVAL
    torch.cuda.synchronize(gpu)


def test_worst_ratios(gpu):
    """Prints the worst err/bound per operation, family and output that this session's tests saw."""
    R.report()
