"""The bounds of tests/_rows.py, checked without a GPU from both sides: (a) a plain float32 restatement of each kernel's
rounding points and summation order fits its bound (err/bound <= 1) on every case tests/test_gpu_rows_matrix.py runs,
and (b) the fp64 result of a slightly WRONG operation, measured against the right operation's bound, breaches it on
the output named.  A bound loose enough to admit (b) or tight enough to reject (a) is wrong; neither side is tuned to
the other.  (c) The fp64 references are autograd's gradients of the fp64 forward."""
import math

import pytest
import torch

import _rows as R

f32, f64 = torch.float32, torch.float64


def _show(tag, res):
    print(f"{tag}: " + "  ".join(f"{k} {v:.3g}" for k, v in res.items()))


def _merge(worst, res):
    for k, v in res.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ---- (a) the float32 restatements fit ------------------------------------------------------------------------------
def _ln_fwd(c):
    x, g, b = c.x.double(), c.gamma.double(), c.beta.double()
    r = R.ln_fwd_ref(x, g, b, c.eps)
    return r, R.ln_fwd_bounds(x, g, b, r)


def _ln_admit(c):
    r, bf = _ln_fwd(c)
    y, mean, rstd = R.ln_fwd_emu(c.x, c.gamma, c.beta, c.eps)
    res = {"y": R.ratio(y, r.y, bf["y"]), "mean": R.ratio(mean, r.mean, bf["mean"]),
           "rstd": R.ratio(rstd, r.rstd, bf["rstd"])}
    R.norm_gate(c.name, "y", y, r.y)
    for var, (dyb, drop, drop_res, has_b) in R.LN_BWD.items():
        dy = (c.dyb if dyb else c.dy).float()
        for tag, (m_in, r_in) in (("ref", (r.mean.float(), r.rstd.float())), ("own", (mean, rstd))):
            rb = R.ln_bwd_ref(c, dy.double(), m_in.double(), r_in.double(), drop, drop_res)
            bb = R.ln_bwd_bounds(c, dy.double(), rb, drop, drop_res)
            got = dict(zip(("dres", "dres_bf16", "dgamma", "dbeta"), R.ln_bwd_emu(c, dy, m_in, r_in, drop, drop_res)))
            for n in got:
                if n == "dres_bf16" and not has_b:
                    continue
                res[f"{n}/{var}/{tag}"] = R.ratio(got[n], getattr(rb, n), bb[n])
                R.norm_gate(f"{c.name} {var} fed {tag}", n, got[n], getattr(rb, n))
    return res


def test_layernorm_bound_admits_float32_emulation():
    """Forward (y, mean, rstd) and every backward variant (f32 / bf16 dy, dropout through dres_bf16 and through dres
    itself), fed the reference's mean / rstd and the emulation's own, on every case of the GPU matrix."""
    worst = {}
    for args in R.ln_matrix():
        c = R.ln_case(*args)
        res = _ln_admit(c)
        assert max(res.values()) <= 1.0, (c.name, {k: v for k, v in res.items() if v > 1.0})
        short = {}
        for k, v in res.items():
            short[k.split("/")[0]] = max(short.get(k.split("/")[0], 0.0), v)
        _merge(worst, short)
    _show("layernorm: worst emulation err/bound", worst)


def _xe_admit(c, n_valid=None):
    r = R.xe_ref(c, n_valid)
    b = R.xe_bounds(c, r)
    loss, dl = R.xe_emu(c, n_valid)
    R.norm_gate(c.name, "dlogits", dl, r.dlogits)
    R.norm_gate(c.name, "loss", loss, r.loss)
    return {"loss": R.ratio(loss, r.loss, b["loss"]), "dlogits": R.ratio(dl, r.dlogits, b["dlogits"])}


def test_xent_bound_admits_float32_emulation():
    worst = {}
    for args in R.xe_matrix():
        c = R.xe_case(*args)
        res = _xe_admit(c)
        _show(c.name, res)
        assert max(res.values()) <= 1.0, (c.name, res)
        _merge(worst, res)
    _show("cross-entropy: worst emulation err/bound", worst)


def test_emotion_bound_admits_float32_emulation():
    worst = {}
    for args in R.emo_matrix():
        c = R.emo_case(*args)
        r = R.emo_ref(c)
        b = R.emo_bounds(c, r)
        got = dict(zip(("logits", "loss_sum", "dW", "dh"), R.emo_emu(c)))
        res = {n: R.ratio(got[n], getattr(r, n), b[n]) for n in got}
        assert max(res.values()) <= 1.0, (c.name, res)
        for n in got:
            R.norm_gate(c.name, n, got[n], getattr(r, n))
        _merge(worst, res)
    for T in R.FIN_T:
        for emo in (True, False):
            c = R.fin_case(T, emo)
            ref = R.fin_ref(c)
            res = {"out": R.ratio(R.fin_emu(c), ref, R.fin_bounds(c, ref))}
            assert res["out"] <= 1.0, (c.name, res)
            _merge(worst, res)
    _show("emotion head, finalize: worst emulation err/bound", worst)


def test_colsum_bound_admits_float32_emulation():
    worst = 0.0
    for args in R.cs_matrix():
        c = R.cs_case(*args)
        for acc in (False, True):
            x = R.ratio(R.cs_emu(c, acc), R.cs_ref(c, acc), R.cs_bounds(c, acc))
            assert x <= 1.0, (c.name, acc, x)
            R.norm_gate(c.name, "colsum", R.cs_emu(c, acc), R.cs_ref(c, acc))
            worst = max(worst, x)
    print(f"colsum: worst emulation err/bound {worst:.3g}")


# ---- (b) wrong operations breach -----------------------------------------------------------------------------------
LN_FWD_WRONG = [  # wrong operation, (E, rows, family), outputs that must breach
    ("var_e1", (4, 9, "benign"), ("rstd",)), ("var_e1", (1024, 9, "benign"), ("rstd",)),
    ("var_e1", (768, 9, "bigmean"), ("rstd",)),
    ("lost_group", (260, 9, "benign"), ("mean", "rstd")), ("lost_group", (260, 9, "outlier"), ("mean", "rstd")),
    ("no_eps", (260, 9, "tinyvar"), ("rstd", "y")), ("no_eps", (768, 9, "tinyvar"), ("rstd", "y")),
    ("gamma_shift", (260, 9, "benign"), ("y",)), ("gamma_shift", (768, 9, "bigmean"), ("y",)),
    ("beta_last", (260, 9, "benign"), ("y",)), ("beta_last", (768, 9, "const"), ("y",)),
]


@pytest.mark.parametrize("wrong,shape,outs", LN_FWD_WRONG, ids=[f"{w}-{s[2]}-E{s[0]}" for w, s, _ in LN_FWD_WRONG])
def test_layernorm_forward_bound_rejects(wrong, shape, outs):
    """Variance over E-1; the last float4 group left out of the statistics at E = 260; eps omitted (visible where eps
    dominates: ``tinyvar``; on benign data eps is 1e-6 of the variance and its loss cannot show); gamma shifted by one
    column; beta of column E-1 dropped."""
    c = R.ln_case(*shape)
    r, bf = _ln_fwd(c)
    w = R.ln_fwd_ref(c.x.double(), c.gamma.double(), c.beta.double(), c.eps, wrong)
    res = {n: R.ratio(getattr(w, n), getattr(r, n), bf[n]) for n in outs}
    _show(f"{c.name}, {wrong}: breach", res)
    assert min(res.values()) > 1.0, res


LN_BWD_WRONG = [  # wrong operation, (E, rows), variant, outputs
    ("no_c1", (260, 9), "f32", ("dres",)), ("no_c1", (768, 9), "bf16", ("dres",)),
    ("pad_mean", (260, 9), "f32", ("dres",)), ("pad_mean", (772, 9), "bf16", ("dres",)),
    ("lost_row", (260, 9), "f32", ("dgamma", "dbeta")), ("lost_row", (768, 33), "bf16", ("dgamma", "dbeta")),
    ("lost_part", R.LN_LONG, "bf16", ("dgamma", "dbeta")),
    ("keep_flip", (260, 9), "bf16-drop", ("dres_bf16",)), ("keep_flip", (768, 9), "bf16-dropres", ("dres",)),
    ("no_drop_b", (260, 9), "bf16-drop", ("dres_bf16",)), ("no_drop_b", (768, 9), "f32-drop", ("dres_bf16",)),
]


@pytest.mark.parametrize("wrong,shape,var,outs", LN_BWD_WRONG, ids=[f"{w}-{v}-E{s[0]}r{s[1]}" for w, s, v, _ in LN_BWD_WRONG])
def test_layernorm_backward_bound_rejects(wrong, shape, var, outs):
    """The x^ * mean(g x^) term dropped; mean(g) over the padded width 256*NV (visible only where E is no multiple of
    256); row rows-1 missing from dgamma / dbeta; partial row 256 lost in the reduce at 258 partial rows; one keep bit
    flipped; dres_bf16 not taken through the dropout.  Benign inputs, fed the reference's fp32 mean / rstd."""
    c = R.ln_case(*shape)
    dyb, drop, drop_res, _ = R.LN_BWD[var]
    dy = (c.dyb if dyb else c.dy).double()
    r, _ = _ln_fwd(c)
    m_in, r_in = r.mean.float().double(), r.rstd.float().double()
    rb = R.ln_bwd_ref(c, dy, m_in, r_in, drop, drop_res)
    bb = R.ln_bwd_bounds(c, dy, rb, drop, drop_res)
    w = R.ln_bwd_ref(c, dy, m_in, r_in, drop, drop_res, wrong)
    res = {n: R.ratio(getattr(w, n), getattr(rb, n), bb[n]) for n in outs}
    _show(f"{c.name} {var}, {wrong}: breach", res)
    assert min(res.values()) > 1.0, res


XE_WRONG = [  # wrong operation, case, outputs
    ("lost_last", R.xe_edge_case(8193, 8200, 0), ("loss", "dlogits")),
    ("lost_last", R.xe_edge_case(53250, 53256, 0), ("loss", "dlogits")),
    ("col_v", (8193, 8200, (2, 5), "benign", "big"), ("loss", "dlogits")),
    ("col_v", (53250, 53256, (6, 2), "benign", "nan"), ("loss", "dlogits")),
    ("no_shift", (8193, 8200, (2, 5), "benign", "big"), ("loss", "dlogits")),
    ("n_plus_1", (8193, 8200, (2, 5), "benign", "big"), ("dlogits",)),
    ("n_plus_1", (53250, 53256, (6, 2), "peaked", "big"), ("dlogits",)),
    ("label_v", (8193, 8200, (2, 5), "benign", "big"), ("loss", "dlogits")),
    ("label_v", (53250, 53256, (6, 2), "benign", "nan"), ("loss", "dlogits")),
    ("hot_next", (8193, 8200, (2, 5), "benign", "big"), ("dlogits",)),
    ("hot_next", (53250, 53256, (6, 2), "wide", "big"), ("dlogits",)),
]


@pytest.mark.parametrize("wrong,case,outs", XE_WRONG, ids=[f"{w}-{c[3]}-V{c[0]}-{c[4]}" for w, c, _ in XE_WRONG])
def test_xent_bound_rejects(wrong, case, outs):
    """Column V-1 left out of the sum of exponentials (visible on ``edge``, where the row maximum sits on it; on benign
    data the column carries 1/V of the sum and its loss is 1e4 times less visible); column V included; labels not
    shifted; 1/(n + 1); a label equal to V scored; the one-hot placed at target + 1."""
    c = R.xe_case(*case)
    r = R.xe_ref(c)
    b = R.xe_bounds(c, r)
    w = R.xe_ref(c, wrong=wrong)
    res = {"loss": R.ratio(w.loss, r.loss, b["loss"]), "dlogits": R.ratio(w.dlogits, r.dlogits, b["dlogits"])}
    res = {n: res[n] for n in outs}
    _show(f"{c.name}, {wrong}: breach", res)
    assert min(res.values()) > 1.0, res


@pytest.mark.parametrize("V,ldl", R.XE_SHAPES)
def test_xent_bound_rejects_every_lost_edge_column(V, ldl):
    """Every column of xe_edges(V) -- V-1, 0 and the last and first column of every 4096-column stripe -- left out of
    the sum of exponentials breaches the loss and dlogits bounds on the ``edge`` part that puts a scored row's maximum
    on it, at every shape of the matrix: 2 columns at V = 203 and 4096, 5 at 8193, ... 28 at 53250, 32 at 65536."""
    least = {"loss": math.inf, "dlogits": math.inf}
    reached = set()
    for part in range(R.xe_edge_parts(V)):
        c = R.xe_case(*R.xe_edge_case(V, ldl, part))
        reached |= {cmax for cmax, _ in R.xe_edge_plan(V, part)}
        r = R.xe_ref(c)
        b = R.xe_bounds(c, r)
        for col in sorted({cmax for cmax, _ in R.xe_edge_plan(V, part)}):
            w = R.xe_ref(c, lost_col=col)
            res = {"loss": R.ratio(w.loss, r.loss, b["loss"]), "dlogits": R.ratio(w.dlogits, r.dlogits, b["dlogits"])}
            assert min(res.values()) > 1.0, (c.name, col, res)
            least = {n: min(least[n], res[n]) for n in res}
    assert reached == set(R.xe_edges(V))
    _show(f"V = {V}: smallest breach over {len(reached)} lost edge columns", least)


def test_xent_lost_column_needs_the_edge_family():
    """Why ``edge`` exists: on benign logits column V-1 carries about 1/V of the sum and its loss moves the per-row
    loss by anything from less than one bound to some ten, depending on the draw; with the row maximum on that column
    it moves it by four orders of magnitude more.  An edge bug that a benign case may or may not show, ``edge`` shows
    beyond doubt."""
    seen = {}
    for fam in ("benign", "edge"):
        c = R.xe_case(8193, 8200, (2, 5), fam, "big")
        r = R.xe_ref(c)
        seen[fam] = R.ratio(R.xe_ref(c, wrong="lost_last").loss, r.loss, R.xe_bounds(c, r)["loss"])
    _show("column V-1 lost, per-row loss err/bound", seen)
    assert seen["benign"] < 100.0 and seen["edge"] > 1e3 * seen["benign"]


@pytest.mark.parametrize("wrong,case,outs", [("lost_sample", (17, 7, 768, 8, "benign"), ("dW",)),
                                             ("mean_b", (17, 7, 768, 8, "benign"), ("dW", "dh")),
                                             ("mean_b", (33, 16, 1024, 8, "benign"), ("dW", "dh"))])
def test_emotion_bound_rejects(wrong, case, outs):
    """Sample B-1 left out of dW at B = 17; the mean taken over B instead of the valid count."""
    c = R.emo_case(*case)
    r = R.emo_ref(c)
    b = R.emo_bounds(c, r)
    w = R.emo_ref(c, wrong)
    res = {n: R.ratio(getattr(w, n), getattr(r, n), b[n]) for n in outs}
    _show(f"{c.name}, {wrong}: breach", res)
    assert min(res.values()) > 1.0, res


@pytest.mark.parametrize("wrong,rows,cols", [("lost_row", 65, 260), ("lost_row", 65, 4), ("lost_cols", 65, 260),
                                             ("lost_cols", 1, 260)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_colsum_bound_rejects(wrong, rows, cols, dtype):
    """Row rows-1 lost at rows = 65 (the second partial block's only row); columns 256..259 lost at cols = 260."""
    c = R.cs_case(rows, cols, dtype)
    for acc in (False, True):
        x = R.ratio(R.cs_ref(c, acc, wrong), R.cs_ref(c, acc), R.cs_bounds(c, acc))
        print(f"{c.name} accumulate {acc}, {wrong}: breach {x:.3g}x")
        assert x > 1.0


# ---- (c) the references are the operations ---------------------------------------------------------------------------
@pytest.mark.parametrize("var", ["f32", "bf16-drop", "bf16-dropres"])
def test_layernorm_reference_matches_autograd(var):
    """With x = a + Z*b (Z = keep/(1-p)) and L = sum(dy * LN(x)) + sum(dres0 * x): dL/da is dres, dL/db is what dres_bf16
    holds, and with drop_res (x = Z*e) dL/de is dres; dL/dgamma, dL/dbeta are dgamma, dbeta."""
    c = R.ln_case(260, 9)
    dyb, drop, drop_res, _ = R.LN_BWD[var]
    dy = (c.dyb if dyb else c.dy).double()
    Z = c.keep.double() * R.ln_scale() if drop else torch.ones(c.rows, c.E, dtype=f64)
    a = (0.0 if drop_res else 1.0) * c.x.double()
    a.requires_grad_(True)
    b = c.dy.double().flip(0).requires_grad_(True)
    gamma, beta = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    x = a + Z * b
    r = R.ln_fwd_ref(x, gamma, beta, c.eps)
    (r.y * dy).sum().add((c.dres0.double() * x).sum()).backward()
    rb = R.ln_bwd_ref(R.NS(**{**vars(c), "x": x.detach()}), dy, r.mean.detach(), r.rstd.detach(), drop, drop_res)
    want = {"dres": b.grad if drop_res else a.grad, "dres_bf16": b.grad, "dgamma": gamma.grad, "dbeta": beta.grad}
    for n, w in want.items():
        got = getattr(rb, n)
        assert (got - w).abs().max().item() < 1e-12 * max(1.0, w.abs().max().item()), n


def test_xent_reference_matches_autograd():
    """Per-row loss and gradient of torch's cross_entropy (ignore_index -100, mean over the scored rows) on the shifted
    logits; labels >= V are ignored by the kernel and are mapped to -100 for torch."""
    c = R.xe_case(203, 208, (2, 5), "benign", "nan")
    r = R.xe_ref(c)
    x = c.logits[:, :c.V].double().requires_grad_(True)
    tgt, valid = R.xe_targets(c.labels, c.V)
    t = torch.where(valid, tgt, torch.full_like(tgt, -100))
    torch.nn.functional.cross_entropy(x, t, ignore_index=-100).backward()
    rows = torch.nn.functional.cross_entropy(x.detach(), t, ignore_index=-100, reduction="none")
    assert int(valid.sum()) == c.n_valid == 5
    assert (r.loss - rows).abs().max().item() < 1e-12
    assert (r.dlogits[:, :c.V] - x.grad).abs().max().item() < 1e-12
    assert not r.dlogits[:, c.V:].any().item()


def test_emotion_reference_matches_autograd():
    c = R.emo_case(17, 7, 100, 8)
    r = R.emo_ref(c)
    hl = r.hl.clone().requires_grad_(True)
    W = c.W.double().requires_grad_(True)
    t = torch.where(r.valid, c.labels, torch.full_like(c.labels, -100))
    (torch.nn.functional.cross_entropy(hl @ W.T, t, ignore_index=-100) * c.gs).backward()
    dh = r.dh.view(c.B, c.S, c.E)[:, c.S - 1] - c.dh0.double().view(c.B, c.S, c.E)[:, c.S - 1]
    assert (r.dW - W.grad).abs().max().item() < 1e-12 and (dh - hl.grad).abs().max().item() < 1e-12


def test_ratio_counts_nan_and_inf_as_a_breach():
    one = torch.ones(1, dtype=f64)
    assert R.ratio(torch.tensor([math.nan]), 0.0 * one, one) == math.inf
    assert R.ratio(torch.tensor([math.inf]), 0.0 * one, one) == math.inf
