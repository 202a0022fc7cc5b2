"""The row kernels of norm.hip and xent.hip on the CPU: LayerNorm forward / backward, the shifted cross-entropy (dense
and compact), the emotion head with ergm_loss_finalize, and ergm_colsum.  For each operation: the cases of
tests/test_gpu_rows_matrix.py, an fp64 reference on exactly the inputs the kernel gets (bf16 inputs are exact), an
elementwise error bound, and a plain float32 restatement of the kernel's rounding points and summation order.  Imports
no GPU code; tests/test_rows_bound.py checks the bounds here, from both sides, without a GPU.

How the bounds are made.  u32 = 2^-24 and u16 = 2^-8 are the unit roundoffs of fp32 and bf16.  Every sum in these
kernels has a fixed tree, so a sum is charged the number of roundings on ONE path from a summand to the result (times
the sum of magnitudes), not the number of summands.  The build has no fast-math: fp32 division and sqrtf are correctly
rounded (1 u32), logf and expf are within 1 ulp (2 u32).  `__expf(a)` is exp2(a * log2e) with the product rounded in
fp32: the product's rounding moves the result by u32*|a| relative, the rounded constant log2e (off by 0.23 u32) by
another 0.23*u32*|a|, and where ``a`` is itself a rounded fp32 difference that is one more u32*|a|; v_exp_f32 is
within 1 ulp and the 8 of the attention bound (tests/_attn.py) is kept for it: rel(__expf(a)) <= u32*(3|a| + 8).  It
flushes subnormal results, and bf16 / fp32 subnormals are the only place where rounding is not relative: an absolute
floor of 2^-100 everywhere, far below anything a wrong element produces (65536 flushed exponentials are 2^-110).
hipcc may contract a*b + c into an FMA; that removes a rounding and never adds one, so the bounds count the
uncontracted form and the float32 restatements are uncontracted.  Nothing here is fitted to any output, GPU or
emulated; no element is excluded from any comparison; a NaN or inf where the reference is finite is an infinite
breach.
"""
import functools
import math
import types
import zlib

import torch

from oracle import philox as X

U16, U32 = 2.0 ** -8, 2.0 ** -24
FLOOR = 2.0 ** -100
LOG2E32 = torch.tensor(1.4426950408889634, dtype=torch.float32)
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
NS = types.SimpleNamespace
WORST = {}  # (operation, family) -> output -> largest err/bound seen
# the older tests' whole-tensor relative Frobenius gates (tests/test_gpu_ops.py), kept as a second opinion
GATE = {"y": 6e-3, "dres": 1e-5, "dres_bf16": 6e-3, "dgamma": 1e-5, "dbeta": 1e-5, "loss": 1e-4, "dlogits": 6e-3,
        "logits": 1e-5, "loss_sum": 1e-5, "dW": 1e-5, "dh": 1e-5, "colsum": 1e-6}


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ratio(got, ref, b):
    """Largest err/bound; a NaN or inf anywhere in ``got`` where ``ref`` is finite counts as infinite."""
    got = got.double()
    if (~torch.isfinite(got) & torch.isfinite(ref)).any().item():
        return math.inf
    if not got.numel():
        return 0.0
    e = (got - ref).abs() / b
    return torch.where(torch.isfinite(ref), e, torch.zeros_like(e)).max().item()


def norm_gate(what, out, got, ref):
    tol = GATE.get(out)
    if tol is None:
        return
    err = (got.double() - ref).norm().item()
    rel = 0.0 if err == 0.0 else err / max(ref.norm().item(), 1e-300)
    assert rel < tol, f"{what} {out}: relative norm error {rel:.3g} past the gate {tol:g}"


def check(what, out, got, ref, b, key=None, gate=True):
    """``got`` against the fp64 ``ref`` of output ``out``: no NaN / inf, every element within the bound ``b`` (the first
    offender reported), then the older whole-tensor norm gate.  Returns, and records under ``key`` = (operation,
    family), the worst err/bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, out, got.shape, ref.shape)
    b = torch.as_tensor(b, dtype=f64).expand_as(ref)
    assert torch.isfinite(got).all().item(), f"{what} {out}: NaN or inf in the result"
    err = (got - ref).abs()
    worst = (err / b).max().item() if err.numel() else 0.0
    if key is not None:
        w = WORST.setdefault(key, {})
        w[out] = max(w.get(out, 0.0), worst)
    bad = err > b
    if bad.any().item():
        i = tuple(int(x) for x in torch.nonzero(bad)[0])
        raise AssertionError(f"{what} {out}: {int(bad.sum())} of {bad.numel()} elements past the bound, worst err/bound "
                             f"{worst:.3g}, first at {i}: got {got[i].item()!r} want {ref[i].item()!r} bound "
                             f"{b[i].item():.3g}")
    if gate:
        norm_gate(what, out, got, ref)
    return worst


def report():
    for key in sorted(WORST):
        print(f"{key[0]:<10} {key[1]:<14} worst err/bound " + "  ".join(f"{k} {v:.4f}" for k, v in WORST[key].items()))


def _tree(v, dim=-1):
    """Sum by pairing neighbours until one value is left (the dimension is a power of two): the order of wave_sum's
    xor butterfly (DPP quad_perm 1, 2, the two row mirrors, the 16- and 32-lane swaps; addition commutes, so every
    lane ends with this tree's value) and of the reduce kernels' `v[j] += v[j + w]` loops."""
    v = v.movedim(dim, -1)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _seq(v, dim):
    """Sequential sum from 0 along ``dim``, in index order."""
    v = v.movedim(dim, 0)
    acc = torch.zeros_like(v[0])
    for i in range(v.shape[0]):
        acc = acc + v[i]
    return acc


def _exp32(a):
    """__expf in float32: exp2(a * log2e), the product rounded."""
    return torch.exp2(a * LOG2E32)


# =====================================================================================================================
# LayerNorm
# =====================================================================================================================
LN_EPS = 1e-5
LN_E = (4, 64, 252, 256, 260, 512, 516, 768, 772, 1024)  # NV 1 1 1 1 2 2 3 3 4 4; 252, 260, 516, 772: ragged group
LN_ROWS = (1, 3, 4, 5, 8, 9, 33)  # around the forward's 4 rows and the backward's 8 rows per workgroup
LN_LONG = (64, 2057)  # 258 partial rows: ln_param_reduce_kernel runs a second round
LN_FAMILIES = ("benign", "bigmean", "tinyvar", "const", "outlier")
LN_FAMILY_SHAPES = ((260, 9), (768, 9))
LN_DROP = dict(p=0.1, seed=0x5EED1234ABCD, offset=3, site=4, row0=1000)
# backward variants: name -> (bf16 dy, dropout, drop_res, dres_bf16 written)
LN_BWD = {"f32": (False, False, False, True), "bf16": (True, False, False, True), "f32-drop": (False, True, False, True),
          "bf16-drop": (True, True, False, True), "bf16-dropres": (True, True, True, False),
          "f32-nob": (False, False, False, False)}


def ln_nv(E):
    return (E + 255) // 256


@functools.lru_cache(maxsize=None)
def ln_case(E, rows, family="benign", dyfam="randn"):
    """x, dy, dres0 f32 [rows, E] (dyb: dy rounded to bf16), gamma / beta f32 [E].  gamma has exact zeros and one
    negative entry; every row differs."""
    name = f"ln-{family}-{dyfam}-E{E}-r{rows}"
    g = _gen(name)
    z = torch.randn(rows, E, generator=g)
    r = torch.arange(rows, dtype=f32)[:, None]
    if family == "benign":
        x = 3.0 * z + 1.0
    elif family == "bigmean":
        x = z + 1000.0
    elif family == "tinyvar":
        x = 1e-4 * z + 0.5
    elif family == "const":
        x = (0.3 * (r + 1.0) - 1.0).expand(rows, E).contiguous()
    elif family == "outlier":
        x = z.clone()
        x[torch.arange(rows), (torch.arange(rows) * 7 + 3) % E] = 1e4
    else:
        raise ValueError(family)
    gamma = 0.5 * torch.randn(E, generator=g) + 1.0
    beta = torch.randn(E, generator=g)
    for i in (1, E // 3, E - 2):
        gamma[i] = 0.0
    gamma[E // 2] = -0.75
    dy = torch.randn(rows, E, generator=g)
    if dyfam == "single":
        keep = torch.zeros(rows, 1)
        keep[rows // 2] = 1.0
        dy = dy * keep
    elif dyfam != "randn":
        raise ValueError(dyfam)
    dres0 = torch.randn(rows, E, generator=g)
    p32 = float(torch.tensor(LN_DROP["p"], dtype=f32))  # the threshold is formed from the descriptor's fp32 p
    keepm = torch.from_numpy(X.keep_mask(LN_DROP["seed"], LN_DROP["offset"], LN_DROP["site"], p32, rows, E,
                                         LN_DROP["row0"]))
    return NS(name=name, E=E, rows=rows, family=family, x=x.float(), gamma=gamma, beta=beta, dy=dy, dyb=dy.bfloat16(),
              dres0=dres0, keep=keepm, eps=LN_EPS)


def ln_scale():
    """1/(1-p) of the dropout, p as the fp32 the descriptor holds."""
    return 1.0 / (1.0 - float(torch.tensor(LN_DROP["p"], dtype=f32)))


def ln_fwd_ref(x, gamma, beta, eps, wrong=None):
    """fp64 LayerNorm (biased variance) of fp64 copies of the kernel's inputs; eps is the fp32 the kernel receives.
    ``wrong`` selects a deliberately WRONG operation (tests/test_rows_bound.py)."""
    E = x.shape[1]
    eps = float(torch.tensor(eps, dtype=f32))
    xs = x[:, :E - 4] if wrong == "lost_group" else x  # the last float4 group left out of the statistics
    mean = xs.mean(1)
    var = ((xs - mean[:, None]) ** 2).sum(1) / (E - 1 if wrong == "var_e1" else xs.shape[1])
    rstd = 1.0 / torch.sqrt(var + (0.0 if wrong == "no_eps" else eps))
    g = torch.roll(gamma, 1) if wrong == "gamma_shift" else gamma
    b = beta.clone()
    if wrong == "beta_last":
        b[E - 1] = 0.0
    xc = x - mean[:, None]
    return NS(mean=mean, var=var, rstd=rstd, xc=xc, y=xc * rstd[:, None] * g + b, eps=eps)


def ln_fwd_bounds(x, gamma, beta, r):
    """Bounds of mean, rstd (fp32) and y (bf16) given the fp64 reference ``r``; NV = ceil(E/256).

    * mean = wave_sum(s) * (1/E): a lane adds NV float4 partials in sequence, each (x0 + x1) + (x2 + x3) (2 adds), the
      butterfly has 6 levels, 1/E is rounded and the product is rounded: NV + 10 roundings on a path.
      bound(mean) = bm = (NV + 10) * u32 * mean|x|.
    * var = wave_sum(q) * (1/E), q summing (x - m^)^2 with the same tree.  Around the kernel's own mean m^ the sum of
      squares is E*var + E*(m^ - mean)^2 exactly, so var moves by at most bm^2; each summand carries the rounding of the
      difference twice and of the square, the tree NV + 10 more: bvar = (NV + 13) * u32 * (var + bm^2) + bm^2.
    * rstd = 1 / sqrtf(var + eps): half the relative error of var + eps (its own rounding included), sqrtf and the
      division correctly rounded: bound(rstd) = rstd * er, er = 0.5 * bvar / (var + eps) + 3 * u32.
    * y = bf16(((x - m^) * r^) * gamma + beta): the difference carries bm absolutely and three roundings relatively
      (difference, times r^, times gamma), r^ carries er, the final add rounds the result:
      d0 = |gamma| * rstd * (|x - mean| * (3 * u32 + er) + bm), d = d0 + u32 * (|y| + d0);
      bound(y) = d + u16 * (|y| + d): a rounding is relative to the value rounded, which already carries an error."""
    E = x.shape[1]
    NV = ln_nv(E)
    bm = (NV + 10) * U32 * x.abs().mean(1)
    bvar = (NV + 13) * U32 * (r.var + bm ** 2) + bm ** 2
    er = 0.5 * bvar / (r.var + r.eps) + 3.0 * U32
    d0 = gamma.abs() * r.rstd[:, None] * (r.xc.abs() * (3.0 * U32 + er[:, None]) + bm[:, None])
    d = d0 + U32 * (r.y.abs() + d0)
    return {"mean": bm.clamp_min(FLOOR), "rstd": (r.rstd * er).clamp_min(FLOOR),
            "y": (d + U16 * (r.y.abs() + d)).clamp_min(FLOOR)}


def _lanes(v, E):
    """[rows, E] -> [rows, NV, 64, 4], zero-padded: lane l of group i holds columns (i*64 + l)*4 .. +3."""
    rows = v.shape[0]
    NV = ln_nv(E)
    p = torch.zeros(rows, NV * 256, dtype=v.dtype)
    p[:, :E] = v
    return p.view(rows, NV, 64, 4)


def _row_sum(v4):
    """ln kernels' row sum of [rows, NV, 64, 4]: float4 pairs, NV in sequence per lane, then the butterfly."""
    part = (v4[..., 0] + v4[..., 1]) + (v4[..., 2] + v4[..., 3])
    return _tree(_seq(part, 1))


def ln_fwd_emu(x, gamma, beta, eps):
    """ln_fwd_kernel in float32.  Returns (y bf16, mean, rstd)."""
    rows, E = x.shape
    inv_e = torch.tensor(1.0, dtype=f32) / torch.tensor(float(E), dtype=f32)
    mean = _row_sum(_lanes(x, E)) * inv_e
    d = x - mean[:, None]
    var = _row_sum(_lanes(d * d, E)) * inv_e
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=f32))
    y = (d * rstd[:, None]) * gamma + beta
    return y.bfloat16(), mean, rstd


def ln_bwd_ref(c, dy, mean, rstd, drop=False, drop_res=False, wrong=None):
    """fp64 backward formula on the kernel's inputs: dy (fp64 copy of the f32 or bf16 dy), the fp32 mean / rstd it is
    fed (fp64 copies), x, gamma, dres0 and the Philox keep bits of case ``c``.
    h = (x - mean)*rstd, g = dy*gamma, dx = rstd*(g - mean(g) - h*mean(g*h)); dres = dres0 + dx, with drop_res taken
    through the dropout; dres_bf16 = dres through the dropout (or dres itself); dgamma = sum_r dy*h, dbeta = sum_r dy."""
    x, gamma, dres0 = c.x.double(), c.gamma.double(), c.dres0.double()
    rows, E = x.shape
    h = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    c1 = (g * h).mean(1)
    c2 = g.sum(1) / (ln_nv(E) * 256 if wrong == "pad_mean" else E)
    if wrong == "no_c1":
        c1 = torch.zeros_like(c1)
    dx = rstd[:, None] * (g - c2[:, None] - h * c1[:, None])
    pre = dres0 + dx
    keep = c.keep.clone()
    if wrong == "keep_flip":
        keep[rows // 2, E // 2 + 1] = ~keep[rows // 2, E // 2 + 1]
    Z = keep.double() * ln_scale() if drop else torch.ones_like(x)
    dres = Z * pre if drop_res else pre
    db = dres if (drop_res or wrong == "no_drop_b") else Z * pre
    w = torch.ones(rows, 1, dtype=f64)
    if wrong == "lost_row":
        w[rows - 1] = 0.0
    if wrong == "lost_part":  # partial row 256 = rows 2048 .. 2055
        w[2048:2056] = 0.0
    return NS(h=h, g=g, c1=c1, c2=c2, pre=pre, Z=Z, dres=dres, dres_bf16=db, dgamma=(w * dy * h).sum(0),
              dbeta=(w * dy).sum(0), rstd=rstd)


def ln_bwd_bounds(c, dy, r, drop=False, drop_res=False):
    """Bounds of dres (fp32), dres_bf16, dgamma, dbeta (fp32) given the fp64 ``r`` of ln_bwd_ref; NV = ceil(E/256).

    * h^ = (x - mean) * rstd carries 2 roundings, g^ = dy * gamma one.  c1 = wave_sum(s1) / E over products g*h (3
      roundings from the factors, 1 from the product) with the forward's tree (NV + 10): bc1 = (NV + 14) * u32 *
      mean|g*h|; c2 likewise without the product: bc2 = (NV + 11) * u32 * mean|g|.
    * dx = rstd * ((g - c2) - h * c1): with A = |g| + |c2| + |h*c1| the roundings of g^, of the two differences, of
      h^*c1 (3) and of the product with rstd sum to at most 5 * u32 * A; bdx = rstd * (5 * u32 * A + bc2 + |h| * bc1).
      The in-place add rounds the result: b(pre) = bdx + u32 * (|dres0 + dx| + bdx).
    * Through a dropout the value is multiplied by keep * fl(1/(1-p)): the bound scales with it and gains 3 * u32 of the
      result (the scale's division and subtraction, the product); dropped elements are exactly 0 on both sides.
    * dres_bf16 = bf16(w): b32(w) + u16 * (|w| + b32(w)).
    * dgamma: a product dy*h^ (3 roundings), 7 sequential adds across the 8 waves of a workgroup, then
      ln_param_reduce_kernel: a 5-level tree over the 32 partial rows a lane holds, one add per round of 256 partial
      rows, a 3-level tree over the 8 row lanes: (18 + rounds) * u32 * sum_r|dy*h|; dbeta has no product:
      (15 + rounds) * u32 * sum_r|dy|."""
    E, rows = c.E, c.rows
    NV = ln_nv(E)
    h, g = r.h, r.g
    bc1 = (NV + 14) * U32 * (g * h).abs().mean(1)
    bc2 = (NV + 11) * U32 * g.abs().mean(1)
    A = g.abs() + r.c2.abs()[:, None] + (h * r.c1[:, None]).abs()
    bdx = r.rstd.abs()[:, None] * (5.0 * U32 * A + bc2[:, None] + h.abs() * bc1[:, None])
    bpre = bdx + U32 * (r.pre.abs() + bdx)
    bdrop = r.Z * bpre + 3.0 * U32 * (r.Z * r.pre).abs()
    bres = bdrop if drop_res else bpre
    b32 = bdrop if (drop and not drop_res) else bres
    bb = b32 + U16 * (r.dres_bf16.abs() + b32)
    rounds = ((rows + 7) // 8 + 255) // 256
    bg = (18 + rounds) * U32 * (dy * h).abs().sum(0)
    bbeta = (15 + rounds) * U32 * dy.abs().sum(0)
    return {"dres": bres.clamp_min(FLOOR), "dres_bf16": bb.clamp_min(FLOOR), "dgamma": bg.clamp_min(FLOOR),
            "dbeta": bbeta.clamp_min(FLOOR)}


def ln_bwd_emu(c, dy, mean, rstd, drop=False, drop_res=False):
    """ln_bwd_kernel and ln_param_reduce_kernel in float32 (dy, mean, rstd float32).  Returns dres f32, dres_bf16,
    dgamma, dbeta."""
    x, gamma = c.x, c.gamma
    rows, E = x.shape
    inv_e = torch.tensor(1.0, dtype=f32) / torch.tensor(float(E), dtype=f32)
    h = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    c1 = _row_sum(_lanes(g * h, E)) * inv_e
    c2 = _row_sum(_lanes(g, E)) * inv_e
    v = c.dres0 + rstd[:, None] * (g - c2[:, None] - h * c1[:, None])
    scale = torch.tensor(1.0, dtype=f32) / (torch.tensor(1.0, dtype=f32) - torch.tensor(LN_DROP["p"], dtype=f32))
    dropped = torch.where(c.keep, v * scale, torch.zeros_like(v))
    if drop and drop_res:
        v = dropped
    u = dropped if (drop and not drop_res) else v
    nparts = (rows + 7) // 8

    def reduce(t):
        p = torch.zeros(nparts * 8, E)
        p[:rows] = t
        part = _seq(p.view(nparts, 8, E), 1)  # the 8 waves in sequence
        rounds = (nparts + 255) // 256
        q = torch.zeros(rounds * 256, E)
        q[:nparts] = part
        lane = _seq(_tree(q.view(rounds, 32, 8, E), 1), 0)  # [8, E]: 32 loads as a tree, rounds in sequence
        return _tree(lane, 0)

    return v, u.bfloat16(), reduce(dy * h), reduce(dy)


# =====================================================================================================================
# Cross-entropy
# =====================================================================================================================
XE_SHAPES = ((203, 208), (4096, 4096), (8193, 8200), (16390, 16392), (32768, 32768), (50260, 50304), (53250, 53256),
             (65536, 65536))  # xent_kernel<2, 2, 4, 8, 8, 13, 16, 16>
XE_FAMILY_SHAPES = ((8193, 8200), (53250, 53256))  # NCH 4 and 16, both with pad columns
XE_FAMILIES = ("benign", "peaked", "offset", "flat", "wide", "edge")  # "edge" runs in parts: edge, edge1, edge2, ...
XE_BS = ((2, 5), (6, 2))
XE_EDGE_BS = (2, 5)  # every row with s < S-1 scored: 8 scored rows per part


def xe_nch(ldl):
    n = ((ldl + 7) // 8 + 511) // 512
    return 2 if n <= 2 else 4 if n <= 4 else 8 if n <= 8 else 13 if n <= 13 else 16


def xe_labels(B, S, V):
    """Targets 0, V-1 and both sides of a 4096-column stripe edge; -100, labels V and V + 7 (>= V: ignored); in the
    (6, 2) layout a sequence whose only label sits at s = 0 (it scores nothing) and a fully ignored one."""
    lo = 4095 if V > 4096 else V // 2
    hi = 4096 if V > 4097 else V // 3
    if (B, S) == (2, 5):
        lab = [[5, 0, V - 1, hi, -100], [-100, V // 2, V, lo, V + 7]]
    elif (B, S) == (6, 2):
        lab = [[9, 0], [-100, V - 1], [3, hi], [7, -100], [-100, -100], [1, V]]
    else:
        raise ValueError((B, S))
    return torch.tensor(lab, dtype=torch.int64)


def xe_edges(V):
    """The columns at which a chunk set or the vocabulary ends or begins: V-1 and 0 first, then the last and first
    column of every 4096-column stripe (8*512*i - 1 and 8*512*i) below V-1."""
    return [V - 1, 0] + [c for i in range(1, 17) for c in (4096 * i - 1, 4096 * i) if c < V - 1]


def xe_edge_parts(V):
    """How many ``edge`` cases of 8 scored rows put the row maximum on every column of xe_edges(V) once."""
    return (len(xe_edges(V)) + 7) // 8


def xe_edge_plan(V, part):
    """(maximum, runner-up) columns of the 8 scored rows of ``edge`` part ``part``: scored row j of part k has its
    maximum on edge 8k + j and the runner-up, which is also its target, on edge 8k + j + 1 (cyclically), so part 0
    begins with the maximum on V-1 and the runner-up on 0."""
    e = xe_edges(V)
    return [(e[(8 * part + j) % len(e)], e[(8 * part + j + 1) % len(e)]) for j in range(8)]


def xe_edge_case(V, ldl, part):
    """The arguments of xe_case for ``edge`` part ``part`` (the pad columns alternate between 1e4 and NaN)."""
    return (V, ldl, XE_EDGE_BS, f"edge{part or ''}", ("big", "nan")[part % 2])


def xe_targets(labels, V, shift=True):
    """Per row t = b*S + s: the target (labels[b][s+1], -100 for s = S-1) and whether the row is scored."""
    B, S = labels.shape
    tgt = torch.full((B, S), -100, dtype=torch.int64)
    if shift:
        tgt[:, :S - 1] = labels[:, 1:]
    else:
        tgt = labels.clone()
    tgt = tgt.reshape(-1)
    return tgt, (tgt >= 0) & (tgt < V)


@functools.lru_cache(maxsize=None)
def xe_case(V, ldl, bs, family="benign", pad="big"):
    """bf16 logits [B*S, ldl], int64 labels [B, S].  Columns [V, ldl) hold +1e4 (``pad`` = "big") or NaN ("nan")."""
    B, S = bs
    T = B * S
    name = f"xe-{family}-V{V}-ld{ldl}-b{B}s{S}-{pad}"
    g = _gen(name)
    edge = family.startswith("edge")
    if edge:  # every row with s < S-1 is scored, against its runner-up column
        part = int(family[4:] or 0)
        assert bs == XE_EDGE_BS and 0 <= part < xe_edge_parts(V), (bs, family)
        plan = xe_edge_plan(V, part)
        labels = torch.full((B, S), 5, dtype=torch.int64)
        labels[:, 1:] = torch.tensor([r for _, r in plan]).view(B, S - 1)
    else:
        labels = xe_labels(B, S, V)
    tgt, valid = xe_targets(labels, V)
    z = torch.randn(T, V, generator=g)
    if family == "benign":
        x = 3.0 * z
    elif family == "peaked":  # +60 on the target (loss ~ 0) / beside it (loss ~ 60), alternating over the scored rows
        x = z.clone()
        j = 0
        for t in range(T):
            col = int(tgt[t]) if valid[t] else t % V
            if valid[t]:
                col = col if j % 2 == 0 else (col + 1) % V
                j += 1
            x[t, col] = 60.0
    elif family == "offset":
        x = 3.0 * z + 200.0
    elif family == "flat":
        x = (0.25 * torch.arange(T, dtype=f32) - 1.0)[:, None].expand(T, V).contiguous()
    elif family == "wide":
        x = 40.0 * z
    elif edge:  # the j-th SCORED row: maximum and runner-up on consecutive columns of xe_edges(V) (xe_edge_plan)
        x = 3.0 * z
        top = x.max(1).values + 8.0
        scored = [t for t in range(T) if valid[t]]
        assert len(scored) == len(plan)
        for t, (cmax, crun) in zip(scored, plan):
            x[t, cmax] = top[t]
            x[t, crun] = top[t] - 1.0
    else:
        raise ValueError(family)
    logits = torch.full((T, ldl), 1e4 if pad == "big" else math.nan, dtype=bf16)
    logits[:, :V] = x.bfloat16()
    return NS(name=name, V=V, ldl=ldl, B=B, S=S, T=T, family=family, pad=pad, logits=logits, labels=labels,
              n_valid=int(valid.sum()), NCH=xe_nch(ldl))


def xe_ref(c, n_valid=None, wrong=None, lost_col=None):
    """fp64 shifted cross-entropy of case ``c``: per-row loss [T], dlogits [T, ldl] (0 on ignored rows and on columns
    >= V), and the compact list (rows, pos, counts).  ``wrong`` / ``lost_col`` (a column left out of the sum of
    exponentials; "lost_last" is column V-1) select a deliberately WRONG operation."""
    V, T = c.V, c.T
    n = c.n_valid if n_valid is None else n_valid
    tgt, valid = xe_targets(c.labels, V + 1 if wrong == "label_v" else V, shift=wrong != "no_shift")
    W = V + 1 if wrong == "col_v" else V
    x = c.logits[:, :W].double()
    if wrong == "lost_last":
        lost_col = V - 1
    if lost_col is not None:
        x = x.clone()
        x[:, lost_col] = -math.inf
    lse = torch.logsumexp(x, 1)
    p = torch.exp(x - lse[:, None])
    xt = c.logits.double()  # the target's logit may lie past V for the wrong operations
    tl = xt[torch.arange(T), tgt.clamp(0, c.ldl - 1)]
    loss = torch.where(valid, lse - tl, torch.zeros_like(lse))
    hot = torch.zeros(T, c.ldl, dtype=f64)
    hot[torch.arange(T), (tgt + (1 if wrong == "hot_next" else 0)).clamp(0, c.ldl - 1)] = 1.0
    pf = torch.zeros(T, c.ldl, dtype=f64)
    pf[:, :W] = p
    pf[:, :V] = torch.where(x[:, :V] == -math.inf, torch.zeros_like(pf[:, :V]), pf[:, :V])
    dl = (pf - hot) / float(max(1, n) + (1 if wrong == "n_plus_1" else 0))
    dl = torch.where(valid[:, None], dl, torch.zeros_like(dl))
    rows = torch.full((T,), -1, dtype=torch.int32)
    pos = torch.full((T,), -1, dtype=torch.int32)
    idx = torch.nonzero(valid)[:, 0].int()
    rows[:idx.numel()] = idx
    pos[idx.long()] = torch.arange(idx.numel(), dtype=torch.int32)
    counts = torch.tensor([idx.numel(), (idx.numel() + 63) // 64 * 64], dtype=torch.int32)
    return NS(loss=loss, dlogits=dl, lse=lse, p=pf, hot=hot, valid=valid, tgt=tgt, n=max(1, n), rows=rows, pos=pos,
              counts=counts)


def xe_bounds(c, r):
    """Bounds of the per-row loss (fp32) and of dlogits (bf16) given the fp64 ``r`` of xe_ref.

    * The row maximum is exact.  A thread sums __expf(x - its own maximum) over its NCH*8 columns in sequence; the
      pairs (max, sum) are combined over 6 butterfly levels and 7 sequential wave combines, each combine rescaling one
      side by __expf(m - max) (the other by __expf(0) = 1) with a multiply and an add.  The gaps along a path add up to
      at most max - x_i, so column i's share of the sum carries u32 * (3*(max - x_i) + 8 + 8*NCH + 13*(8 + 2)), and the
      sum the p-weighted mean of that: ese = u32 * (3 * sum_i p_i*(max - x_i) + 8*NCH + 138).
    * lse = max + logf(sum): bl = ese + 2*u32*|log sum| + u32*|lse|; loss = lse - x[target]: bound bl + u32*(|loss| + bl).
    * p = __expf(x - lse^): ep = bl + u32*(3*|x - lse| + 8) relative.  g = (p - onehot) * fl(1/n): the difference, the
      division and the product are 3 roundings of |p - onehot|; at the target column the value is (p - 1)/n and its
      error is that of p, absolute.  d = (p*ep + 3*u32*|p - onehot|)/n;  bound(dlogits) = d + u16*(|ref| + d).
      Ignored rows and columns >= V are exactly 0 on both sides."""
    V = c.V
    x = c.logits[:, :V].double()
    mx = x.max(1).values
    p = r.p[:, :V]
    gap = torch.where(p > 0, p * (mx[:, None] - x), torch.zeros_like(p)).sum(1)
    ese = U32 * (3.0 * gap + 8.0 * c.NCH + 138.0)
    bl = ese + 2.0 * U32 * (r.lse - mx).abs() + U32 * r.lse.abs()
    bloss = torch.where(r.valid, bl + U32 * (r.loss.abs() + bl), torch.zeros_like(bl))
    ep = bl[:, None] + U32 * (3.0 * (x - r.lse[:, None]).abs() + 8.0)
    d = torch.zeros_like(r.dlogits)
    d[:, :V] = (p * ep + 3.0 * U32 * (p - r.hot[:, :V]).abs()) / r.n
    d = torch.where(r.valid[:, None], d, torch.zeros_like(d))
    return {"loss": bloss.clamp_min(FLOOR), "dlogits": (d + U16 * (r.dlogits.abs() + d)).clamp_min(FLOOR)}


def xe_emu(c, n_valid=None):
    """xent_kernel in float32: returns (row loss f32 [T], dlogits bf16 [T, ldl])."""
    V, T, ldl = c.V, c.T, c.ldl
    n = c.n_valid if n_valid is None else n_valid
    tgt, valid = xe_targets(c.labels, V)
    NCH = c.NCH
    W = NCH * 512 * 8
    x = torch.full((T, W), -math.inf, dtype=f32)
    x[:, :V] = c.logits[:, :V].float()
    xt = x.view(T, NCH, 512, 8)  # thread tid holds chunks tid + i*512
    mt = xt.amax((1, 3))  # [T, 512]
    safe = torch.where(mt == -math.inf, torch.zeros_like(mt), mt)
    e = _exp32(xt - safe[:, None, :, None])
    e = torch.where(xt == -math.inf, torch.zeros_like(e), e)
    se = torch.zeros(T, 512)
    for i in range(NCH):
        for j in range(8):
            se = se + e[:, i, :, j]

    def combine(m, s, m2, s2):
        mn = torch.maximum(m, m2)
        ok = mn != -math.inf
        mz = torch.where(ok, mn, torch.zeros_like(mn))
        a = torch.where(m == -math.inf, torch.zeros_like(s), s * _exp32(torch.where(m == -math.inf, mz, m) - mz))
        b = torch.where(m2 == -math.inf, torch.zeros_like(s2), s2 * _exp32(torch.where(m2 == -math.inf, mz, m2) - mz))
        return torch.where(ok, mn, m), torch.where(ok, a + b, s)

    m, s = mt.view(T, 8, 64), se.view(T, 8, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        m, s = combine(m, s, m[..., lane ^ o], s[..., lane ^ o])
    mx, sm = m[:, 0, 0], s[:, 0, 0]
    for w in range(1, 8):
        mx, sm = combine(mx, sm, m[:, w, 0], s[:, w, 0])
    lse = mx + torch.log(sm)
    tl = x[torch.arange(T), tgt.clamp(0, V - 1)]
    loss = torch.where(valid, lse - tl, torch.zeros(T))
    inv_n = torch.tensor(1.0, dtype=f32) / torch.tensor(float(max(1, n)), dtype=f32)
    hot = torch.zeros(T, V)
    hot[torch.arange(T), tgt.clamp(0, V - 1)] = 1.0
    g = (_exp32(x[:, :V] - lse[:, None]) - hot) * inv_n
    dl = torch.zeros(T, ldl)
    dl[:, :V] = torch.where(valid[:, None], g, torch.zeros_like(g))
    return loss, dl.bfloat16()


# =====================================================================================================================
# Emotion head and ergm_loss_finalize
# =====================================================================================================================
EMO_B, EMO_C, EMO_E, EMO_S = (1, 15, 16, 17, 33), (1, 7, 16), (64, 100, 768, 1024), (1, 8)
EMO_CASES = tuple((B, C, E, S) for B in EMO_B for C in EMO_C for E in EMO_E for S in EMO_S)
EMO_GS = 0.375
FIN_T = (1, 255, 256, 257, 2049)


@functools.lru_cache(maxsize=None)
def emo_case(B, C, E, S, family="benign"):
    """h bf16 [B*S, E] (rows other than S-1 of a sample hold NaN: the kernel must not read them), W f32 [C, E], labels
    with -100 and y == C among them, dh0 f32 [B*S, E].  ``dominant``: one logit leads by about 40."""
    name = f"emo-{family}-B{B}-C{C}-E{E}-S{S}"
    g = _gen(name)
    hl = torch.randn(B, E, generator=g)
    W = 0.02 * torch.randn(C, E, generator=g)
    if family == "dominant":
        W[C - 1] = W[C - 1] + 40.0 * hl[0].bfloat16().float() / hl[0].bfloat16().float().pow(2).sum()
        hl = hl[0:1].expand(B, E) * (1.0 + 0.01 * torch.arange(B, dtype=f32)[:, None])
    elif family != "benign":
        raise ValueError(family)
    labels = torch.randint(0, C, (B,), generator=g)
    if B >= 3:
        labels[1], labels[2] = -100, C
    h = torch.full((B, S, E), math.nan, dtype=bf16)
    h[:, S - 1] = hl.bfloat16()
    dh0 = torch.randn(B * S, E, generator=g)
    valid = (labels >= 0) & (labels < C)
    return NS(name=name, B=B, C=C, E=E, S=S, family=family, h=h.view(B * S, E), W=W, labels=labels, dh0=dh0,
              n_valid=int(valid.sum()), gs=EMO_GS)


def emo_ref(c, wrong=None):
    """fp64 emotion head: logits [B, C], loss_sum, dW [C, E], dh [B*S, E] (dh0 plus dlogits*W on the rows S-1)."""
    B, C, E, S = c.B, c.C, c.E, c.S
    hl = c.h.view(B, S, E)[:, S - 1].double()
    W = c.W.double()
    lg = hl @ W.T
    valid = (c.labels >= 0) & (c.labels < C)
    y = c.labels.clamp(0, C - 1)
    lse = torch.logsumexp(lg, 1)
    p = torch.exp(lg - lse[:, None])
    hot = torch.zeros(B, C, dtype=f64)
    hot[torch.arange(B), y] = 1.0
    n = B if wrong == "mean_b" else max(1, c.n_valid)
    dl = torch.where(valid[:, None], (p - hot) * c.gs / n, torch.zeros_like(p))
    loss = torch.where(valid, lse - lg[torch.arange(B), y], torch.zeros_like(lse))
    dlw = dl.clone()
    if wrong == "lost_sample":
        dlw[B - 1] = 0.0
    dh = c.dh0.double().clone().view(B, S, E)
    dh[:, S - 1] += dl @ W
    return NS(hl=hl, logits=lg, lse=lse, p=p, hot=hot, valid=valid, y=y, dl=dl, loss=loss, loss_sum=loss.sum().reshape(1),
              dW=dlw.T @ hl, dh=dh.view(B * S, E), n=n)


def emo_bounds(c, r):
    """Bounds of logits, loss_sum, dW and dh (all fp32) given the fp64 ``r`` of emo_ref; KL = ceil(E/64).

    * logit = wave_sum over lanes that each add KL products in sequence: bl = (KL + 7) * u32 * |h||W|^T.
    * Thread 0 takes the softmax of the kernel's own logits with expf (2 u32) of a rounded difference, C sequential
      adds: ese = u32 * (sum_c p_c*(max - l_c) + 2 + C); the logits' own errors move lse by mix = sum_c p_c*bl_c.
      row loss = (max + logf(sum)) - l_y: bl_y + mix + ese + 2*u32*|log sum| + u32*|lse| + u32*|loss|; loss_sum adds
      the B rows in sequence: sum_b of that + B * u32 * sum_b|loss_b|.
    * d = ((p - onehot) * gs) * fl(1/n), p = expf(.)/sum: ep = bl_c + mix + ese + u32*(max - l_c + 3) relative, and 4
      roundings of |p - onehot|: bd = (p*ep + 4*u32*|p - onehot|) * gs/n.
    * dW[c][e] = sum_b d[b][c]*h[b][e] in sequence: sum_b bd*|h| + (B + 1) * u32 * sum_b|d*h|.
    * dh[e] = dh0 + sum_c d[c]*W[c][e] in sequence: sum_c bd*|W| + (C + 2) * u32 * (|dh0| + sum_c|d*W|)."""
    B, C, E, S = c.B, c.C, c.E, c.S
    KL = (E + 63) // 64
    W = c.W.double()
    bl = (KL + 7) * U32 * (r.hl.abs() @ W.abs().T)
    mx = r.logits.max(1).values
    gap = mx[:, None] - r.logits
    mix = (r.p * bl).sum(1)
    ese = U32 * ((r.p * gap).sum(1) + 2.0 + C)
    brow = (bl[torch.arange(B), r.y] + mix + ese + 2.0 * U32 * (r.lse - mx).abs() + U32 * r.lse.abs()
            + U32 * r.loss.abs())
    brow = torch.where(r.valid, brow, torch.zeros_like(brow))
    bsum = brow.sum() + B * U32 * r.loss.abs().sum()
    ep = bl + (mix + ese)[:, None] + U32 * (gap + 3.0)
    bd = (r.p * ep + 4.0 * U32 * (r.p - r.hot).abs()) * abs(c.gs) / r.n
    bd = torch.where(r.valid[:, None], bd, torch.zeros_like(bd))
    bW = bd.T @ r.hl.abs() + (B + 1) * U32 * (r.dl.abs().T @ r.hl.abs())
    bh = torch.zeros(B, S, E, dtype=f64)
    d0 = c.dh0.double().view(B, S, E)[:, S - 1]
    bh[:, S - 1] = bd @ W.abs() + (C + 2) * U32 * (d0.abs() + r.dl.abs() @ W.abs())
    return {"logits": bl.clamp_min(FLOOR), "loss_sum": bsum.reshape(1).clamp_min(FLOOR), "dW": bW.clamp_min(FLOOR),
            "dh": bh.view(B * S, E).clamp_min(FLOOR)}


def emo_emu(c):
    """emotion_row_kernel and emotion_dw_kernel in float32: logits, loss_sum, dW, dh."""
    B, C, E, S = c.B, c.C, c.E, c.S
    hl = c.h.view(B, S, E)[:, S - 1].float()
    KL = (E + 63) // 64
    pad = torch.zeros(B, C, KL * 64)
    pad[:, :, :E] = hl[:, None, :] * c.W[None]
    lg = _tree(_seq(pad.view(B, C, KL, 64), 2))
    valid = (c.labels >= 0) & (c.labels < C)
    y = c.labels.clamp(0, C - 1)
    mx = lg.max(1).values
    e = torch.exp(lg - mx[:, None])
    se = _seq(e, 1)
    hot = torch.zeros(B, C)
    hot[torch.arange(B), y] = 1.0
    inv_n = torch.tensor(1.0, dtype=f32) / torch.tensor(float(max(1, c.n_valid)), dtype=f32)
    d = torch.where(valid[:, None], ((e / se[:, None] - hot) * torch.tensor(c.gs, dtype=f32)) * inv_n, torch.zeros(B, C))
    loss = torch.where(valid, (mx + torch.log(se)) - lg[torch.arange(B), y], torch.zeros(B))
    dW = _seq(d[:, :, None] * hl[:, None, :], 0)
    dh = c.dh0.clone().view(B, S, E)
    dh[:, S - 1] = dh[:, S - 1] + _seq(d[:, :, None] * c.W[None], 1)
    return lg, _seq(loss, 0).reshape(1), dW, dh.view(B * S, E)


@functools.lru_cache(maxsize=None)
def fin_case(T, emo=True):
    g = _gen(f"fin-{T}-{emo}")
    row_loss = 10.0 * torch.rand(T, generator=g)
    row_loss[::3] = 0.0  # ignored rows
    return NS(name=f"fin-T{T}-{'emo' if emo else 'lm'}", T=T, row_loss=row_loss, n_valid=max(1, int((row_loss > 0).sum())),
              emo_sum=torch.tensor([13.625 * 1.37], dtype=f32) if emo else None, n_emo=11)


def fin_ref(c):
    """fp64 ergm_loss_finalize: out[0] = sum(row_loss)/n_valid, out[1] = emo_sum/n_emo (0 without), out[2] = their sum."""
    lm = c.row_loss.double().sum() / c.n_valid
    emo = c.emo_sum.double()[0] / c.n_emo if c.emo_sum is not None else torch.tensor(0.0, dtype=f64)
    return torch.stack([lm, emo, lm + emo])


def fin_bounds(c, ref):
    """A thread adds ceil(T/256) values in sequence, then 6 butterfly levels, 3 adds over the 4 waves and a division:
    b0 = (ceil(T/256) + 10) * u32 * sum|row_loss|/n; out[1] is one division: u32*|out1|; out[2] one more add."""
    b0 = ((c.T + 255) // 256 + 10) * U32 * c.row_loss.double().abs().sum() / c.n_valid
    b1 = U32 * ref[1].abs()
    return torch.stack([b0, b1, b0 + b1 + U32 * ref[2].abs()]).clamp_min(FLOOR)


def fin_emu(c):
    T = c.T
    n = (T + 255) // 256
    p = torch.zeros(n * 256)
    p[:T] = c.row_loss
    w = _tree(_seq(p.view(n, 256), 0).view(4, 64))
    lm = (((w[0] + w[1]) + w[2]) + w[3]) / torch.tensor(float(c.n_valid), dtype=f32)
    emo = c.emo_sum[0] / torch.tensor(float(c.n_emo), dtype=f32) if c.emo_sum is not None else torch.tensor(0.0)
    return torch.stack([lm, emo, lm + emo])


# =====================================================================================================================
# Column sums
# =====================================================================================================================
CS_ROWS = (1, 63, 64, 65, 130)
CS_COLS = (4, 252, 256, 260)


@functools.lru_cache(maxsize=None)
def cs_case(rows, cols, dtype="f32"):
    g = _gen(f"cs-{rows}-{cols}-{dtype}")
    Xm = torch.randn(rows, cols, generator=g) + 0.5
    Xm = Xm.bfloat16() if dtype == "bf16" else Xm
    return NS(name=f"cs-{dtype}-r{rows}-c{cols}", rows=rows, cols=cols, dtype=dtype, X=Xm,
              out0=torch.randn(cols, generator=g))


def cs_ref(c, accumulate, wrong=None):
    Xd = c.X.double().clone()
    if wrong == "lost_row":
        Xd[c.rows - 1] = 0.0
    if wrong == "lost_cols":
        Xd[:, 256:260] = 0.0
    return Xd.sum(0) + (c.out0.double() if accumulate else 0.0)


def cs_bounds(c, accumulate):
    """A row lane adds CS_ROWS/4 = 16 rows in sequence, the 4 lanes add in sequence (3), the partial blocks of 64 rows
    add in sequence when there are more than one (nparts), the old value adds once more with ``accumulate``:
    (19 + [nparts > 1]*nparts + [accumulate]) * u32 * (sum_r|X| + |out0|)."""
    nparts = (c.rows + 63) // 64
    depth = 19 + (nparts if nparts > 1 else 0) + (1 if accumulate else 0)
    mag = c.X.double().abs().sum(0) + (c.out0.double().abs() if accumulate else 0.0)
    return (depth * U32 * mag).clamp_min(FLOOR)


def cs_emu(c, accumulate):
    rows, cols = c.X.shape
    nparts = (rows + 63) // 64
    p = torch.zeros(nparts * 64, cols)
    p[:rows] = c.X.float()
    part = _seq(_seq(p.view(nparts, 16, 4, cols), 1), 1)  # rows r0 + rl + 4k in sequence, then the 4 row lanes
    if nparts == 1:
        return part[0] + c.out0 if accumulate else part[0]
    s = _seq(part, 0)
    return s + c.out0 if accumulate else s


# =====================================================================================================================
# The case matrix tests/test_gpu_rows_matrix.py runs and tests/test_rows_bound.py admits the emulation on
# =====================================================================================================================
def ln_matrix():
    """(E, rows, family, dy family): every E x rows on benign inputs, the long case, every family (and the single-row
    dy) at the two family shapes."""
    out = [(E, rows, "benign", "randn") for E in LN_E for rows in LN_ROWS] + [LN_LONG + ("benign", "randn")]
    for E, rows in LN_FAMILY_SHAPES:
        out += [(E, rows, fam, "randn") for fam in LN_FAMILIES if fam != "benign"] + [(E, rows, "benign", "single")]
    return out


def xe_matrix():
    """(V, ldl, (B, S), family, pad): every shape on benign inputs in both label layouts (5 + 3 scored rows, the pad
    columns holding 1e4 in one and NaN in the other); peaked, offset, flat and wide at the NCH = 4 and NCH = 16 shapes,
    the layout and the pad alternating; ``edge`` at EVERY shape in as many parts of 8 scored rows as put the row maximum
    on every column of xe_edges(V): 1 part at V = 203, 4096 (2 edges) and 8193 (5), 2 at 16390 (10) and 32768 (16), 4 at
    50260 (26), 53250 (28) and 65536 (32: every chunk set of xent_kernel<16>)."""
    out = []
    for i, (V, ldl) in enumerate(XE_SHAPES):
        out += [(V, ldl, XE_BS[k], "benign", ("big", "nan")[(i + k) % 2]) for k in range(2)]
        out += [xe_edge_case(V, ldl, k) for k in range(xe_edge_parts(V))]
    for V, ldl in XE_FAMILY_SHAPES:
        out += [(V, ldl, XE_BS[j % 2], fam, ("nan", "big")[j % 2]) for j, fam in enumerate(XE_FAMILIES[1:5])]
    return out


def emo_matrix():
    return [c + ("benign",) for c in EMO_CASES] + [(17, 7, 768, 8, "dominant"), (16, 16, 100, 1, "dominant")]


def cs_matrix():
    return [(rows, cols, dt) for rows in CS_ROWS for cols in CS_COLS for dt in ("f32", "bf16")]
