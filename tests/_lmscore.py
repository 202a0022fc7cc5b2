"""ergm_lm_score (lmscore.hip) on the CPU: the cases of tests/test_gpu_lmscore_ops.py, an fp64 reference on exactly the
bf16 inputs the kernel gets, elementwise error bounds counted from the kernel's rounding points, and a plain float32
restatement of its partition and combine order.  Imports no GPU code; tests/test_lmscore_bound.py checks the bounds
here, from both sides, without a GPU.  Conventions (u32, the __expf charge, the floor, no fitting, no element
excluded) are those of tests/_rows.py.

The kernel.  The vocabulary is cut into partitions of PW = TPP * BN columns; inside a partition, lane l (0..15) of a
row sees the columns congruent to l mod 16, 8 per column tile, tile after tile; the 16 lanes then meet in an xor
butterfly (1, 2, 4, 8) and the partitions are folded in ascending order by a second kernel.

Bounds.
* logit x_j: the GEMM matrix test's 2*K*u32*sum_k |x_k||w_jk| (bx).
* lse = m + logf(s): as a function of the logits, d lse = sum_j p_j dx_j, so the logit errors enter p-weighted.  The
  online combine: column j's share of s is exp(x_j - m) formed as a product of __expf factors whose exponents' gaps
  add up to at most m - x_j along the path (3*u32*(m - x_j) in all) and whose count is at most 1 (its own) + 3 (later
  tiles of the lane) + 4 (butterfly) + P - 1 (partitions), each charged 8*u32 plus the multiply and the add of its
  combine (2*u32), plus the at most 8 adds of each of the lane's 4 tile sums:
      ese = u32 * (3 * sum_j p_j (m - x_j) + 10 * (8 + P - 1) + 32)   relative on s, absolute on log s;
  logf is within 2*u32 of |log s| and the final add rounds lse: bl = sum_j p_j bx_j + ese + 2*u32*|log s| + u32*|lse|.
* logprob = x_t - lse: bound bx_t + bl + u32 * (|logprob| + bx_t + bl); an unscored row is exactly 0.
* top1: the returned column c must hold a logit within bx_c + bx_a of the fp64 maximum (a its column), and
  top1_logit must be within bx_c of the fp64 logit of column c; where the fp64 margin between the maximum and the
  runner-up exceeds both their bounds the column itself is demanded.
"""
import functools
import math
import types
import zlib

import torch

U32 = 2.0 ** -24
FLOOR = 2.0 ** -100
LOG2E32 = torch.tensor(1.4426950408889634, dtype=torch.float32)
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
NS = types.SimpleNamespace
INF = math.inf

BM, BN, TPP = 64, 128, 4  # LS_BM, LS_BN, LS_TPP of lmscore.hip
PW = BN * TPP             # columns of a vocabulary partition

ROWS = (1, 15, 16, 17, 33, BM - 1, BM, BM + 1, 2 * BM + 3)
DEPTHS = (64, 192, 768, 1024)
VOCABS = ((203, 208), (BN, BN), (BN + 1, BN + 8), (PW + 1, PW + 8))  # the last: one column past a partition edge
BIG = (50257, 50304)
BIG_ROWS = (1, 15, 16, 17, 33)
BIG_K = 768
FAMILIES = ("benign", "wide", "peaked", "edge", "tie")
FAMILY_SHAPES = ((33, 192, (PW + 1, PW + 8)), (33, 768, BIG))


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def parts(V):
    return (V + PW - 1) // PW


def edges(V):
    """V-1 and 0, then the last and first column of every column tile (every 4th one a partition's) below V-1."""
    e = [V - 1, 0]
    for c in range(BN, V, BN):
        for x in (c - 1, c):
            if x < V - 1 and x not in e:
                e.append(x)
    return e


def edge_parts(V, R):
    """How many ``edge`` cases of R scored rows put the row maximum on every column of edges(V) once."""
    return (len(edges(V)) + R - 1) // R


def edge_plan(V, R, part):
    """(maximum, target) columns of the R rows of ``edge`` part ``part``: consecutive edge columns, cyclically."""
    e = edges(V)
    return [(e[(R * part + j) % len(e)], e[(R * part + j + 1) % len(e)]) for j in range(R)]


def target_list(V):
    """0, V-1, both sides of every tile and partition edge there is (the first two tiles, the first partition), and
    the unscored values."""
    t = [0, V - 1, -100, V // 2, V, V + 7]
    for c in (BN - 1, BN, 2 * BN - 1, 2 * BN, PW - 1, PW, V - 2):
        if 0 <= c < V and c not in t:
            t.append(c)
    return t


@functools.lru_cache(maxsize=4)
def _base_w(wrows, K, scale):
    return torch.randn(wrows, K, generator=_gen(f"lmscore-w-{wrows}-{K}")) * (scale / math.sqrt(K))


@functools.lru_cache(maxsize=2)
def case(R, K, vw, family="benign", part=0):
    """X bf16 [R, K], W bf16 [wrows, K] (rows at or past V: 1e4 or NaN, alternating with the case), targets int64 [R].
    ``planted``: rows whose maximum column is known by construction (edge, peaked, tie) -> that column."""
    V, wrows = vw
    name = f"lmscore-{family}{part or ''}-R{R}-K{K}-V{V}"
    g = _gen(name)
    X = torch.randn(R, K, generator=g)
    W = _base_w(wrows, K, 25.0 if family == "wide" else 3.0).clone()
    tl = target_list(V)
    targets = torch.tensor([tl[(r + K // 64) % len(tl)] for r in range(R)], dtype=torch.int64)
    planted = {}
    n2 = (X.double() ** 2).sum(1)
    coef = {}  # column -> {row: logit planted for that row}

    def plant(col, row, val):
        coef.setdefault(col, {})[row] = val

    if family == "edge":  # every row scored: maximum on one edge column, target on the next
        assert 0 <= part < edge_parts(V, R)
        for r, (cmax, ctgt) in enumerate(edge_plan(V, R, part)):
            plant(cmax, r, 60.0)
            if ctgt != cmax:
                plant(ctgt, r, 30.0)
            targets[r] = ctgt
            planted[r] = cmax
    elif family == "peaked":  # +60 on the target / beside it, alternating over the scored rows
        used = set()
        for r in range(R):
            t = int(targets[r])
            col = (t if r % 2 == 0 else (t + 1) % V) if 0 <= t < V else (7 * r + 3) % V
            if col in used:
                continue
            used.add(col)
            plant(col, r, 60.0)
            planted[r] = col
    elif family == "tie":  # two identical rows of W: across a tile edge, a partition edge, inside a tile, a lane
        pairs = [(BN - 1, BN), (5, PW + 5), (3, 9), (4, 4 + BN), (0, V - 1), (V - 2, V - 1)]
        used = set()
        for r, (c1, c2) in enumerate(pairs[:R]):
            if c1 >= c2 or c2 >= V or c1 in used or c2 in used:
                continue
            used |= {c1, c2}
            plant(c1, r, 60.0)
            plant(c2, r, 60.0)
            planted[r] = c1
    elif family not in ("benign", "wide"):
        raise ValueError(family)
    for col, rows in coef.items():
        W[col] = sum((val / n2[r]) * X[r].double() for r, val in rows.items()).float()
    Wb = torch.full((wrows, K), 1e4 if zlib.crc32(name.encode()) % 2 == 0 else math.nan, dtype=bf16)
    Wb[:V] = W[:V].bfloat16()
    ties = []
    if family == "tie":  # the same bits in both rows
        for r, c1 in planted.items():
            c2 = [c for c, rows in coef.items() if r in rows and c != c1][0]
            Wb[c2] = Wb[c1]
            ties.append((c1, c2))
    return NS(name=name, R=R, K=K, V=V, wrows=wrows, family=family, X=X.bfloat16(), W=Wb, targets=targets,
              planted=planted, ties=ties, P=parts(V))


def ref(c, wrong=None):
    """fp64 reference of case ``c``: logits x [R, V], lse, top1 (first maximum), top1_logit, logprob (0 on unscored
    rows), p, valid.  ``wrong`` selects a deliberately WRONG operation (tests/test_lmscore_bound.py)."""
    V = c.V
    Wd = c.W[:V + 1 if wrong == "col_v" else V].double()
    x = c.X.double() @ Wd.T
    xs = x.clone()
    if wrong == "lost_last":
        xs[:, V - 1] = -INF
    if wrong == "drop_last_part":
        xs[:, (c.P - 1) * PW:] = -INF
    if wrong == "no_rescale":  # every partition's sum taken relative to its own maximum, added as if to the row's
        m = xs.max(1).values
        s = torch.zeros_like(m)
        for p in range(c.P):
            xp = xs[:, p * PW:(p + 1) * PW]
            s = s + torch.exp(xp - xp.max(1, keepdim=True).values).sum(1)
        lse = m + torch.log(s)
    else:
        lse = torch.logsumexp(xs, 1)
    top1 = xs.argmax(1)
    valid = (c.targets >= 0) & (c.targets < V)
    tcol = (c.targets + (1 if wrong == "target_next" else 0)).clamp(0, x.shape[1] - 1)
    xt = x[torch.arange(c.R), tcol]
    logprob = torch.where(valid, xt - lse, torch.zeros_like(lse))
    return NS(x=x[:, :V], lse=lse, top1=top1, top1_logit=xs.max(1).values, logprob=logprob, valid=valid,
              p=torch.exp(x[:, :V] - torch.logsumexp(x[:, :V], 1)[:, None]), tcol=c.targets.clamp(0, V - 1))


def bounds(c, r):
    """bx [R, V] and the bounds of lse, logprob (module docstring) given the fp64 ``r`` of ref(c)."""
    V = c.V
    bx = (2.0 * c.K * U32) * (c.X.double().abs() @ c.W[:V].double().abs().T)
    m = r.x.max(1).values
    gap = torch.where(r.p > 0, r.p * (m[:, None] - r.x), torch.zeros_like(r.p)).sum(1)
    ese = U32 * (3.0 * gap + 10.0 * (8 + c.P - 1) + 32.0)
    bl = (r.p * bx).sum(1) + ese + 2.0 * U32 * (r.lse - m).abs() + U32 * r.lse.abs()
    bxt = bx[torch.arange(c.R), r.tcol]
    blp = bxt + bl + U32 * (r.logprob.abs() + bxt + bl)
    blp = torch.where(r.valid, blp, torch.zeros_like(blp))
    return NS(x=bx.clamp_min(FLOOR), lse=bl.clamp_min(FLOOR), logprob=blp)


def margins_ok(c, r, b):
    """Per row: does the fp64 margin between the maximum and the runner-up exceed both their logit bounds?"""
    top2 = r.x.topk(min(2, c.V), 1)
    if c.V < 2:
        return torch.ones(c.R, dtype=torch.bool)
    rows = torch.arange(c.R)
    return (top2.values[:, 0] - top2.values[:, 1]) > b.x[rows, top2.indices[:, 0]] + b.x[rows, top2.indices[:, 1]]


def ratio(got, want, b):
    """Largest err/bound; a NaN or inf in ``got`` where ``want`` is finite counts as infinite; a zero bound demands
    equality."""
    got = got.double()
    if (~torch.isfinite(got) & torch.isfinite(want)).any().item():
        return INF
    err = (got - want).abs()
    e = torch.where(err == 0, torch.zeros_like(err), err / b)
    return torch.where(torch.isfinite(want), e, torch.zeros_like(e)).max().item()


def judge(c, r, b, logprob, lse, top1_logit, top1):
    """err/bound of the four outputs of one run against ref / bounds; top1 is 0 where the column is acceptable (the
    planted column on planted rows and wherever the fp64 margin decides, else a column within the two bounds), inf
    where not; top1_logit is judged against the fp64 logit of the column returned."""
    rows = torch.arange(c.R)
    t = top1.long()
    inside = ((t >= 0) & (t < c.V)).all().item()
    res = {"lse": ratio(lse, r.lse, b.lse), "logprob": ratio(logprob, r.logprob, b.logprob)}
    if not inside:
        res["top1"] = res["top1_logit"] = INF
        return res
    res["top1_logit"] = ratio(top1_logit, r.x[rows, t], b.x[rows, t])
    exact = margins_ok(c, r, b)
    for row in c.planted:
        exact[row] = True
    near = (r.top1_logit - r.x[rows, t]) <= b.x[rows, t] + b.x[rows, r.top1]
    good = torch.where(exact, t == r.top1, near)
    res["top1"] = 0.0 if good.all().item() else INF
    return res


def _exp32(a):
    """__expf in float32: exp2(a * log2e), the product rounded."""
    return torch.exp2(a * LOG2E32)


def _combine(m, s, i, m2, s2, i2, rescale=True):
    """ls_combine of lmscore.hip on float32 tensors."""
    take = (m2 > m) | ((m2 == m) & (i2 < i))
    i = torch.where(take, i2, i)
    mn = torch.maximum(m, m2)
    ok = mn != -INF
    mz = torch.where(ok, mn, torch.zeros_like(mn))
    if rescale:
        a = torch.where(m == -INF, torch.zeros_like(s), s * _exp32(torch.where(m == -INF, mz, m) - mz))
        b = torch.where(m2 == -INF, torch.zeros_like(s2), s2 * _exp32(torch.where(m2 == -INF, mz, m2) - mz))
    else:
        a, b = s, s2
    return torch.where(ok, mn, m), torch.where(ok, a + b, s), i


def emu(c, x32=None):
    """lm_score_kernel + lm_score_combine_kernel in float32 from float32 logits (a float32 matrix product of the bf16
    operands unless given).  Returns (logprob, lse, top1_logit, top1)."""
    R, V, P = c.R, c.V, c.P
    if x32 is None:
        x32 = c.X.float() @ c.W[:V].float().T
        for c1, c2 in c.ties:  # identical rows of W give identical logits on the GPU, whatever the host's blocking does
            x32[:, c2] = x32[:, c1]
    x = torch.full((R, P * PW), -INF, dtype=f32)
    x[:, :V] = x32
    col = torch.arange(P * PW, dtype=torch.int64).view(P, TPP, BN // 16, 16)
    x = x.view(R, P, TPP, BN // 16, 16)  # [row, partition, tile, j, lane]: column = base + 16 j + lane
    big = torch.iinfo(torch.int32).max
    rm = torch.full((R, P, 16), -INF, dtype=f32)
    rs = torch.zeros(R, P, 16, dtype=f32)
    ri = torch.full((R, P, 16), big, dtype=torch.int64)
    for t in range(TPP):
        xt = x[:, :, t]  # [R, P, 8, 16]
        tmax, tj = xt.max(2)  # the first maximum: ascending columns
        tidx = torch.gather(col[:, t].expand(R, P, BN // 16, 16), 2, tj[:, :, None, :])[:, :, 0, :]
        ri = torch.where(tmax > rm, tidx, ri)
        mn = torch.maximum(rm, tmax)
        ok = mn != -INF
        mz = torch.where(ok, mn, torch.zeros_like(mn))
        s = torch.where(rm == -INF, torch.zeros_like(rs), rs * _exp32(torch.where(rm == -INF, mz, rm) - mz))
        for j in range(BN // 16):
            e = _exp32(xt[:, :, j] - mz)
            s = s + torch.where(xt[:, :, j] == -INF, torch.zeros_like(e), e)
        rs = torch.where(ok, s, rs)
        rm = torch.where(ok, mn, rm)
    lane = torch.arange(16)
    for off in (1, 2, 4, 8):
        rm, rs, ri = _combine(rm, rs, ri, rm[..., lane ^ off], rs[..., lane ^ off], ri[..., lane ^ off])
    m, s, i = rm[:, 0, 0], rs[:, 0, 0], ri[:, 0, 0]
    for p in range(1, P):
        m, s, i = _combine(m, s, i, rm[:, p, 0], rs[:, p, 0], ri[:, p, 0])
    lse = m + torch.log(s)
    valid = (c.targets >= 0) & (c.targets < V)
    xtg = x32[torch.arange(R), c.targets.clamp(0, V - 1)]
    logprob = torch.where(valid, xtg - lse, torch.zeros(R, dtype=f32))
    return logprob, lse, m, i.clamp(0, V - 1).int()


def matrix():
    """The benign cases of the GPU matrix: (R, K, (V, rows of W))."""
    for R in ROWS:
        for K in DEPTHS:
            for vw in VOCABS:
                yield R, K, vw
    for R in BIG_ROWS:
        yield R, BIG_K, BIG


def family_cases():
    """(R, K, vw, family, part) of every family at FAMILY_SHAPES; ``edge`` in as many parts as cover edges(V)."""
    for R, K, vw in FAMILY_SHAPES:
        for fam in FAMILIES:
            for part in range(edge_parts(vw[0], R) if fam == "edge" else 1):
                yield R, K, vw, fam, part
