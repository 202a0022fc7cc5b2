"""Attention (head dim 64) on the CPU: the cases of tests/test_gpu_attn_matrix.py, the fp64 reference of the forward
and of the backward *formula* the kernels implement, the elementwise error bound, and a plain float32 restatement of
the kernels' rounding points.  Imports no GPU code; tests/test_attn_bound.py checks the bound here, without a GPU.

Tensors are [B, H, S, 64]; ``to_rows`` / ``from_rows`` convert to and from the kernels' token-major [B*S, H*64].

Reference (fp64 on the bf16-rounded operands, per (b, h)).  S = Q K^T / 8, masked to -inf; LSE = logsumexp(S);
P = exp(S - LSE); O = P~ V with P~ = P * Z, Z = keep / (1 - p) (all ones without dropout; keep from oracle/philox.py,
rows (b*H + h)*Sq + q, cols Sk).  The backward takes ``o_in`` (bf16) and ``lse_in`` (fp32) as inputs, as the kernels
do: P = exp(S - lse_in), dP = dO V^T, delta = rowsum(dO * o_in), dS = P * (dP * Z - delta), dV = P~^T dO,
dK = dS^T Q / 8, dQ = dS K / 8.
"""
import functools
import math
import types
import zlib

import torch

from oracle import philox as X

U16, U32 = 2.0 ** -8, 2.0 ** -24
FLOOR = 2.0 ** -100
LOG2E = 1.4426950408889634
GATE = {"O": 8e-3, "LSE": 1e-4, "dQ": 2e-2, "dK": 2e-2, "dV": 2e-2}  # the older tests' relative Frobenius norms
WORST = {}  # family -> output -> largest err/bound seen


def to_rows(x):
    """[B, H, S, 64] -> token-major [B*S, H*64]."""
    B, H, S, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * D)


def from_rows(x, B, H):
    """Token-major [B*S, H*64] -> [B, H, S, 64]."""
    return x.reshape(B, x.shape[0] // B, H, 64).permute(0, 2, 1, 3)


def visible(Sq, Sk, causal):
    v = torch.ones(Sq, Sk, dtype=torch.bool)
    return v.tril() if causal else v


# ---- fp64 reference -------------------------------------------------------------------------------------------------
def ref_fwd(q, k, v, vis, Z=None, sum_after_drop=False):
    """q, k, v fp64 [B, H, S, 64]; vis bool, broadcastable to [B, H, Sq, Sk]; Z = keep/(1-p) or None.
    ``sum_after_drop`` is a deliberately WRONG operation (the row sum taken over the dropped probabilities) that
    tests/test_attn_bound.py uses as a mutation."""
    S = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~vis, -math.inf)
    Z = torch.ones_like(S) if Z is None else Z
    if sum_after_drop:
        m = S.max(-1, keepdim=True).values
        E = torch.exp(S - m) * Z
        lsum = E.sum(-1, keepdim=True)
        return types.SimpleNamespace(S=S, P=E / lsum, Pt=E / lsum, O=(E / lsum) @ v, LSE=(m + lsum.log())[..., 0], Z=Z)
    LSE = torch.logsumexp(S, -1)
    P = torch.exp(S - LSE[..., None])
    return types.SimpleNamespace(S=S, P=P, Pt=P * Z, O=(P * Z) @ v, LSE=LSE, Z=Z)


def ref_bwd(q, k, v, do, o_in, lse_in, vis, Z=None):
    """The backward formula on fp64 copies of the kernel's inputs (o_in: the bf16 O, lse_in: the fp32 LSE)."""
    S = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~vis, -math.inf)
    Z = torch.ones_like(S) if Z is None else Z
    P = torch.exp(S - lse_in[..., None])
    dP = do @ v.transpose(-1, -2)
    delta = (do * o_in).sum(-1)
    dS = P * (dP * Z - delta[..., None])
    Pt = P * Z
    return types.SimpleNamespace(P=P, Pt=Pt, dP=dP, delta=delta, dS=dS, Z=Z, dV=Pt.transpose(-1, -2) @ do,
                                 dK=dS.transpose(-1, -2) @ q / 8.0, dQ=dS @ k / 8.0)


# ---- the bound ------------------------------------------------------------------------------------------------------
def _eP(Sabs, lse):
    return U32 * (64.0 * Sabs + 4.0 * lse.abs()[..., None] + 8.0)


def fwd_bounds(q, k, v, r):
    """Elementwise error bounds of O (bf16) and LSE (fp32) given the fp64 reference ``r`` of ref_fwd.

    Derivation, from the kernels' rounding points (nothing is fitted to kernel output); u16 = 2^-8 and u32 = 2^-24 are
    the unit roundoffs of bf16 and fp32, |X| is elementwise, Sabs = |Q||K|^T / 8.

    * A score is an fp32 sum of 64 exact bf16 products: off by at most 64*u32*Sabs*8 before the scale, 64*u32*Sabs
      after it.  A probability is recomputed as exp2(fma(s, c, -shift*log2e)) with one v_exp_f32: the score's error,
      the rounding of c = log2e/8 and of shift*log2e (u32 each, on magnitudes Sabs and |shift|), the FMA's own rounding
      and the few ulp of v_exp_f32 give the RELATIVE error eP = u32*(64*Sabs + 4*|LSE| + 8) of a probability (the
      forward's shift is the running maximum and a final division by l; both are within |LSE| + log Sk of the score
      and enter the same way).
    * O = bf16((sum_k bf16(P~) V) / l): P~ is rounded to bf16 by RNE before the second MFMA (u16*T, T = P~|V|), carries
      eP ((P~*eP)|V|), and the products are summed in fp32 in an order MFMA does not specify (Sk*u32*T).  As for the
      GEMMs the sum of these is doubled for the rescales by alpha between key tiles, the division by l (whose relative
      error is a P-weighted mean of eP plus summation error, all within the same three terms) and the rounding of a
      value that already carries an error; the final bf16 rounding is u16*|O|.
      bound(O) = u16*|O| + 2*(u16*T + (P~*eP)|V| + Sk*u32*T).
    * LSE = m/8 + logf(l): an ABSOLUTE error equal to the relative error of l (at most the largest eP of the row, whose
      Sabs term is rowmax over the visible pairs) plus logf's few ulp and the final add, both relative to |LSE|:
      bound(LSE) = u32*(2*|LSE| + 64*rowmax(Sabs) + 16).
    * Everywhere an absolute floor of 2^-100: fp32 / bf16 subnormals are the only place where rounding is not relative,
      and 2^-100 is far below anything a wrong element produces."""
    Sabs = q.abs() @ k.abs().transpose(-1, -2) / 8.0
    eP = _eP(Sabs, r.LSE)
    T = r.Pt @ v.abs()
    Sk = k.shape[-2]
    bO = U16 * r.O.abs() + 2.0 * (U16 * T + (r.Pt * eP) @ v.abs() + Sk * U32 * T)
    rowmax = Sabs.masked_fill(r.S == -math.inf, 0.0).max(-1).values
    bL = U32 * (2.0 * r.LSE.abs() + 64.0 * rowmax + 16.0)
    return {"O": bO.clamp_min(FLOOR), "LSE": bL.clamp_min(FLOOR)}


def bwd_bounds(q, k, v, do, o_in, lse_in, rb):
    """Elementwise error bounds of dQ, dK, dV (bf16) and delta (fp32) given the fp64 ``rb`` of ref_bwd.

    Same rounding points as fwd_bounds: P~ and dS are rounded to bf16 (pack_p / f2bf) before the second MFMA, every
    accumulation is fp32, one v_exp_f32 per score with the relative error eP (its shift is lse_in*log2e).
    * dS = P*(dP*Z - delta): dP and delta are fp32 sums of 64 exact products, so their difference is off by
      64*u32*(|dO||V|^T*Z + rowsum(|dO||o_in|)) ABSOLUTELY, however small the difference itself is (without this term
      a row whose softmax is one-hot has reference and bound both 0); P carries eP; the result is rounded to bf16:
      D(dS) = u16*|dS| + P*(eP*|dP*Z - delta| + 64*u32*(|dO||V|^T*Z + rowsum(|dO||o_in|))).
    * dV = bf16(bf16(P~)^T dO):  u16*|dV| + 2*((u16*P~ + P~*eP)^T|dO| + Sq*u32*P~^T|dO|).
    * dK = bf16(bf16(dS)^T Q / 8): u16*|dK| + 2*(D(dS)^T|Q|/8 + Sq*u32*|dS|^T|Q|/8); dQ likewise over the keys with |K|.
      The division by 8 is exact.  The factor 2 is the GEMM bound's (unspecified MFMA order; rounding a value that
      already carries an error).
    * delta: 2*64*u32*rowsum(|dO||o_in|).
    * The 2^-100 floor of fwd_bounds."""
    Sq, Sk = q.shape[-2], k.shape[-2]
    Sabs = q.abs() @ k.abs().transpose(-1, -2) / 8.0
    eP = _eP(Sabs, lse_in)
    Tdelta = (do.abs() * o_in.abs()).sum(-1)
    cancel = 64.0 * U32 * ((do.abs() @ v.abs().transpose(-1, -2)) * rb.Z + Tdelta[..., None])
    dDS = U16 * rb.dS.abs() + rb.P * (eP * (rb.dP * rb.Z - rb.delta[..., None]).abs() + cancel)
    dDS = torch.where(rb.P > 0, dDS, torch.zeros_like(dDS))  # masked pairs: exactly 0 on both sides
    Pt = rb.Pt
    bV = U16 * rb.dV.abs() + 2.0 * ((U16 * Pt + Pt * eP).transpose(-1, -2) @ do.abs()
                                    + Sq * U32 * (Pt.transpose(-1, -2) @ do.abs()))
    bK = U16 * rb.dK.abs() + 2.0 * (dDS.transpose(-1, -2) @ q.abs() / 8.0
                                    + Sq * U32 * (rb.dS.abs().transpose(-1, -2) @ q.abs()) / 8.0)
    bQ = U16 * rb.dQ.abs() + 2.0 * (dDS @ k.abs() / 8.0 + Sk * U32 * (rb.dS.abs() @ k.abs()) / 8.0)
    bD = 2.0 * 64.0 * U32 * Tdelta
    return {n: b.clamp_min(FLOOR) for n, b in (("dQ", bQ), ("dK", bK), ("dV", bV), ("delta", bD))}


def ratio(got, ref, b):
    """Largest err/bound; a NaN anywhere in ``got`` counts as infinite."""
    got = got.double()
    if torch.isnan(got).any().item():
        return math.inf
    return ((got - ref).abs() / b).max().item() if got.numel() else 0.0


def norm_gate(what, out, got, ref, gate=True):
    """The older tests' relative Frobenius norm over the whole tensor (GATE), the check that sees a small error of one
    sign on every element.  It always runs, except on the outputs a caller names in ``ungated`` (below), and an error
    of exactly 0 passes whatever the reference's norm (flat inputs: dK = dS^T 0 = 0 on both sides)."""
    tol = GATE.get(out)
    if not gate or tol is None:
        return
    err = (got.double() - ref).norm().item()
    rel = 0.0 if err == 0.0 else err / max(ref.norm().item(), 1e-300)
    assert rel < tol, f"{what} {out}: relative norm error {rel:.3g} past the gate {tol:g}"


def ungated(c):
    """The outputs of case ``c`` whose reference is 0 up to rounding, so that a relative norm says nothing (the
    elementwise bound, which has an absolute term for exactly this, still holds them): with one-hot routing, or a
    single key, every row's softmax is one-hot, dP*Z - delta cancels to rounding noise and dS, dQ, dK are ~0."""
    return ("dQ", "dK") if c.family == "routing" or c.Sk == 1 else ()


def check(what, out, got, ref, b, family=None, gate=True):
    """``got`` against the fp64 ``ref`` of output ``out`` (O, LSE, dQ, dK, dV, delta): no NaN, every element within the
    bound ``b`` (the first offender reported with got / want), then norm_gate as a second opinion (``gate=False``:
    the caller found ``out`` in ungated(case)).  Returns, and records under ``family``, the worst err/bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, out, got.shape, ref.shape)
    assert not torch.isnan(got).any().item(), f"{what} {out}: NaN in the result"
    err = (got - ref).abs()
    worst = (err / b).max().item() if err.numel() else 0.0
    if family is not None:
        w = WORST.setdefault(family, {})
        w[out] = max(w.get(out, 0.0), worst)
    bad = err > b
    if bad.any().item():
        i = tuple(int(x) for x in torch.nonzero(bad)[0])
        raise AssertionError(f"{what} {out}: {int(bad.sum())} of {bad.numel()} elements past the bound, worst "
                             f"err/bound {worst:.3g}, first at (b, h, row[, col]) = {i}: got {got[i].item()!r} want "
                             f"{ref[i].item()!r} bound {b[i].item():.3g}")
    norm_gate(what, out, got, ref, gate)
    return worst


def report(family):
    w = WORST.get(family, {})
    print(f"{family}: worst err/bound " + "  ".join(f"{k} {w[k]:.4f}" for k in ("O", "LSE", "dQ", "dK", "dV", "delta")
                                                     if k in w))


# ---- float32 emulation of the kernels' rounding points --------------------------------------------------------------
def _bf(x):
    return x.bfloat16().float()


def emu_fwd(q, k, v, vis, Z=None):
    """Online softmax over 64-key tiles in the exp2 domain, bf16 P~ before the PV product, fp32 everywhere else.
    q, k, v float32 holding bf16 values.  Returns (O bf16, LSE fp32)."""
    B, H, Sq, _ = q.shape
    Sk = k.shape[-2]
    c = torch.tensor(0.125 * LOG2E, dtype=torch.float32)
    s = (q @ k.transpose(-1, -2)).masked_fill(~vis, -math.inf)  # raw scores
    Z = torch.ones_like(s) if Z is None else Z.float()
    m = torch.full((B, H, Sq, 1), -math.inf)
    l = torch.zeros(B, H, Sq, 1)
    o = torch.zeros(B, H, Sq, 64)
    for k0 in range(0, Sk, 64):
        st = s[..., k0:k0 + 64]
        mnew = torch.maximum(m, st.max(-1, keepdim=True).values)
        m2 = torch.where(mnew == -math.inf, torch.zeros_like(mnew), mnew) * c
        alpha = torch.exp2(m * c - m2)
        p = torch.exp2(st * c - m2)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + _bf(p * Z[..., k0:k0 + 64]) @ v[..., k0:k0 + 64, :]
        m = mnew
    return (o * (1.0 / l)).bfloat16(), (m * 0.125 + l.log())[..., 0]


def emu_bwd(q, k, v, do, o_in, lse_in, vis, Z=None):
    """The backward with P recomputed by exp2, bf16 P~ and dS before the second product.  Returns bf16 dQ, dK, dV."""
    c = torch.tensor(0.125 * LOG2E, dtype=torch.float32)
    s = q @ k.transpose(-1, -2)
    Z = torch.ones_like(s) if Z is None else Z.float()
    p = torch.exp2(s * c - (lse_in * torch.tensor(LOG2E, dtype=torch.float32))[..., None])
    p = torch.where(vis, p, torch.zeros_like(p))
    dp = do @ v.transpose(-1, -2)
    delta = (do * o_in).sum(-1, keepdim=True)
    pt, ds = _bf(p * Z), _bf(p * (dp * Z - delta))
    dv = (pt.transpose(-1, -2) @ do).bfloat16()
    dk = ((ds.transpose(-1, -2) @ q) * 0.125).bfloat16()
    dq = ((ds @ k) * 0.125).bfloat16()
    return dq, dk, dv


# ---- cases ----------------------------------------------------------------------------------------------------------
DROP = dict(p=0.1, seed=0x5EED1234ABCD, offset=3, site=5)
# causal S -> (B, H); (2, 4) and (1, 8) have B*H % 8 == 0 and take attn_block()'s XCD remap
CAUSAL = ((1, (1, 1)), (15, (3, 2)), (16, (2, 4)), (17, (1, 8)), (63, (1, 1)), (64, (3, 2)), (65, (2, 4)),
          (127, (1, 8)), (128, (3, 2)), (129, (1, 1)), (191, (3, 2)), (192, (1, 1)), (193, (2, 4)), (193, (1, 8)),
          (257, (1, 8)), (257, (2, 4)))
NONCAUSAL = (((1, 1), (1, 1)), ((1, 200), (3, 2)), ((200, 1), (2, 4)), ((64, 65), (1, 8)), ((65, 64), (1, 1)),
             ((128, 129), (3, 2)), ((129, 128), (2, 4)), ((17, 130), (1, 8)), ((130, 17), (1, 1)),
             ((257, 70), (2, 4)), ((257, 70), (1, 8)))
LENGTHS = tuple((S, S, True, bh) for S, bh in CAUSAL) + tuple((sq, sk, False, bh) for (sq, sk), bh in NONCAUSAL)
FAMILY_SHAPES = ((65, 65, True, (3, 2)), (129, 129, True, (2, 4)), (193, 193, True, (1, 8)),
                 (129, 128, False, (1, 1)), (257, 70, False, (2, 4)))
FAMILIES = ("peaked4", "peaked8", "late", "early", "flat", "routing")
DROP_SHAPES = ((128, 128, True, (3, 2)), (129, 129, True, (2, 4)), (65, 130, False, (1, 8)), (130, 65, False, (3, 2)),
               (1024, 1024, True, (1, 1)))
RING_SHAPES = ((257, 257, True, (1, 8)), (257, 70, False, (2, 4)))
# the nine cases of the float32 self-check: (Sq, Sk, causal, family, scale of q and k)
SELF_CHECK = ((65, 65, True, "benign", 1.0), (129, 200, False, "benign", 1.0), (192, 192, True, "benign", 1.0),
              (129, 129, True, "benign", 4.0), (100, 77, False, "benign", 6.0), (192, 192, True, "benign", 8.0),
              (64, 257, False, "benign", 10.0), (130, 130, True, "benign", 0.25), (70, 193, False, "late", 1.0))


def case_id(Sq, Sk, causal, bh, family="benign", scale=1.0, drop=False, salt=0):
    s = f"{Sq}c" if causal else f"{Sq}x{Sk}"
    return (f"{family}{'' if scale == 1.0 else f'x{scale:g}'}{'-drop' if drop else ''}-{s}-b{bh[0]}h{bh[1]}"
            f"{f'-draw{salt}' if salt else ''}")


@functools.lru_cache(maxsize=None)
def make_case(Sq, Sk, causal, bh, family="benign", scale=1.0, drop=False, salt=0):
    """One case on the CPU: bf16 q, k, v, do [B, H, S, 64] with independent data per (b, h), the visibility, Z.
    ``salt`` selects another draw of the same case."""
    B, H = bh
    name = case_id(Sq, Sk, causal, bh, family, scale, drop, salt)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    q = torch.randn(B, H, Sq, 64, generator=g)
    k = torch.randn(B, H, Sk, 64, generator=g)
    v = torch.randn(B, H, Sk, 64, generator=g)
    do = torch.randn(B, H, Sq, 64, generator=g)
    if family == "peaked4":
        q, k = 4.0 * q, 4.0 * k
    elif family == "peaked8":
        q, k = 8.0 * q, 8.0 * k
    elif family in ("late", "early"):  # one key (in the last tile / key 0) = 4 x the last query row, which sees it
        q = q.bfloat16().float()
        k[:, :, Sk - 1 if family == "late" else 0] = 4.0 * q[:, :, Sq - 1]
    elif family == "flat":
        q = torch.zeros_like(q)
    elif family == "routing":  # P one-hot in fp32: O[i] = V[pi(i)]
        k = 4.0 * (2.0 * torch.randint(0, 2, (B, H, Sk, 64), generator=g).float() - 1.0)
        if causal:
            pi = (torch.rand(B, H, Sq, generator=g) * (torch.arange(Sq) + 1)).long().clamp_max(Sq - 1)
            pi = torch.minimum(pi, torch.arange(Sq).expand(B, H, Sq))
        else:
            pi = torch.randint(0, Sk, (B, H, Sq), generator=g)
        q = torch.gather(k, 2, pi[..., None].expand(B, H, Sq, 64))
        # an asymmetric ramp of 127 levels (odd multiples of 1/16: exact in bf16, never 0, so that the e^-64 the other
        # keys weigh cannot show in a rounded output) that differs along keys, dims, heads and batches
        j, d = torch.arange(Sk)[:, None], torch.arange(64)[None, :]
        pair = torch.arange(B * H).view(B, H, 1, 1)
        v = (2 * ((7 * j + 3 * d + 11 * pair) % 127) - 125).float() / 16.0
    elif family != "benign":
        raise ValueError(family)
    q, k = scale * q, scale * k
    c = types.SimpleNamespace(name=name, salt=salt, B=B, H=H, Sq=Sq, Sk=Sk, causal=causal, family=family,
                              drop=DROP if drop else None,
                              q=q.bfloat16(), k=k.bfloat16(), v=v.bfloat16(), do=do.bfloat16(),
                              vis=visible(Sq, Sk, causal), keep=None, Z=None)
    if family == "routing":
        c.pi = pi
    if drop:
        keep = torch.from_numpy(X.keep_mask(DROP["seed"], DROP["offset"], DROP["site"], DROP["p"], B * H * Sq, Sk))
        c.keep = keep.view(B, H, Sq, Sk)
        c.Z = c.keep.double() / (1.0 - DROP["p"])
    return c


@functools.lru_cache(maxsize=None)
def case_fwd(Sq, Sk, causal, bh, family="benign", scale=1.0, drop=False, salt=0):
    """(case, fp64 forward reference, its bounds): computed once, shared, never modified."""
    c = make_case(Sq, Sk, causal, bh, family, scale, drop, salt)
    q, k, v = c.q.double(), c.k.double(), c.v.double()
    r = ref_fwd(q, k, v, c.vis, c.Z)
    return c, r, fwd_bounds(q, k, v, r)


def case_bwd(c, o_in, lse_in):
    """fp64 backward reference and bounds of case ``c`` for the given o_in (bf16) / lse_in (fp32), CPU tensors
    [B, H, Sq, 64] / [B, H, Sq]."""
    q, k, v, do = c.q.double(), c.k.double(), c.v.double(), c.do.double()
    o_in, lse_in = o_in.double(), lse_in.double()
    rb = ref_bwd(q, k, v, do, o_in, lse_in, c.vis, c.Z)
    return rb, bwd_bounds(q, k, v, do, o_in, lse_in, rb)


@functools.lru_cache(maxsize=None)
def case_bwd_ref_fed(Sq, Sk, causal, bh, family="benign", scale=1.0, drop=False, salt=0):
    """(o_in = bf16(ref O), lse_in = fp32(ref LSE), reference, bounds) of the backward fed the reference's outputs."""
    c, r, _ = case_fwd(Sq, Sk, causal, bh, family, scale, drop, salt)
    o_in, lse_in = r.O.bfloat16(), r.LSE.float()
    return (o_in, lse_in) + case_bwd(c, o_in, lse_in)
