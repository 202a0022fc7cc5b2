"""Decode attention (ergm_attn_decode, ergm_amd/csrc/decode.hip) on the CPU: the cases of
tests/test_gpu_decode_attn_matrix.py with their host images, the fp64 reference of the operation include/ergm_hip.h
documents, the elementwise error bound of the bf16 output, and a plain restatement of the kernels' structure (chunks,
key slots, the slot merge, the split merge, the appended row) that runs in float32 (the emulation) or in float64 with
one deliberately WRONG operation switched on (the mutations).  Imports no GPU code; tests/test_decode_attn_bound.py
checks the bound from both sides without a GPU.

Reference (fp64 on the bf16-rounded inputs, per sequence b and head h).  n_b = clamp(lens[b], 0, max_len - append).
The keys are the cache rows t < n_b and, with ``append``, the row taken from qkv; S = q K^T / 8, P = softmax(S),
O = P V.  No key at all (n_b = 0, append = 0) gives zeros.  Sabs = |q||K|^T / 8 and T = P|V| are kept for the bound.
"""
import functools
import math
import types
import zlib

import numpy as np
import torch

U16, U32 = 2.0 ** -8, 2.0 ** -24
FLOOR = 2.0 ** -100
E_EXP = 4.0          # the relative error allowed to one expf, in units of u32: 2 ulp (the HIP math API documents 1)
SENT = 24576.0       # exact in bf16; read by mistake it wrecks the output, overwritten it shows
GUARD = 4096         # elements before and after each allocation the kernel is told about
SLOTS, MAX_SPLITS, PART = 32, 32, 66   # DEC_SLOTS, DEC_MAX_SPLITS, DEC_PART of decode.hip
OLD_GATE = 8e-3      # the whole-tensor relative Frobenius norm of tests/test_gpu_decode_ops.py
LAYOUTS = ("interleaved", "separate")


# ---- the split count ------------------------------------------------------------------------------------------------
def split_cap(max_len):
    return min(MAX_SPLITS, max(1, max_len // 256))


def auto_splits(B, H, max_len):
    """decode_auto_splits of decode.hip: what splits = 0 selects."""
    return min(split_cap(max_len), max(1, (256 + B * H - 1) // (B * H)))


def chunks(n, splits):
    """[k0, k1) of every split of a sequence of n rows: ceil(n / splits) rounded up to 32 rows each."""
    chunk = ((n + splits - 1) // splits + 31) & ~31
    k0 = [min(n, s * chunk) for s in range(splits)]
    return [(a, min(n, a + chunk)) for a in k0]


# ---- fp64 reference and bound of one sequence ------------------------------------------------------------------------
def ref_rows(q, K, V, scale=0.125):
    """q [H, 64], K, V [H, n, 64] fp64 (n may be 0): S, P, O, Sabs, T of the softmax attention of one query."""
    S = torch.einsum("hd,hnd->hn", q, K) * scale
    Sabs = torch.einsum("hd,hnd->hn", q.abs(), K.abs()) * 0.125
    P = torch.softmax(S, -1) if K.shape[1] else S
    return types.SimpleNamespace(S=S, P=P, Sabs=Sabs, O=torch.einsum("hn,hnd->hd", P, V),
                                 T=torch.einsum("hn,hnd->hd", P, V.abs()))


def bound_rows(r, V, n_cache):
    """The elementwise error bound [H, 64] of the bf16 output of one sequence, given its fp64 reference ``r``, the
    values V [H, n, 64] and the number of attended CACHE rows n_cache (the appended row not counted).

    Derivation, from the rounding points of attn_decode_kernel, attn_decode_merge_kernel and decode_finish as they
    stand (nothing is fitted to kernel output).  u16 = 2^-8, u32 = 2^-24 are the unit roundoffs of bf16 and fp32,
    |X| is elementwise; terms of second order in u32 are dropped, the closed forms expm1 and 1/(1 - x) are used where
    a first-order expansion would otherwise be needed.

    What the kernels compute is N / D with N = sum_t w_t v_t and D = sum_t w_t, where the effective weight w_t of key
    t is a product of expf values: p = expf(s_t - m) when the key enters its slot, one c = expf(m - mn) for every later
    row of the same slot, the slot's w = expf(sm_m[j] - M) in the LDS merge, the split's weight in the merge kernel and
    the append c of decode_finish.  N and D are fed the SAME computed factors, so a common factor (the maximum that is
    subtracted, and its error) cancels in N / D; what remains is a relative error E_t of each key's weight:
    * the score: an fp32 sum of 64 exact products of bf16 values (8 sequential additions per lane, then 3 shfl_xor
      levels; for the appended row the 6 levels of wave_sum), so every product passes through at most 10 additions:
      |ds_t| <= 10*u32*Sabs_t before and after the exact *0.125; 11*u32*Sabs_t here.  exp turns it into a relative
      error of the weight;
    * the arguments of the expf chain: each is a difference of two fp32 numbers, rounded once (u32*|argument|).  Every
      argument is <= 0 and they telescope to s_t - M, M the final maximum, so together they err by at most
      u32*(M - s_t), however long the chain is;
    * the roundings that every key passes whatever its score, with e = E_EXP the allowance of one expf in u32 and
      R = ceil(n_cache / 32) the most rows a slot can hold at any split count: entering the slot e + 2 (expf, p*v, the
      add), each later row of the slot e + 2 (c, acc*c, the add; c = 1 is exact and costs only the add), the slot merge
      e + 1 + 32 (w, the product, 32 additions), the split merge the same (at most 32 splits), the appended row's
      rescale e + 2, the division 1:  C = (e + 2)*(R + 1) + 2*(e + 33) + 1.  (An FMA contraction of l*c + p or
      acc*c + p*v removes one of these roundings; the count is an upper bound either way.)  This is the (n + c)*u32*T
      part; its n is n_cache/32, not n_cache, because a slot sums only its own rows.
      E_t = expm1(u32*(11*Sabs_t + (M - s_t) + C)).
    An addition rounds the partial sum, which is at most the sum of the |w_t v_t| so far, hence the error of N is taken
    against |V|:  |dN| / D <= (P*E)|V|,  |dD| / D <= sum_t P_t E_t =: eD, and
      |N^/D^ - O| <= ((P*E)|V| + |O|*eD) / (1 - eD) =: F.
    The final f2bf is RNE of the fp32 quotient: u16*(|O| + F).
      bound(O) = u16*|O| + (1 + u16)*F,  at least 2^-100
    (fp32 / bf16 subnormals and an expf that underflows are the only places where rounding is not relative; 2^-100 is
    far above what they contribute and far below anything a wrong element produces).  P is never rounded to bf16 in
    these kernels, so no u16*T term appears: for an output that is not a sum of cancelling terms the bound is the
    final bf16 rounding plus about 1e-5 of T."""
    if V.shape[1] == 0:
        return torch.full_like(r.O, FLOOR)
    R = (n_cache + SLOTS - 1) // SLOTS
    C = (E_EXP + 2.0) * (R + 1) + 2.0 * (E_EXP + 33.0) + 1.0
    d = r.S.max(-1, keepdim=True).values - r.S
    PE = r.P * torch.expm1(U32 * (11.0 * r.Sabs + d + C))
    eD = PE.sum(-1, keepdim=True)
    F = (torch.einsum("hn,hnd->hd", PE, V.abs()) + r.O.abs() * eD) / (1.0 - eD)
    return (U16 * r.O.abs() + (1.0 + U16) * F).clamp_min(FLOOR)


def ratio(got, ref, b):
    """Largest err/bound; a NaN anywhere in ``got`` counts as infinite."""
    got = got.double()
    if torch.isnan(got).any().item():
        return math.inf
    return ((got - ref).abs() / b).max().item() if got.numel() else 0.0


def old_gate_rel(got, ref):
    """The relative Frobenius norm over the whole [B, E] output that test_attn_decode_ragged gates at OLD_GATE."""
    got = got.double()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


# ---- cases ----------------------------------------------------------------------------------------------------------
A_LENS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319)
GROUPS = {  # name -> max_len, H, lens with append, lens without, splits of the benign family
    "A": (320, 2, A_LENS, A_LENS + (320,), (1, 2, 3, 5, 32, 0)),
    "B": (1100, 2, (1024, 1025, 1099, 513, 33, 0), None, (0, 4, 7, 32)),
    "C": (8192, 1, (8191, 4097), None, (0, 32, 1)),
    "D16": (512, 16, (0, 1, 7, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 9, 32), None, (0,)),
    "D8": (512, 16, (0, 1, 31, 64, 129, 256, 319, 8), None, (0,)),
}
FAMILIES = ("peaked", "flat", "late-max", "append-max", "early-max", "lonely-split", "const-keys", "cancel")
FAMILY_GROUPS = ("A", "B")
FAMILY_SPLITS = (1, 3, 32)
# every case of the GPU matrix: (group, family, append)
CASES = tuple((g, "benign", a) for g in GROUPS for a in (0, 1)) + tuple(
    (g, f, a) for g in FAMILY_GROUPS for f in FAMILIES for a in (0, 1) if a or f != "append-max")


def case_id(group, family, append):
    return f"{group}-{family}-{'append' if append else 'read'}"


def case_splits(group, family):
    return GROUPS[group][4] if family == "benign" else FAMILY_SPLITS


def group_case(group, family="benign", append=0):
    """(case, reference, bound) of a case of the matrix: computed once, shared, never modified."""
    max_len, H, lens1, lens0, _ = GROUPS[group]
    return make_case(max_len, H, lens1 if append or lens0 is None else lens0, family, append, 0, group)


def _dominate(q, keys, row, margin, over_max):
    """Make keys[row] = alpha*q with alpha chosen so that its score stands ``margin`` nats above the logsumexp
    (``over_max``: above the maximum) of the other keys' scores.  q [64], keys [n, 64], bf16-valued float64."""
    s = keys @ q / 8.0
    s[row] = -math.inf
    if keys.shape[0] == 1:
        base = 0.0
    else:
        base = max(0.0, (s.max() if over_max else torch.logsumexp(s, 0)).item())
    keys[row] = (8.0 * (base + margin) / (q @ q).item()) * q


@functools.lru_cache(maxsize=None)
def make_case(max_len, H, lens, family="benign", append=0, salt=0, group="x"):
    """One launch on the CPU: B = len(lens) sequences, independent data per (b, h).  Returns a namespace with the
    pristine caches K, V [B, max_len, E] (bf16, SENT in every row >= n_b), qkv [B, 3E] (bf16), lens, n (clamped), the
    fp64 reference O [B, E] and its bound, and per sequence the reference's P, Sabs, T ([H, keys] / [H, 64]).

    Families (what each stresses):
      benign        randn baseline
      peaked, flat  q, k x10 / x0.25: rescale factors far from 1 / near 1
      late-max      the last cache row holds e^3 times the weight of all other keys: the rescale after many rows
      append-max    the same for the appended row (append = 1): the append c of decode_finish
      early-max     the same for row 0: the weights of the later slots and splits
      lonely-split  the last cache row stands >= 20 nats above every other key: its chunk is the last non-empty one at
                    every split count (at n = 1 mod the chunk it is alone there) and every other split's weight is
                    <= e^-20: the split weights
      const-keys    all keys equal, O = mean V: the accumulation of l over n terms
      cancel        V alternating in sign along the rows over a flat softmax, |O| << T: the absolute term"""
    B, E = len(lens), 64 * H
    n = [max(0, min(x, max_len - append)) for x in lens]
    name = f"{group}-{family}-{max_len}x{H}-{','.join(map(str, lens))}-a{append}-s{salt}"
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    bf = lambda x: x.bfloat16().double()
    K = torch.full((B, max_len, H, 64), SENT, dtype=torch.float64)
    V = torch.full((B, max_len, H, 64), SENT, dtype=torch.float64)
    qkv = torch.empty(B, 3, H, 64, dtype=torch.float64)
    scale = {"peaked": 10.0, "flat": 0.25, "cancel": 0.25}.get(family, 1.0)
    for b in range(B):
        nb = n[b]
        q = bf(scale * torch.randn(H, 64, generator=g))
        k = scale * torch.randn(nb + 1, H, 64, generator=g).double()   # row nb: the appended key
        v = torch.randn(nb + 1, H, 64, generator=g).double()
        if family == "const-keys":
            k[:] = k[:1].clone()
        elif family == "cancel":
            sign = 1.0 - 2.0 * (torch.arange(nb + 1) % 2).double()
            v = sign[:, None, None] * (1.0 + v[:1].abs())
        elif family in ("late-max", "append-max", "early-max", "lonely-split"):
            row = {"late-max": nb - 1, "lonely-split": nb - 1, "append-max": nb, "early-max": 0}[family]
            keys = nb + 1 if append else nb
            if 0 <= row < keys:
                for h in range(H):
                    kh = bf(k[:keys, h])
                    if family == "lonely-split":
                        _dominate(q[h], kh, row, 24.0, True)
                    else:
                        _dominate(q[h], kh, row, 3.0, False)
                    k[:keys, h] = kh
        elif family not in ("benign", "peaked", "flat"):
            raise ValueError(family)
        K[b, :nb], V[b, :nb] = bf(k[:nb]), bf(v[:nb])
        qkv[b, 0], qkv[b, 1], qkv[b, 2] = q, bf(k[nb]), bf(v[nb])
    c = types.SimpleNamespace(name=name, group=group, family=family, append=append, salt=salt, B=B, H=H, E=E,
                              max_len=max_len, lens=tuple(lens), n=tuple(n),
                              K=K.view(B, max_len, E).bfloat16(), V=V.view(B, max_len, E).bfloat16(),
                              qkv=qkv.view(B, 3 * E).bfloat16(), P=[], Sabs=[], T=[], S=[])
    O, bound = [], []
    for b in range(B):
        nb = n[b]
        kk, vv = K[b, :nb], V[b, :nb]
        if append:
            kk, vv = torch.cat([kk, qkv[b, 1][None]]), torch.cat([vv, qkv[b, 2][None]])
        kk, vv = kk.permute(1, 0, 2), vv.permute(1, 0, 2)
        r = ref_rows(qkv[b, 0], kk, vv)
        if family == "lonely-split" and kk.shape[1] > 1 and nb:   # a condition of the family, not of the kernel
            others = torch.cat([r.S[:, :nb - 1], r.S[:, nb:]], 1)
            assert (r.S[:, nb - 1] - others.max(-1).values).min().item() >= 20.0, name
        O.append(r.O.reshape(E))
        bound.append(bound_rows(r, vv, nb).reshape(E))
        for lst, x in ((c.P, r.P), (c.Sabs, r.Sabs), (c.T, r.T), (c.S, r.S)):
            lst.append(x)
    c.O, c.bound = torch.stack(O), torch.stack(bound)
    return c


# ---- host images ----------------------------------------------------------------------------------------------------
def image(c, layout):
    """The host image of case ``c`` as tests/test_gpu_decode_ops.py::_make builds it: for every allocation
    guard | B sequences of ld_seq | guard, SENT everywhere except the first n_b rows of each sequence's columns [0, E).
      interleaved   one buffer, K | V of a position in one row: ld_row = 2E, V at element offset E
      separate      one buffer each for K and V with ld_row = E + 8 (8 padding columns holding SENT)
    In both, a gap of 64 elements follows every sequence, qkv has rows of 3E + 8 and out rows of E + 8 elements, the
    padding holding SENT.  Returns bufs (bf16, flat), want (the same after the call: with ``append`` row n_b holds the
    K | V of the qkv row, bitwise, and nothing else moves), where K and V start (buffer index, element offset), the
    strides, and the padded qkv."""
    B, E, L = c.B, c.E, c.max_len
    if layout == "interleaved":
        ld_row = 2 * E
        ld_seq = L * ld_row + 64
        bufs = [torch.full((GUARD + B * ld_seq + GUARD,), SENT, dtype=torch.bfloat16)]
        at = {"k": (0, GUARD), "v": (0, GUARD + E)}
    elif layout == "separate":
        ld_row = E + 8
        ld_seq = L * ld_row + 64
        bufs = [torch.full((GUARD + B * ld_seq + GUARD,), SENT, dtype=torch.bfloat16) for _ in range(2)]
        at = {"k": (0, GUARD), "v": (1, GUARD)}
    else:
        raise ValueError(layout)

    def rows(bs, which):
        i, off = at[which]
        return bs[i].as_strided((B, L, E), (ld_seq, ld_row, 1), off)

    rows(bufs, "k").copy_(c.K)
    rows(bufs, "v").copy_(c.V)
    want = [b.clone() for b in bufs]
    if c.append:
        for b, nb in enumerate(c.n):
            rows(want, "k")[b, nb] = c.qkv[b, E:2 * E]
            rows(want, "v")[b, nb] = c.qkv[b, 2 * E:]
    qkv = torch.full((B, 3 * E + 8), SENT, dtype=torch.bfloat16)
    qkv[:, :3 * E] = c.qkv
    return types.SimpleNamespace(bufs=bufs, want=want, at=at, ld_seq=ld_seq, ld_row=ld_row, qkv=qkv, ldo=E + 8)


# ---- the kernels' structure, in float32 (the emulation) or float64 (the mutations) ---------------------------------
WRONG = ("chunk-end", "row128", "slot31", "split-w1", "no-append", "stale-k", "scale2", "empty-w1", "empty-stale")
_XOR = [np.arange(8) ^ x for x in (1, 2, 4)]


def _neginf(x):
    return np.isneginf(x)


def emu_decode(c, splits, dtype=np.float32, wrong=None):
    """The structure of attn_decode_kernel + attn_decode_merge_kernel + decode_finish, not only their formula: chunks of
    ceil(n / splits) rounded up to 32 rows; row t of a chunk goes to slot (t - k0) mod 32 in row order, each slot with
    its own online softmax (m, l, acc); the 32 slots merged in slot order, the splits in split order, then the appended
    row from the qkv row.  The score is summed as the lanes do (8 sequential, 3 xor levels; the appended row's by the
    adjacent-pair tree of wave_sum).  dtype float32: the emulation, returns bf16 [B, E].  dtype float64: the same
    structure without rounding, returns float64 [B, E]; with ``wrong`` = None that is the reference itself.

    ``wrong`` switches one WRONG operation on (tests/test_decode_attn_bound.py):
      chunk-end    the loop's guard reads t < k1 - 1 in every chunk but the last non-empty one: its last row is lost
      row128       row k0 + 128 of every chunk, the first row of the second loop iteration, is lost
      slot31       slot 31 is left out of the LDS merge
      split-w1     a non-empty split that does not hold the maximum is merged with weight 1, not exp(m_s - M)
      no-append    the appended row is stored but not attended
      stale-k      the appended row's score is taken from the cache's row n_b as it was before the call
      scale2       the scale 1/8 is applied twice
      empty-w1     an empty split's partial (m = -inf) is merged with weight 1, not 0
      empty-stale  an empty split writes no partial; the merge reads split 0's in its place"""
    assert wrong is None or wrong in WRONG, wrong
    S = splits or auto_splits(c.B, c.H, c.max_len)
    B, H, L, E, f = c.B, c.H, c.max_len, c.E, dtype
    Kf = c.K.float().numpy().reshape(B, L, H, 64).astype(f)
    Vf = c.V.float().numpy().reshape(B, L, H, 64).astype(f)
    qkv = c.qkv.float().numpy().reshape(B, 3, H, 64).astype(f)
    q = qkv[:, 0]
    n = np.array(c.n, dtype=np.int64)
    chunk = ((n + S - 1) // S + 31) & ~31
    k0 = np.minimum(n[:, None], np.arange(S)[None] * chunk[:, None])          # [B, S]
    k1 = np.minimum(n[:, None], k0 + chunk[:, None])
    k1v = k1
    if wrong == "chunk-end":
        last = (k1 > k0).sum(1) - 1
        k1v = np.where(np.arange(S)[None] < last[:, None], k1 - 1, k1)
    eighth = f(0.125)
    m = np.full((B, S, SLOTS, H), -np.inf, dtype=f)
    l = np.zeros((B, S, SLOTS, H), dtype=f)
    acc = np.zeros((B, S, SLOTS, H, 64), dtype=f)
    bidx = np.arange(B)[:, None, None]
    with np.errstate(all="ignore"):
        for j in range(int(chunk.max()) // SLOTS):
            t = k0[:, :, None] + SLOTS * j + np.arange(SLOTS)[None, None]         # [B, S, 32]
            ok = t < k1v[:, :, None]
            if wrong == "row128" and SLOTS * j == 128:
                ok = ok & (np.arange(SLOTS)[None, None] != 0)
            if not ok.any():
                continue
            tc = np.minimum(t, L - 1)
            kf, vf = Kf[bidx, tc], Vf[bidx, tc]                                   # [B, S, 32, H, 64]
            p8 = (q[:, None, None] * kf).reshape(B, S, SLOTS, H, 8, 8)
            s = p8[..., 0]
            for i in range(1, 8):
                s = s + p8[..., i]
            for x in _XOR:
                s = s + s[..., x]
            s = s[..., 0] * eighth
            if wrong == "scale2":
                s = s * eighth
            ok = ok[..., None]
            mn = np.maximum(m, s)
            cc = np.where(_neginf(m), f(0), np.exp(m - mn))
            p = np.exp(s - mn)
            l = np.where(ok, l * cc + p, l)
            acc = np.where(ok[..., None], acc * cc[..., None] + p[..., None] * vf, acc)
            m = np.where(ok, mn, m)
        # the LDS merge, slot order
        M = m.max(axis=2)                                                         # [B, S, H]
        Ls = np.zeros((B, S, H), dtype=f)
        Os = np.zeros((B, S, H, 64), dtype=f)
        for j in range(SLOTS):
            if wrong == "slot31" and j == 31:
                continue
            w = np.where(_neginf(m[:, :, j]), f(0), np.exp(m[:, :, j] - M))
            Ls = Ls + l[:, :, j] * w
            Os = Os + acc[:, :, j] * w[..., None]
        if wrong == "empty-stale":
            empty = _neginf(M)
            M = np.where(empty, M[:, :1], M)
            Ls = np.where(empty, Ls[:, :1], Ls)
            Os = np.where(empty[..., None], Os[:, :1], Os)
        # the split merge, split order (splits = 1: one partial of weight expf(0) = 1, the same bits)
        Mg = M.max(axis=1)                                                        # [B, H]
        w = np.where(_neginf(M), f(0), np.exp(M - Mg[:, None]))
        if wrong == "split-w1":
            w = np.where(~_neginf(M) & (M < Mg[:, None]), f(1), w)
        if wrong == "empty-w1":
            w = np.where(_neginf(M), f(1), w)
        Lg = np.zeros((B, H), dtype=f)
        Og = np.zeros((B, H, 64), dtype=f)
        for s_ in range(S):
            Lg = Lg + Ls[:, s_] * w[:, s_]
            Og = Og + Os[:, s_] * w[:, s_, :, None]
        if c.append and wrong != "no-append":
            kn, vn = qkv[:, 1], qkv[:, 2]
            if wrong == "stale-k":
                kn = Kf[np.arange(B), n]
            x = q * kn
            while x.shape[-1] > 1:
                x = x[..., 0::2] + x[..., 1::2]
            s = x[..., 0] * eighth
            if wrong == "scale2":
                s = s * eighth
            Mn = np.maximum(Mg, s)
            cc = np.where(_neginf(Mg), f(0), np.exp(Mg - Mn))
            p = np.exp(s - Mn)
            Lg = Lg * cc + p
            Og = Og * cc[..., None] + p[..., None] * vn
        out = np.where(Lg[..., None] > 0, Og / Lg[..., None], f(0)).reshape(B, E)
    out = torch.from_numpy(np.ascontiguousarray(out))
    return out.bfloat16() if f is np.float32 else out


# ---- checking a result ----------------------------------------------------------------------------------------------
WORST = {}  # (family, group) -> largest err/bound seen


def check(c, what, got):
    """``got`` [B, E] against the fp64 reference of case ``c``: no NaN, every element within the bound; on failure the
    sequence, head, dim, n and err/bound of the worst element.  Returns, and records under (family, group), the worst
    err/bound."""
    got = got.detach().double().cpu()
    assert got.shape == c.O.shape, (what, got.shape, c.O.shape)
    assert not torch.isnan(got).any().item(), f"{what}: NaN in the result"
    rat = (got - c.O).abs() / c.bound
    worst = rat.max().item()
    key = (c.family, c.group)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if worst > 1.0:
        b, e = divmod(int(rat.argmax()), c.E)
        raise AssertionError(f"{what}: {int((rat > 1.0).sum())} of {rat.numel()} elements past the bound, worst "
                             f"err/bound {worst:.3g} at sequence {b} (n = {c.n[b]}), head {e // 64}, dim {e % 64}: got "
                             f"{got[b, e].item()!r} want {c.O[b, e].item()!r} bound {c.bound[b, e].item():.3g}")
    return worst


def report():
    for fam, grp in sorted(WORST):
        print(f"{fam:<13s} {grp:<4s} worst err/bound {WORST[(fam, grp)]:.4f}")
