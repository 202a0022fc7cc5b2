"""The batched-generation kernels (ergm_amd/csrc/decode.hip) on the GPU: ragged decode attention against fp64 and
against ergm_attn_fwd with Sq = 1, with sentinels around and inside the cache; ergm_embed_rows bitwise against
ergm_embed_fwd; ergm_topp_sample against the fp64 restatement of its rule (tests/_topp.py)."""
import numpy as np
import pytest
import torch

import _topp
from ergm_amd import ops

pytestmark = pytest.mark.gpu

H, E, B = 2, 128, 3
MAXLEN = 130
LD_ROW = 2 * E                      # K | V interleaved in one [max_len][2E] buffer
LD_SEQ = MAXLEN * LD_ROW + 64       # a gap after every sequence
GUARD = 4096                        # elements before and after the allocation the kernel is told about
SENT = 24576.0                      # exact in bf16; read by mistake it wrecks the output, overwritten it shows
ATTN_REL = 8e-3                     # the ergm_attn_fwd output gate, tests/test_gpu_ops.py:196


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _bits(t):
    return t.cpu().view(torch.int16)


def _make(lens_filled, seed, fill_all=False):
    """Host image: guard | B sequences of LD_SEQ | guard, sentinel everywhere except the first lens_filled[b] rows."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((GUARD + B * LD_SEQ + GUARD,), SENT, dtype=torch.bfloat16)
    rows = buf[GUARD:GUARD + B * LD_SEQ].view(B, LD_SEQ)[:, :MAXLEN * LD_ROW].view(B, MAXLEN, LD_ROW)
    for b, n in enumerate(lens_filled):
        n = MAXLEN if fill_all else n
        rows[b, :n] = torch.randn(n, LD_ROW, generator=g).bfloat16()
    qkv = torch.randn(B, 3 * E, generator=g).bfloat16()
    return buf, rows, qkv


def _views(buf_d):
    kc = buf_d.as_strided((B, MAXLEN, E), (LD_SEQ, LD_ROW, 1), GUARD)
    vc = buf_d.as_strided((B, MAXLEN, E), (LD_SEQ, LD_ROW, 1), GUARD + E)
    return kc, vc


def _ref64(rows, qkv, lens, append):
    """fp64 softmax attention over the same bf16-rounded inputs; [B, E]."""
    out = torch.zeros(B, E, dtype=torch.float64)
    for b, n in enumerate(lens):
        for h in range(H):
            c = slice(64 * h, 64 * h + 64)
            k, v = rows[b, :n, :E][:, c].double(), rows[b, :n, E:][:, c].double()
            if append:
                k = torch.cat([k, qkv[b, E:2 * E][c].double()[None]])
                v = torch.cat([v, qkv[b, 2 * E:][c].double()[None]])
            if k.shape[0]:
                out[b, c] = torch.softmax(k @ qkv[b, :E][c].double() / 8.0, 0) @ v
    return out


def _run(gpu, buf, qkv, lens, append, splits):
    buf_d, qkv_d = buf.to(gpu), qkv.to(gpu)
    kc, vc = _views(buf_d)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=gpu)
    out = ops.attn_decode(qkv_d if append else qkv_d[:, :E], kc, vc, lens_d, append, splits=splits)
    torch.cuda.synchronize()
    assert lens_d.cpu().tolist() == list(lens)   # never modified
    return out, buf_d


@pytest.mark.parametrize("append", [0, 1])
@pytest.mark.parametrize("lens", [(0, 1, 63), (64, 65, 100), (MAXLEN - 1, 7, 33)])
def test_attn_decode_ragged(gpu, lens, append):
    """Three lengths per call; 100 straddles the 64-row boundary of splits = 3 (chunks of ceil(100/3) -> 64 rows,
    the third empty); MAXLEN - 1 with append is the last legal slot."""
    buf, rows, qkv = _make(lens, seed=sum(lens) + append)
    ref = _ref64(rows, qkv, lens, append)
    want = buf.clone()
    if append:  # row lens[b] <- the K | V of the qkv row, bitwise; nothing else moves
        w = want[GUARD:GUARD + B * LD_SEQ].view(B, LD_SEQ)[:, :MAXLEN * LD_ROW].view(B, MAXLEN, LD_ROW)
        for b, n in enumerate(lens):
            w[b, n] = qkv[b, E:]
    outs = {}
    for splits in (1, 3, 0):
        out, buf_d = _run(gpu, buf, qkv, lens, append, splits)
        out2, _ = _run(gpu, buf, qkv, lens, append, splits)
        assert torch.equal(_bits(out), _bits(out2)), splits            # the same bits on every run
        assert torch.equal(_bits(buf_d), _bits(want)), splits          # sentinels, appended row, every other row
        err = _rel(out.cpu(), ref)
        print(f"attn_decode lens {lens} append {append} splits {splits}: rel {err:.2e}")
        assert err < ATTN_REL, splits
        outs[splits] = out
        for b, n in enumerate(lens):
            if n == 0:   # append = 0: a zero row; append = 1: attention over the new row alone = the new V
                exp = qkv[b, 2 * E:] if append else torch.zeros(E, dtype=torch.bfloat16)
                assert torch.equal(_bits(out[b]), _bits(exp)), (splits, b)
    assert _rel(outs[3], outs[1]) < ATTN_REL and _rel(outs[0], outs[1]) < ATTN_REL
    # the training kernel doing the same job, one sequence at a time (Sq = 1 over the first n rows)
    kc, vc = _views(buf_d)
    qkv_d = qkv.to(gpu)
    got, fwd = [], []
    for b, n in enumerate(lens):
        n += append
        if n:
            o, _ = ops.attn_fwd(qkv_d[b:b + 1, :E], kc[b, :n], vc[b, :n], 1, H, 1, n, False)
            fwd.append(o[0])
            got.append(outs[1][b])
    assert _rel(torch.stack(got), torch.stack(fwd)) < ATTN_REL


@pytest.mark.parametrize("append", [0, 1])
def test_attn_decode_clamps_wild_lengths(gpu, append):
    """lens past max_len and negative: clamped to [0, max_len - append], ERGM_OK, nothing outside the cache written.
    Every row of the cache holds data here and the guard regions are part of the test's own allocation, so the
    clamped call only ever touches valid memory."""
    lens = (MAXLEN + 1000, -5, 2 ** 31 - 1)
    eff = [MAXLEN - append, 0, MAXLEN - append]
    buf, rows, qkv = _make(lens, seed=5, fill_all=True)
    want = buf.clone()
    if append:
        w = want[GUARD:GUARD + B * LD_SEQ].view(B, LD_SEQ)[:, :MAXLEN * LD_ROW].view(B, MAXLEN, LD_ROW)
        for b, n in enumerate(eff):
            w[b, n] = qkv[b, E:]
    for splits in (1, 2):
        out, buf_d = _run(gpu, buf, qkv, lens, append, splits)   # raises unless ERGM_OK
        assert torch.equal(_bits(buf_d), _bits(want)), splits
        assert _rel(out.cpu(), _ref64(rows, qkv, eff, append)) < ATTN_REL


def test_embed_rows_matches_embed_fwd_bitwise(gpu):
    V, P = 500, 64
    g = torch.Generator().manual_seed(3)
    wte, wpe = torch.randn(V, E, generator=g).to(gpu), torch.randn(P, E, generator=g).to(gpu)
    ids, tt, pos = torch.tensor([17, 499, 0]), torch.tensor([498, 497, 499]), [0, 1, P - 1]
    full_ids, full_tt = torch.randint(0, V, (B, P), generator=g), torch.randint(0, V, (B, P), generator=g)
    for b in range(B):
        full_ids[b, pos[b]], full_tt[b, pos[b]] = ids[b], tt[b]
    pos_d = torch.tensor(pos, dtype=torch.int32, device=gpu)
    for types in (tt, None):
        h0, _ = ops.embed_fwd(full_ids.to(gpu), None if types is None else full_tt.to(gpu), full_ids.to(gpu), wte, wpe)
        rows = ops.embed_rows(ids.to(gpu), None if types is None else types.to(gpu), pos_d, wte, wpe)
        want = torch.stack([h0.view(B, P, E)[b, pos[b]] for b in range(B)])
        assert torch.equal(rows.view(torch.int32), want.view(torch.int32))
    # indices outside their tables are clamped (ids, positions) or add nothing (types): never followed
    wild = ops.embed_rows(torch.tensor([-7, 10 ** 6, 3]).to(gpu), torch.tensor([-1, V, 5]).to(gpu),
                          torch.tensor([1000, -3, 2], dtype=torch.int32, device=gpu), wte, wpe)
    want = torch.stack([wte[0] + wpe[P - 1], wte[V - 1] + wpe[0], (wte[3] + wpe[2]) + wte[5]])
    assert torch.equal(wild, want)


# ---- nucleus sampling -------------------------------------------------------------------------------
EOS = 7
TOP_P = 0.6
# head probabilities {token: p} of each row; the tail shares the rest evenly.  With top_p = 0.6 the cut of every
# row lies >= 0.05 inside an interval >= 0.15 wide (asserted below, from the fp64 ranking).
ROWS = [
    {311: 0.30, 12: 0.20, 140: 0.15, 77: 0.10, 499: 0.05},   # 0.6 in (0.50, 0.65]: 3 kept
    {205: 0.80},                                             # one-token nucleus: the first p is above top_p
    {300: 0.20, 100: 0.20, 40: 0.50},                        # two tied tokens straddle the cut: 100 kept, 300 not
    {EOS: 0.90, 33: 0.05},                                   # must draw EOS: the flag is set
    {1: 0.40, 2: 0.30},                                      # finished before the call: emits EOS, draws nothing
]
WANT_KEPT = [3, 1, 2, 1, 0]
# seeds chosen on the CPU (tests/_topp.py) so that for every live row u·mass lies >= 1e-4·mass from every boundary
# of the kept tokens' CDF, at top_p = 0.6 and at top_p = 1.0: {V: seed}
SEEDS = {500: 1, 5000: 1, 50257: 1}
CHI2_SEED = 5   # the helper's own 4,096 draws with this seed give chi-square 6.31


def _logits(V, rows=ROWS):
    out = np.empty((len(rows), V), dtype=np.float32)
    for r, head in enumerate(rows):
        p = np.full(V, (1.0 - sum(head.values())) / (V - len(head)))
        for t, v in head.items():
            p[t] = v
        out[r] = np.log(p)
    return out


def _sample(gpu, logits, V, top_p, seed, step=0, finished=None):
    lg = torch.from_numpy(logits).to(gpu)
    n = lg.shape[0]
    fin = None if finished is None else torch.tensor(finished, dtype=torch.uint8, device=gpu)
    kept = torch.full((n,), -1, dtype=torch.int32, device=gpu)
    mass = torch.full((n,), -1.0, dtype=torch.float32, device=gpu)
    tok = ops.topp_sample(lg, V, top_p, seed, step, EOS, finished=fin, kept=kept, kept_mass=mass)
    torch.cuda.synchronize()
    return tok.cpu().tolist(), kept.cpu().tolist(), mass.cpu().tolist(), None if fin is None else fin.cpu().tolist()


@pytest.mark.parametrize("V", [500, 5000, 50257])
def test_topp_sample_known_cuts(gpu, V):
    logits = _logits(V)
    seed = SEEDS[V]
    fin0 = [0, 0, 0, 0, 1]
    for top_p in (TOP_P, 1.0):
        want_tok, want_kept = [], []
        for r in range(4):
            if top_p < 1.0:   # the margin the exact kept count rests on: fp32 sums over V terms err by <= V·2^-24 = 3e-3
                lo, hi = _topp.cut_margin(logits[r], top_p)
                assert lo >= 0.008 and hi >= 0.008 and lo + hi >= 0.02, (r, lo, hi)
            tok, gap, kept, _ = _topp.draw(logits[r], top_p, _topp.uniform(seed, r, 0))
            assert gap >= 1e-4, (r, gap)   # a condition of the test: every row qualifies, none is left out
            want_tok.append(tok)
            want_kept.append(kept.size)
        assert want_kept == (WANT_KEPT[:4] if top_p < 1.0 else [V] * 4)
        tok, kept, mass, fin = _sample(gpu, logits, V, top_p, seed, finished=fin0)
        print(f"V {V} top_p {top_p}: tokens {tok} kept {kept} mass {mass}")
        assert kept == want_kept + [0]
        assert tok == want_tok + [EOS]
        assert fin == [int(t == EOS) for t in want_tok] + [1]
        if top_p < 1.0:
            assert want_tok[3] == EOS and tok[2] in (40, 100)
            for r in range(4):
                k, p = _topp.kept_set(logits[r], top_p)
                assert abs(mass[r] - p[k].sum()) < 1e-4
        # a finished row is indifferent to the seed; a live row is not bound to one token
        tok2, kept2, _, fin2 = _sample(gpu, logits, V, top_p, seed + 1, finished=fin0)
        assert tok2[4] == EOS and kept2[4] == 0 and fin2[4] == 1
        # without the optional arguments
        lg = torch.from_numpy(logits).to(gpu)
        assert ops.topp_sample(lg, V, top_p, seed, 0, EOS).cpu().tolist()[:4] == want_tok


def test_topp_sample_flat_row(gpu):
    """Random logits (std 1) over 50,257 tokens: no margin exists, so the kept count is only bracketed by the
    fp64 counts at top_p -+ delta, delta = V·2^-24 (the worst-case fp32 summation error)."""
    V, top_p = 50257, 0.9
    delta = V * 2.0 ** -24
    logits = np.random.default_rng(8).normal(size=(2, V)).astype(np.float32)
    a = _sample(gpu, logits, V, top_p, 11)
    b = _sample(gpu, logits, V, top_p, 11)
    assert a == b
    for r in range(2):
        lo, _ = _topp.kept_set(logits[r], top_p - delta)
        hi, _ = _topp.kept_set(logits[r], top_p + delta)
        exact, _ = _topp.kept_set(logits[r], top_p)
        print(f"flat row {r}: kept {a[1][r]} (fp64 {exact.size}, bracket {lo.size}..{hi.size}), token {a[0][r]}")
        assert lo.size <= a[1][r] <= hi.size
        assert a[0][r] in set(hi.tolist())


def test_topp_sample_distribution(gpu):
    """4,096 draws (step = 0 .. 4095) of a row whose nucleus is 8 tokens: chi-square against the renormalised
    nucleus probabilities below the 99.9 % quantile of 7 degrees of freedom (24.32).  The seed is fixed."""
    V, top_p, n = 500, 0.9, 4096
    head = {9: 0.25, 450: 0.20, 3: 0.15, 120: 0.10, 77: 0.08, 301: 0.06, 18: 0.04, 200: 0.04}   # 0.9 in (0.88, 0.92]
    logits = _logits(V, [head])
    lo, hi = _topp.cut_margin(logits[0], top_p)
    assert lo >= 0.008 and hi >= 0.008 and lo + hi >= 0.02
    kept, p = _topp.kept_set(logits[0], top_p)
    assert kept.tolist() == sorted(head)
    expect = n * p[kept] / p[kept].sum()
    lg = torch.from_numpy(logits).to(gpu)
    out = torch.empty(n, dtype=torch.int64, device=gpu)
    for step in range(n):
        ops.topp_sample(lg, V, top_p, CHI2_SEED, step, EOS, tokens=out[step:step + 1])
    toks = out.cpu().numpy()
    assert np.isin(toks, kept).all()
    counts = np.array([(toks == t).sum() for t in kept])
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    cpu = np.array([_topp.draw(logits[0], top_p, _topp.uniform(CHI2_SEED, 0, s))[0] for s in range(0, n, 64)])
    print(f"chi-square {chi2:.2f} over {n} draws; counts {counts.tolist()}")
    assert (toks[::64] == cpu).mean() > 0.9   # the same Philox stream as the helper
    assert chi2 < 24.322
