"""ergm_linear_rows on the GPU against fp64 (cases, bound and gates: tests/_linear_rows.py, whose float32 self-check
runs without a GPU in tests/test_decode_exec_abi.py).

Per (K, N, layout): every M in {1, 15, 16, 17, 32, 33} (one row; either side of one MFMA fragment and of the 32-row
group), every epilogue (KN) or NONE and BIAS_RESID (NK), with and without the LayerNorm prologue, every leading
dimension wider than the logical width.  C is allocated with rows past M and columns past N filled with a sentinel and compared in full;
the allocation rows of A / x past M hold NaN, so a read of one would surface as a non-finite result."""
import pytest
import torch

import _linear_rows as R
from ergm_amd import _lib as L
from ergm_amd import ops

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev_case(gpu):
    """The device copies of a case's operands, made once per (K, N, layout)."""
    cache = {}

    def get(K, N, layout):
        key = (K, N, layout)
        if key not in cache:
            c = R.case(K, N, layout)
            Wa = torch.full((c["W_stored"].shape[0], c["W_stored"].shape[1] + 8), NAN, dtype=torch.bfloat16)
            Wa[:, :c["W_stored"].shape[1]] = c["W_stored"]                 # ldw wider than the logical width
            cache[key] = dict(c=c, W=Wa.to(gpu)[:, :c["W_stored"].shape[1]], gamma=c["gamma"].to(gpu),
                              beta=c["beta"].to(gpu), bias=c["bias"].to(gpu))
        return cache[key]
    return get


def _operand(c, ln, M, gpu, rows=None):
    """A (bf16, lda = K + 8) or x (f32, ldx = K + 4) with two allocation rows past M and the pad columns NaN."""
    src = (c["x"] if ln else c["A"])[:M] if rows is None else (c["x"] if ln else c["A"])[rows]
    a = torch.full((src.shape[0] + 2, c["K"] + (4 if ln else 8)), NAN, dtype=src.dtype)
    a[:src.shape[0], :c["K"]] = src
    return a.to(gpu)[:, :c["K"]]


def _run(d, ln, epi, M, gpu, in_place=True, A=None):
    """One call; returns the whole C allocation [M + 3, N + 8] (sentinel outside [:M, :N])."""
    c = d["c"]
    K, N = c["K"], c["N"]
    ob = c["refs"][(ln, epi)][2]
    Ca = torch.full((M + 3, N + 8), R.SENT, dtype=torch.bfloat16 if ob else torch.float32, device=gpu)
    aux = None
    if epi == "resid":
        if in_place:
            Ca[:M, :N] = c["resid"][:M].to(gpu)
            aux = Ca[:, :N]
        else:
            aux = torch.full((M + 1, N + 16), NAN, dtype=torch.float32, device=gpu)
            aux[:M, :N] = c["resid"][:M].to(gpu)
            aux = aux[:, :N]
    A = _operand(c, ln, M, gpu) if A is None else A
    ops.linear_rows(A, d["W"], M, N, K, c["layout"], out=Ca[:, :N], epilogue=R.EPILOGUES[epi],
                    bias=None if epi == "none" else d["bias"], aux=aux, ln_gamma=d["gamma"] if ln else None,
                    ln_beta=d["beta"] if ln else None, ln_eps=R.EPS)
    return Ca


def _contained(Ca, M, N):
    assert (Ca[M:] == R.SENT).all().item() and (Ca[:, N:] == R.SENT).all().item(), "a sentinel was overwritten"


@pytest.mark.parametrize("K,N,layout", R.SHAPES)
def test_every_m_epilogue_and_prologue_against_fp64(gpu, dev_case, K, N, layout):
    d = dev_case(K, N, layout)
    worst = {}
    for M in R.MS:
        for ln in (False, True):
            for epi in R.epilogues_of(layout):
                for in_place in ((True, False) if epi == "resid" else (True,)):
                    Ca = _run(d, ln, epi, M, gpu, in_place)
                    _contained(Ca, M, N)
                    what = f"K {K} N {N} M {M} ln {ln} {epi} in_place {in_place}"
                    ratio, rel = R.check(what, Ca[:M, :N], d["c"], ln, epi, M)
                    k = (ln, epi)
                    worst[k] = (max(worst.get(k, (0, 0))[0], ratio), max(worst.get(k, (0, 0))[1], rel))
    print(f"K {K} N {N}: worst err/bound, rel Frobenius:", {k: (round(v[0], 3), float("%.2g" % v[1])) for k, v in worst.items()})


@pytest.mark.parametrize("K,N,layout", R.SHAPES)
def test_same_bits_twice_and_row_alone(gpu, dev_case, K, N, layout):
    """The same call twice gives the same bits, and row r of an M = 32 call equals the M = 1 call on that row alone
    (r = 0, 15, 31; with and without the prologue; an f32 and, on KN, a bf16 epilogue)."""
    d = dev_case(K, N, layout)
    for ln in (False, True):
        for epi in (("none", "gelu") if layout == L.KN else ("none",)):
            full = _run(d, ln, epi, 32, gpu)
            again = _run(d, ln, epi, 32, gpu)
            assert torch.equal(full, again), (ln, epi)
            for r in (0, 15, 31):
                one = _run(d, ln, epi, 1, gpu, A=_operand(d["c"], ln, 1, gpu, rows=slice(r, r + 1)))
                _contained(one, 1, N)
                assert torch.equal(one[0, :N], full[r, :N]), (ln, epi, r)
