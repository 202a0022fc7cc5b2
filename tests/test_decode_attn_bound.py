"""The decode-attention bound of tests/_decode_attn.py, checked without a GPU from both sides: (a) a float32 evaluation
with the kernels' structure (chunks, key slots, slot merge, split merge, appended row) fits it on every case and split
count that tests/test_gpu_decode_attn_matrix.py runs, with no factor on the bound, and (b) the fp64 result of a
slightly WRONG operation breaches it in at least one element.  The same wrong results are also put through the older
whole-tensor norm gate (8e-3, tests/test_gpu_decode_ops.py), and which of them it lets through is printed: that is
the reason for the elementwise gate.  Neither side is tuned to the other.

One listed mutation cannot be seen by any gate, and the test asserts exactly that instead of a breach: an EMPTY
split's partial merged with weight 1 instead of 0.  attn_decode_kernel writes (m, l, o) = (-inf, 0, 0) for an empty
chunk, so whatever weight the merge gives it multiplies zeros (and with every split empty, n = 0, L stays 0 and the
output stays zero): the wrong operation computes the same function, bit for bit.  What that guard can get wrong
visibly is the partial itself; ``empty-stale`` (the empty split writes nothing and the merge reads another split's
partial in its place) stands in for it and is rejected."""
import numpy as np
import pytest
import torch

import _decode_attn as D

ADMIT = {}    # family -> worst emulation err/bound
REJECT = {}   # mutation label -> (breach factor, old gate's relative norm)


@pytest.mark.parametrize("group,family,append", D.CASES, ids=[D.case_id(*x) for x in D.CASES])
def test_bound_admits_float32_emulation(group, family, append):
    """The emulation fits the bound, as it stands, at every split count the GPU matrix runs the case at."""
    c = D.group_case(group, family, append)
    for splits in D.case_splits(group, family):
        r = D.ratio(D.emu_decode(c, splits), c.O, c.bound)
        ADMIT[family] = max(ADMIT.get(family, 0.0), r)
        print(f"{D.case_id(group, family, append)} splits {splits}: emulation err/bound {r:.4f}")
        assert r <= 1.0, (c.name, splits, r)


@pytest.mark.parametrize("group,family,append,splits", [("A", "benign", 0, 1), ("A", "benign", 1, 5),
                                                         ("B", "benign", 1, 7), ("A", "peaked", 1, 32),
                                                         ("B", "lonely-split", 1, 3), ("D8", "benign", 1, 0)])
def test_structure_in_fp64_is_the_reference(group, family, append, splits):
    """The restatement run in float64 with nothing switched on agrees with the reference formula to a millionth of
    the bound: chunking, slots and merges lose or double no row."""
    c = D.group_case(group, family, append)
    got = D.emu_decode(c, splits, dtype=np.float64)
    assert ((got - c.O).abs() / c.bound).max().item() < 1e-6, c.name


# ---- wrong operations -----------------------------------------------------------------------------------------------
# label -> (wrong, lens of the launch, family, append, splits, (sequence, lost row) that _draw looks at or None)
MUTATIONS = {
    "last row of chunk 0 lost, n = 100, splits 3": ("chunk-end", (1, 7, 100), "benign", 0, 3, (2, 63)),
    "last row of chunk 0 lost, n = 257, splits 2": ("chunk-end", (1, 7, 257), "benign", 0, 2, (2, 159)),
    "row 128 lost, n = 200": ("row128", (1, 7, 200), "benign", 0, 1, (2, 128)),
    "slot 31 out of the LDS merge": ("slot31", (7, 33, 100), "benign", 0, 1, None),
    "non-maximal split merged with weight 1": ("split-w1", (7, 33, 100), "lonely-split", 0, 3, None),
    "appended row left out": ("no-append", (7, 33, 100), "benign", 1, 1, None),
    "appended V with the stale cache K": ("stale-k", (7, 33, 100), "benign", 1, 1, None),
    "scale 1/8 applied twice": ("scale2", (7, 33, 100), "benign", 0, 1, None),
    "empty split's partial not written, n = 33, splits 32": ("empty-stale", (7, 33, 100), "benign", 0, 32, None),
}
MAX_LEN, H = 320, 2


def _draw(lens, family, append, look):
    """The data of a lost-row check.  A key that carries next to no weight can be lost without changing anything a test
    could see, so the check runs on the first draw in which the lost key carries at least the mean weight of its row
    (head 0).  The criterion reads the fp64 reference only; the chosen draw is printed."""
    if look is None:
        return 0
    b, t = look
    for salt in range(256):
        c = D.make_case(MAX_LEN, H, lens, family, append, salt, "mutation")
        P = c.P[b][0]
        if P[t].item() * P.numel() >= 1.0:
            print(f"lens {lens}, key {t} of sequence {b}: draw {salt}, weight {P[t].item() * P.numel():.2f} x the "
                  f"row's mean")
            return salt
    raise AssertionError("no draw meets the criterion")


@pytest.mark.parametrize("label", MUTATIONS)
def test_bound_rejects_wrong_operation(label):
    """The wrong operation's fp64 result breaches the right operation's bound in at least one element."""
    wrong, lens, family, append, splits, look = MUTATIONS[label]
    c = D.make_case(MAX_LEN, H, lens, family, append, _draw(lens, family, append, look), "mutation")
    right = D.emu_decode(c, splits, dtype=np.float64)
    assert D.ratio(right, c.O, c.bound) < 1e-6
    got = D.emu_decode(c, splits, dtype=np.float64, wrong=wrong)
    breach, rel = D.ratio(got, c.O, c.bound), D.old_gate_rel(got, c.O)
    REJECT[label] = (breach, rel)
    print(f"{label}: breach {breach:.3g}x; the whole-tensor norm gate sees {rel:.2e} "
          f"({'ADMITS' if rel < D.OLD_GATE else 'rejects'} at {D.OLD_GATE:g})")
    assert breach > 1.0, (label, breach)


def test_empty_split_weight_cannot_be_seen():
    """n = 33 at 32 splits (two live chunks, thirty empty) and n = 0 (all empty): an empty split's (-inf, 0, 0) merged
    with weight 1 gives the same bits as weight 0, in float64 and in float32 (module docstring)."""
    c = D.make_case(MAX_LEN, H, (0, 33, 100), "benign", 0, 0, "mutation")
    for dtype in (np.float64, np.float32):
        a, b = D.emu_decode(c, 32, dtype=dtype), D.emu_decode(c, 32, dtype=dtype, wrong="empty-w1")
        assert torch.equal(a.float(), b.float())
    REJECT["empty split's -inf partial given weight 1"] = (0.0, 0.0)


def test_check_names_the_worst_element():
    """The GPU matrix's own check passes the reference rounded to bf16, raises on a wrong result with the sequence,
    its n, the head and the dim of the worst element, and refuses a NaN."""
    c = D.make_case(MAX_LEN, H, (7, 33, 100), "benign", 1, 0, "mutation")
    assert D.check(c, "rounded reference", c.O.bfloat16()) <= 1.0
    with pytest.raises(AssertionError, match=r"worst err/bound .* at sequence \d \(n = \d+\), head \d, dim \d+"):
        D.check(c, "appended row left out", D.emu_decode(c, 1, dtype=np.float64, wrong="no-append"))
    bad = c.O.clone()
    bad[1, 5] = float("nan")
    with pytest.raises(AssertionError, match="NaN"):
        D.check(c, "a NaN", bad)
    D.WORST.pop(("benign", "mutation"), None)


def test_tables():
    """Prints the admit table (worst emulation err/bound per family) and the reject table with the older gate's
    verdict next to it.  The older gate's column is a record, not an assertion."""
    print("worst emulation err/bound per family:")
    for fam in sorted(ADMIT):
        print(f"  {fam:<13s} {ADMIT[fam]:.4f}")
    print(f"breach of the wrong operations (fp64 result against the right operation's bound) | relative norm of the "
          f"whole output, gated at {D.OLD_GATE:g} before:")
    for label, (breach, rel) in REJECT.items():
        verdict = "same function" if breach == 0.0 else ("ADMITTED" if rel < D.OLD_GATE else "rejected")
        print(f"  {label:<55s} {breach:10.3g}x | {rel:.2e} {verdict}")
