"""Extension of live sequences without a GPU: the new entry points (ergm_attn_fwd_extend, ergm_rows_to_slots_at,
ergm_decode_extend, ergm_decode_extend_launches) are declared, bound and exported with the ABI still 14; every refusal
of ergm_decode_extend comes back as ERGM_EINVAL with a telling message on fake pointers, before anything launches; and
the dry launch count of an extension.  Plan and helpers are tests/test_continuous_abi.py's."""
import ctypes as C
import re

import test_continuous_abi as CA
from ergm_amd import _lib as L

NEW = ["ergm_attn_fwd_extend", "ergm_rows_to_slots_at", "ergm_decode_extend", "ergm_decode_extend_launches"]
TINY = CA.TINY


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(CA.HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and lib.ergm_version() == 14
    assert int(re.search(r"#define ERGM_ABI_VERSION (\d+)", src).group(1)) == 14
    assert int(re.search(r"#define ERGM_EXTEND_META_ROWS (\d+)", src).group(1)) == L.EXTEND_META_ROWS
    assert int(re.search(r"#define ERGM_ADMIT_META_ROWS (\d+)", src).group(1)) == L.ADMIT_META_ROWS   # as it was


def test_extend_refusals_without_a_gpu():
    lib = L.load()
    plan, keep, p = CA._plan()
    big = 1 << 30
    try:
        ptrs = (C.c_void_p * 2)(p.value, p.value)

        def extend(slots, past, lens, caps, new, ws_bytes=big, ids=p, meta=p, pos=p):
            n = len(slots)
            return lib.ergm_decode_extend(plan, n, CA._arr(*slots), CA._arr(*past), CA._arr(*lens), CA._arr(*caps),
                                          CA._arr(*new), meta, ids, p, pos, p, ws_bytes, None)

        def refused(word, *a, **kw):
            assert extend(*a, **kw) == L.ERGM_EINVAL
            assert word in L.last_error(), (word, L.last_error())

        refused("slots bound", [0], [8], [5], [7], [4])
        assert lib.ergm_decode_bind_slots(plan, ptrs, ptrs, p, p, p, p, p, p, p) == L.ERGM_OK
        # every refusal of the issue's list
        refused("slot 4", [4], [8], [5], [7], [4])                          # a slot out of range
        refused("slot -1", [-1], [8], [5], [7], [4])
        refused("named twice", [2, 0, 2], [8, 8, 8], [5, 6, 7], [7, 7, 7], [4, 4, 4])
        refused("no new token", [0], [8], [0], [7], [4])                    # n_b < 1
        refused("past", [0], [1], [5], [7], [4])                            # past_b < 2
        refused("past", [0], [0], [5], [7], [4])
        refused("cap_max", [0], [8], [5], [0], [4])                         # c_b outside [1, cap_max]
        refused("cap_max", [0], [8], [5], [33], [4])
        refused("max_new", [0], [8], [5], [7], [0])                         # max_new < 1
        refused("max_len", [0], [8], [5], [7], [20])                        # past_b + n_b + max_new > max_len
        refused("max_len", [0], [30], [2], [7], [1])
        refused("max_len", [0], [33], [1], [7], [1])
        refused("workspace", [0, 1], [8, 8], [16, 15], [7, 7], [1, 1], ws_bytes=CA._admit_ws(30, 1))   # 31 rows > 30
        refused("n_seq", [0, 1, 2, 3, 0], [8] * 5, [1] * 5, [1] * 5, [1] * 5)
        refused("null", [0], [8], [5], [7], [4], ids=None)
        refused("null", [0], [8], [5], [7], [4], meta=None)
        refused("null", [0], [8], [5], [7], [4], pos=None)
        assert lib.ergm_decode_extend(None, 1, CA._arr(0), CA._arr(8), CA._arr(5), CA._arr(7), CA._arr(4), p, p, p, p, p, big,
                                      None) == L.ERGM_EINVAL
        # the admission's refusals are what they were
        assert lib.ergm_decode_admit(plan, 1, CA._arr(4), CA._arr(5), CA._arr(7), CA._arr(4), p, p, p, p, None, None, None, p,
                                     big, None) == L.ERGM_EINVAL and "slot 4" in L.last_error()
    finally:
        lib.ergm_decode_destroy(plan)


def _gemm_kernels(M, N, K, nk=False, c_dtype=L.BF16, epi=L.EPI_BIAS, ldb=None):
    """1, or 2 when ergm_gemm_plan splits K (the GEMM and its reduction), for the executor's descriptor."""
    keep, p = CA._buf()
    g = L.GemmDesc(M=M, N=N, K=K, lda=K, ldb=ldb or (K if nk else N), ldc=N, a_layout=L.MK,
                   b_layout=L.NK if nk else L.KN, c_dtype=c_dtype, epilogue=epi, alpha=1.0)
    if epi != L.EPI_NONE:
        g.bias = p
    if epi == L.EPI_BIAS_RESID:
        g.aux, g.ld_aux = p, N
    if epi == L.EPI_BIAS_GELU:
        g.aux_out, g.ld_aux_out = p, N
    cfg, split, flags = C.c_int(), C.c_int(), C.c_int()
    assert L.load().ergm_gemm_plan(C.byref(g), C.byref(cfg), C.byref(split), C.byref(flags)) == L.ERGM_OK, L.last_error()
    return 2 if split.value > 1 else 1


def _block_gemms(R, E, F):
    """The six GEMMs of a block over R rows, in every mode: qkv, the cross query, c_fc and the three projections."""
    return (_gemm_kernels(R, 3 * E, E) + _gemm_kernels(R, E, E) + _gemm_kernels(R, F, E, epi=L.EPI_BIAS_GELU)
            + 2 * _gemm_kernels(R, E, E, c_dtype=L.F32, epi=L.EPI_BIAS_RESID)
            + _gemm_kernels(R, E, F, c_dtype=L.F32, epi=L.EPI_BIAS_RESID))


def _head_gemm(rows, E, Vp):
    return _gemm_kernels(rows, Vp, E, nk=True, c_dtype=L.F32, epi=L.EPI_NONE)


def extend_kernels(R, n_seq, E, F, Vp, n_layer):
    """The launch sequence of ergm_decode_extend, counted by hand: the embedding; per block 3 LayerNorms, the row
    scatter, the two attentions and 6 GEMMs; the gather of the last rows, ln_f, the head, the logits scatter and the
    slot state."""
    return 1 + n_layer * (6 + _block_gemms(R, E, F)) + 4 + _head_gemm(n_seq, E, Vp)


def admit_kernels(R, Rc, n_seq, E, F, Vp, n_layer):
    """The launch sequence of ergm_decode_admit, counted by hand: the packed embedding; per block 3 LayerNorms, the two
    ragged attentions, the two row scatters, the block's 6 GEMMs and the caption K | V GEMM over layer l's columns of
    the stacked weight (ldb = L·2E); the gather of the last rows, ln_f, the head, the logits scatter, the slot state."""
    cap = _gemm_kernels(Rc, 2 * E, E, ldb=n_layer * 2 * E)
    return 1 + n_layer * (7 + _block_gemms(R, E, F) + cap) + 4 + _head_gemm(n_seq, E, Vp)


def _attn_decode_kernels(B, H, rows):
    """Launches of one ergm_attn_decode call with splits = 0, from the header's description: the partials of `splits`
    chunks go through a workspace of B·H·splits·66 floats, ergm_attn_decode_workspace_size covers the automatic choice,
    and more than one split adds the merge.  Where the query has room for one split only, the choice is 1 and the call
    is one launch.  Where it has room for more the header does not fix the choice ("1 when B*H fills the chip"):
    None, and the caller stays with a bound."""
    room = L.load().ergm_attn_decode_workspace_size(B, H, rows) // (B * H * 66 * 4)
    return 1 if room == 1 else None


def step_kernels(B, engine, E, F, Vp, n_layer, H, max_len, cap_rows):
    """The launch sequence of one decode step over B rows, counted by hand: the embedding; per block the two decode
    attentions and, on engine 0, 3 LayerNorms and 6 GEMMs, on engine 1 one ergm_linear_rows in the place of each
    LayerNorm + GEMM pair and of each projection (6 launches); ln_f, the head GEMM (both engines) and the length
    update.  None where the attention's split choice cannot be told from the header."""
    attn = [_attn_decode_kernels(B, H, max_len), _attn_decode_kernels(B, H, cap_rows)]
    if None in attn:
        return None
    block = sum(attn) + (3 + _block_gemms(B, E, F) if engine == 0 else 6)
    return 1 + n_layer * block + 1 + _head_gemm(B, E, Vp) + 1


def test_admit_and_step_launch_counts_are_exact():
    """The dry walks against the hand counts, at the tiny dims: the admission at three row counts that take different
    GEMM configurations, for 1 and 3 sequences; the step unbound (all max_batch rows, cap_max caption rows) and bound
    to one sequence, on both engines."""
    lib = L.load()
    plan, keep, p = CA._plan()
    E, F, Vp, n_layer, H = (TINY[k] for k in ("n_embd", "n_inner", "vocab_pad", "n_layer", "n_head"))
    try:
        for rows, cap_rows in ((3, 3), (30, 22), (100, 64)):
            for n_seq in (1, 3):
                assert (lib.ergm_decode_admit_launches(plan, n_seq, rows, cap_rows)
                        == admit_kernels(rows, cap_rows, n_seq, E, F, Vp, n_layer)), (rows, cap_rows, n_seq)
        ptrs = (C.c_void_p * n_layer)(*[p.value] * n_layer)
        for B, Sc in ((TINY["max_batch"], TINY["cap_max"]), (1, 4)):
            if B == 1:
                assert lib.ergm_decode_bind(plan, 1, 8, ptrs, ptrs, Sc, p, p, p, p) == L.ERGM_OK
            for engine in (0, 1):
                want = step_kernels(B, engine, E, F, Vp, n_layer, H, TINY["max_len"], Sc)
                assert want is not None and lib.ergm_decode_launches(plan, engine) == want, (B, engine)
    finally:
        lib.ergm_decode_destroy(plan)


def test_extend_launch_count_is_a_dry_walk():
    """12 kernels per block + 6 when no GEMM splits K, a split-K GEMM adding its reduction; the count does not depend
    on the number of sequences."""
    lib = L.load()
    plan, keep, p = CA._plan()
    try:
        for rows in (3, 12, 30, 100):
            one, three = lib.ergm_decode_extend_launches(plan, 1, rows), lib.ergm_decode_extend_launches(plan, 3, rows)
            assert one == extend_kernels(rows, 1, TINY["n_embd"], TINY["n_inner"], TINY["vocab_pad"], TINY["n_layer"]), rows
            assert one == three >= 12 * TINY["n_layer"] + 6, rows
        assert lib.ergm_decode_extend_launches(plan, 1, 12) == 12 * TINY["n_layer"] + 6
        assert lib.ergm_decode_extend_launches(plan, 0, 30) == L.ERGM_EINVAL
        assert lib.ergm_decode_extend_launches(plan, 3, 2) == L.ERGM_EINVAL
        assert lib.ergm_decode_extend_launches(plan, 1, 4 * 32 + 1) == L.ERGM_EINVAL
        assert lib.ergm_decode_extend_launches(None, 1, 30) == L.ERGM_EINVAL
        # the admission's count is what it was
        assert lib.ergm_decode_admit_launches(plan, 1, 30, 22) >= 14 * TINY["n_layer"] + 6
    finally:
        lib.ergm_decode_destroy(plan)
