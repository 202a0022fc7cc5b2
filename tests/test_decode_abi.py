"""The batched-generation entry points (ABI 13) without a GPU: exported and bound, argument errors reported from the
host before anything launches, the workspace query host-only; and the fp64 restatement of the sampling rule
(tests/_topp.py) against a literal transcription of the reference's sort / cumsum / shift / scatter lines."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _topp
from ergm_amd import _lib as L

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ergm_hip.h")
NEW = ["ergm_attn_decode", "ergm_attn_decode_workspace_size", "ergm_embed_rows", "ergm_topp_sample"]


def test_new_exports_declared_bound_and_present():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert L.ABI_VERSION == 14 and re.search(r"#define\s+ERGM_ABI_VERSION\s+14\b", src)


def _buf(nbytes=256):
    """A host buffer and a 16-byte aligned address inside it (never dereferenced: every call below fails its
    host-side checks first)."""
    raw = C.create_string_buffer(nbytes + 16)
    return raw, C.c_void_p((C.addressof(raw) + 15) & ~15)


def _decode(lib, qkv, kc, vc, lens, out, B=2, H=2, max_len=64, append=1, splits=1, ld_qkv=384, ld_seq=64 * 256,
            ld_row=256, ldo=128, ws=None, ws_bytes=0):
    return lib.ergm_attn_decode(qkv, ld_qkv, kc, vc, ld_seq, ld_row, lens, B, H, max_len, append, splits, out, ldo, ws,
                                ws_bytes, None)


def test_attn_decode_errors_without_a_gpu():
    lib = L.load()
    keep, p = _buf()
    assert _decode(lib, None, p, p, p, p) == L.ERGM_EINVAL and "null" in L.last_error()
    assert _decode(lib, p, p, p, None, p) == L.ERGM_EINVAL and "null" in L.last_error()
    assert _decode(lib, p, p, p, p, None) == L.ERGM_EINVAL and "null" in L.last_error()
    for kw in (dict(B=0), dict(H=0), dict(max_len=0), dict(B=-3)):
        assert _decode(lib, p, p, p, p, p, **kw) == L.ERGM_EINVAL and "shape" in L.last_error(), kw
    for kw in (dict(ld_qkv=388), dict(ld_row=260), dict(ld_seq=64 * 256 + 4), dict(ldo=132)):
        assert _decode(lib, p, p, p, p, p, **kw) == L.ERGM_EINVAL and "multiples of 8" in L.last_error(), kw
    assert _decode(lib, p, p, p, p, p, ld_qkv=128) == L.ERGM_EINVAL and "stride" in L.last_error()  # no room for K | V
    assert _decode(lib, p, p, p, p, p, ld_seq=32 * 256) == L.ERGM_EINVAL and "stride" in L.last_error()
    assert _decode(lib, p, p, p, p, p, splits=4) == L.ERGM_EINVAL and "workspace" in L.last_error()
    need = 2 * 2 * 4 * 66 * 4
    assert _decode(lib, p, p, p, p, p, splits=4, ws=p, ws_bytes=need - 1) == L.ERGM_EINVAL
    assert "workspace" in L.last_error()
    assert _decode(lib, p, p, p, p, p, splits=33) == L.ERGM_EINVAL and "splits" in L.last_error()
    assert _decode(lib, p, p, p, p, p, append=2) == L.ERGM_EINVAL and "append" in L.last_error()


def test_embed_rows_and_topp_errors_without_a_gpu():
    lib = L.load()
    keep, p = _buf()
    assert lib.ergm_embed_rows(None, None, p, p, p, p, 2, 128, 500, 64, None) == L.ERGM_EINVAL
    assert "null" in L.last_error()
    assert lib.ergm_embed_rows(p, None, None, p, p, p, 2, 128, 500, 64, None) == L.ERGM_EINVAL
    assert "null" in L.last_error()
    for B, E, V, P in ((0, 128, 500, 64), (2, 0, 500, 64), (2, 126, 500, 64), (2, 128, 0, 64), (2, 128, 500, 0)):
        assert lib.ergm_embed_rows(p, None, p, p, p, p, B, E, V, P, None) == L.ERGM_EINVAL, (B, E, V, P)
        assert "shape" in L.last_error()
    assert lib.ergm_topp_sample(None, 512, 2, 500, 0.9, 1, 0, None, 1, p, None, None, None) == L.ERGM_EINVAL
    assert "null" in L.last_error()
    assert lib.ergm_topp_sample(p, 512, 2, 500, 0.9, 1, 0, None, 1, None, None, None, None) == L.ERGM_EINVAL
    assert "null" in L.last_error()
    for ldl, B, V in ((512, 0, 500), (512, 2, 0), (496, 2, 500)):
        assert lib.ergm_topp_sample(p, ldl, B, V, 0.9, 1, 0, None, 1, p, None, None, None) == L.ERGM_EINVAL
        assert "shape" in L.last_error()
    assert lib.ergm_topp_sample(p, 512, 2, 500, float("nan"), 1, 0, None, 1, p, None, None, None) == L.ERGM_EINVAL


def test_decode_workspace_query_is_host_only_and_monotone():
    ws = L.load().ergm_attn_decode_workspace_size
    assert ws(1, 12, 1024) >= 12 * 2 * 66 * 4  # room for a split across workgroups when B·H is small
    for a, b in (((1, 12, 1024), (2, 12, 1024)), ((4, 2, 256), (4, 3, 256)), ((1, 12, 128), (1, 12, 1024)),
                 ((32, 12, 64), (32, 12, 65)), ((3, 2, 1), (3, 2, 4096))):
        assert ws(*a) <= ws(*b), (a, b)
    assert ws(1, 12, 128) < ws(1, 12, 1024) and ws(1, 12, 1024) < ws(2, 12, 1024) < ws(2, 13, 1024)
    assert ws(0, 12, 1024) == 0 and ws(1, 12, -1) == 0


def _reference_kept(row, top_p):
    """src/main.py:259-270, literally (fp64 torch), as the set of tokens with nonzero probability afterwards."""
    probs = torch.softmax(torch.tensor(row, dtype=torch.float64).unsqueeze(0), dim=-1)
    sorted_probs, sorted_idxs = torch.sort(probs, descending=True)
    cumsum_probs = torch.cumsum(sorted_probs, dim=-1)
    idx_remove = cumsum_probs > top_p
    idx_remove[:, 1:] = idx_remove[:, :-1].clone()
    idx_remove[:, 0] = False
    sorted_probs[idx_remove] = 0.0
    sorted_probs /= torch.sum(sorted_probs, dim=-1, keepdim=True)
    probs = torch.zeros(probs.shape, dtype=torch.float64).scatter_(-1, sorted_idxs, sorted_probs)
    return np.flatnonzero(probs[0].numpy() > 0), probs[0].numpy()


@pytest.mark.parametrize("V,top_p,seed", [(500, 0.9, 0), (500, 0.5, 1), (500, 0.05, 2), (4001, 0.95, 3), (37, 1.0, 4)])
def test_helper_matches_the_reference_lines(V, top_p, seed):
    row = np.random.default_rng(seed).normal(size=V) * 2.0  # continuous: no ties
    assert np.unique(row).size == V
    kept, p = _topp.kept_set(row, np.float64(top_p))
    # the helper rounds top_p to float32 as the kernel receives it: use a value float32 holds exactly where it matters
    want, probs = _reference_kept(row, float(np.float32(top_p)))
    assert np.array_equal(kept, want)
    assert np.allclose(probs[kept], p[kept] / p[kept].sum(), rtol=1e-12)
    # and the draw walks the kept tokens in ascending id
    tok, _, _, mass = _topp.draw(row, top_p, 0.5)
    cdf = np.cumsum(p[kept])
    assert tok == kept[np.searchsorted(cdf, 0.5 * mass)]
    assert _topp.draw(row, top_p, 1e-12)[0] == kept[0] and _topp.draw(row, top_p, 1 - 1e-12)[0] == kept[-1]


def test_helper_ties_go_to_the_lower_id():
    p = np.full(10, 0.1 / 7)
    p[[7, 2, 5]] = 0.5, 0.2, 0.2
    kept, _ = _topp.kept_set(np.log(p), 0.6)
    assert kept.tolist() == [2, 7]
    lo, hi = _topp.cut_margin(np.log(p), 0.6)
    assert abs(lo - 0.1) < 1e-6 and abs(hi - 0.1) < 1e-6
