"""The sampling rule of ergm_sample_rows (include/ergm_hip.h) restated in fp64 — test helper only.  It builds on
tests/_topp.py (the plain nucleus rule) and oracle/philox.py (through _topp.uniform).

Steps 1 to 3 (penalty over the seen tokens, the eos mask, temperature) are single IEEE f32 operations per logit, so the
helper takes them in f32 as the kernel does and every later step in fp64: p = softmax over the tokens that hold one,
rank by descending p with ties by ascending id, top-k (on for 1 <= k < the number of tokens whose integer mass
floor(e · 2^30) is positive), top-p over the renormalised top-k set, and the draw of _topp.draw.
"""
import numpy as np

import _topp
from _topp import uniform  # noqa: F401  (the same Philox word as the old sampler)


def _factor(v):
    v = np.float32(v)
    return v if np.isfinite(v) and v > 0 else np.float32(1.0)


def process(row, seen=(), rep=1.0, temp=1.0, no_eos=None):
    """Steps 1 to 3 on one logit row, in f32: NaN marks the masked eos (a slot that holds no token)."""
    x = np.asarray(row, dtype=np.float32).copy()
    r, t = _factor(rep), _factor(temp)
    idx = np.array(sorted(set(int(i) for i in seen)), dtype=np.int64)
    if idx.size:
        v = x[idx]
        x[idx] = np.where(v < 0, v * r, v / r)
    if no_eos is not None:
        x[no_eos] = np.nan
    return (x / t).astype(np.float32)


class Ranking:
    """The processed row ranked: ``order`` (token ids by rank), ``cum`` (inclusive cumulative p by rank, of the whole
    row), ``k`` (the ranks that remain under top-k; all of them when it is off), ``p`` (per token id)."""

    def __init__(self, row, top_k=0, **proc):
        x = process(row, **proc)
        valid = np.flatnonzero(~np.isnan(x))
        xv = x[valid].astype(np.float64)
        self.x, self.valid = x, valid
        self.p = np.zeros(x.size)
        self.p[valid] = _topp.softmax64(xv)
        order, self.cum = _topp.ranked(self.p[valid])
        self.order = valid[order]
        with_mass = int((np.floor(np.exp(xv - xv.max()) * 2.0 ** 30) > 0).sum())
        self.k = int(top_k) if 1 <= top_k < with_mass else self.order.size
        self.Sk = self.cum[self.k - 1]   # the share of the row's probability that remains under top-k


def kept_set(row, top_p, top_k=0, **proc):
    """(kept token ids ascending, p per token id of the processed row)."""
    r = Ranking(row, top_k, **proc)
    before = np.concatenate(([0.0], r.cum[:-1]))
    keep = (np.arange(r.order.size) < r.k) & (before <= float(np.float32(top_p)) * r.Sk)
    keep[0] = True
    n = int(keep.sum())
    assert keep[:n].all()
    return np.sort(r.order[:n]), r.p


def cut_margin(row, top_p, top_k=0, **proc):
    """(lo, hi): how far top_p lies inside the interval (cum[r-1], cum[r]] that contains it, of the ranking
    renormalised over the top-k set; hi is inf when top_p lies above the last one."""
    r = Ranking(row, top_k, **proc)
    cum = r.cum[:r.k] / r.Sk
    tp = float(np.float32(top_p))
    i = int(np.searchsorted(cum, tp, side="left"))
    lo = tp - (cum[i - 1] if i > 0 else 0.0)
    hi = (cum[i] if i < cum.size else np.inf) - tp
    return lo, hi


def draw(row, top_p, u, top_k=0, **proc):
    """(token, distance of u·mass to the nearest CDF boundary as a share of the mass, kept ids, kept mass)."""
    kept, p = kept_set(row, top_p, top_k, **proc)
    cdf = np.cumsum(p[kept])
    mass = cdf[-1]
    i = min(int(np.searchsorted(cdf, u * mass, side="left")), kept.size - 1)
    gap = np.abs(cdf - u * mass).min() / mass
    return int(kept[i]), gap, kept, mass


def logprob(row, token, **proc):
    """ln p(token) under the processed distribution before truncation."""
    x = process(row, **proc)
    xv = x[~np.isnan(x)].astype(np.float64)
    return float(np.float64(x[token]) - xv.max() - np.log(np.exp(xv - xv.max()).sum()))
