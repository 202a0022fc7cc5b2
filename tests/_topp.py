"""The nucleus-sampling rule of ergm_topp_sample (include/ergm_hip.h) restated in fp64 — test helper only.

p = softmax(row); rank by descending p, ties by ascending token id; rank r is kept iff r == 0 or the summed p of
the ranks < r is <= top_p; the draw takes the first kept token, in ascending token id, whose running sum of kept
p reaches u · (kept mass), u = (w + 0.5) / 2^32 with w = word 0 of Philox4x32-10({b, 0, 0xE5A3, step}, seed).
"""
import numpy as np

from oracle.philox import philox4x32_10


def softmax64(row):
    x = np.asarray(row, dtype=np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def ranked(p):
    """Token ids by descending p, ties by ascending id, and the inclusive cumulative p in that order."""
    order = np.lexsort((np.arange(p.size), -p))
    return order, np.cumsum(p[order])


def kept_set(row, top_p):
    """(kept token ids ascending, p) for one logit row; top_p as the kernel sees it (float32)."""
    p = softmax64(row)
    order, cum = ranked(p)
    before = np.concatenate(([0.0], cum[:-1]))
    keep = before <= float(np.float32(top_p))
    keep[0] = True
    k = int(keep.sum())
    assert keep[:k].all()  # a prefix of the ranking
    return np.sort(order[:k]), p


def cut_margin(row, top_p):
    """(lo, hi): how far top_p lies inside the interval (cum[r-1], cum[r]] of the ranking that contains it."""
    p = softmax64(row)
    _, cum = ranked(p)
    tp = float(np.float32(top_p))
    r = int(np.searchsorted(cum, tp, side="left"))  # first cum[r] >= top_p
    lo = tp - (cum[r - 1] if r > 0 else 0.0)
    hi = (cum[r] if r < cum.size else np.inf) - tp
    return lo, hi


def uniform(seed, b, step):
    w = philox4x32_10(b, 0, 0xE5A3, step, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return (float(w) + 0.5) / 4294967296.0


def draw(row, top_p, u):
    """(token, distance of u·mass to the nearest CDF boundary as a share of the mass, kept ids, kept mass)."""
    kept, p = kept_set(row, top_p)
    cdf = np.cumsum(p[kept])
    mass = cdf[-1]
    i = min(int(np.searchsorted(cdf, u * mass, side="left")), kept.size - 1)
    gap = np.abs(cdf - u * mass).min() / mass
    return int(kept[i]), gap, kept, mass
