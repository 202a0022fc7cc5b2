"""The logit rules of include/ergm_hip.h ("Logit rules") restated in plain Python — test helper only, no GPU.

``banned`` is the set of tokens one row may not take next; ``apply`` is ergm_logit_rules_apply over a whole buffer
(numpy, in place on a copy); ``parse_pool`` reads a bad-word pool row the way the kernel does; ``pool`` writes one.
``cases`` builds the rows tests/test_gpu_rules_ops.py runs: every case is a dict of one row's device values.
"""
import numpy as np

NGRAM_MAX = 8


def clamp(x, lo, hi):
    return max(lo, min(int(x), hi))


def parse_pool(row):
    """The sequences of a pool row: length-prefixed, ended by a length outside [1, 8], by a sequence the row cuts off,
    or by the end of the row."""
    row = [int(x) for x in row]
    words, q = [], 0
    while q < len(row):
        m = row[q]
        if m < 1 or m > NGRAM_MAX or q + m >= len(row):
            break
        words.append(tuple(row[q + 1:q + 1 + m]))
        q += 1 + m
    return words


def pool(words, cap):
    row = []
    for w in words:
        row += [len(w), *w]
    assert len(row) <= cap
    return row + [0] * (cap - len(row))


def banned(hist, length, max_len, V, eos_id, n=0, s0=0, words=()):
    """The tokens row ``hist`` (any sequence of ints, at least max_len long where length says so) may not take next."""
    L = clamp(length, 0, max_len)
    h = [int(x) for x in hist[:L]]
    out = set()
    if 1 <= n <= NGRAM_MAX:
        s = clamp(s0, 0, L)
        if L - s >= n - 1:
            tail = h[L - n + 1:L] if n > 1 else []
            for i in range(s, L - n + 1):
                if h[i:i + n - 1] == tail:
                    out.add(h[i + n - 1])
    for w in words:
        m = len(w)
        if m - 1 <= L and h[L - m + 1:L] == list(w[:m - 1]):
            out.add(int(w[m - 1]))
    return {j for j in out if 0 <= j < V and j != eos_id}


def apply(logits, V, hist, lens, eos_id, max_len, start=None, ngram=None, bad=None, finished=None):
    """ergm_logit_rules_apply on a numpy f32 buffer [R, ldl]: returns the copy with the bans written."""
    out = np.array(logits, dtype=np.float32, copy=True)
    for r in range(out.shape[0]):
        if finished is not None and finished[r]:
            continue
        words = parse_pool(bad[r]) if bad is not None else ()
        ban = banned(hist[r], lens[r], max_len, V, eos_id, 0 if ngram is None else int(ngram[r]),
                     0 if start is None else int(start[r]), words)
        for j in ban:
            out[r, j] = -np.inf
    return out


def repeats(seq, n, s0=0):
    """True when some n-gram occurs twice in seq[s0:]."""
    seq = [int(x) for x in seq[s0:]]
    grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    return len(set(grams)) != len(grams)


def brute_force_ngram(h, n, s0):
    """The n-gram rule by enumeration, written without reference to ``banned``: token j is banned iff appending it to
    h makes the last n-gram of h[s0:] + [j] equal an n-gram that h[s0:] already holds."""
    seg = list(h[s0:])
    if len(seg) < n - 1:
        return set()
    have = {tuple(seg[i:i + n]) for i in range(len(seg) - n + 1)}
    alphabet = set(h) | {0, 1, 2, 3}
    return {j for j in alphabet if tuple((seg + [j])[-n:]) in have}


# ---- the rows of the kernel test ------------------------------------------------------------------------------------
def cases(V, eos_id, max_len, cap, seed=0):
    """Rows for tests/test_gpu_rules_ops.py: a list of dicts with keys hist (max_len ints), len, start, ngram, bad (cap
    ints), finished.  Histories run over the 3-token alphabet {a, b, c} so several positions match."""
    rng = np.random.default_rng(seed)
    a, b, c = 3, V - 1, 7
    abc = [a, b, c]
    out = []

    def row(hist, length=None, start=0, ngram=0, bad=(), finished=0, raw_pool=None):
        hist = list(hist)
        length = len(hist) if length is None else length
        full = (hist + [int(x) for x in rng.choice(abc, max_len)])[:max_len]   # what lies past the length is live data
        out.append(dict(hist=full, len=length, start=start, ngram=ngram, finished=finished,
                        bad=list(raw_pool) if raw_pool is not None else pool(bad, cap)))

    rnd = lambda k: [int(x) for x in rng.choice(abc, k)]

    def pat(L, n):
        """L tokens that end in an (n-1)-gram T which also stands earlier, followed there by a, b, c in turn: a random
        front, blocks T + [follower], then T.  Too short for one block: random."""
        k = (L - (n - 1)) // n
        if n < 2 or k < 1:
            return rnd(L)
        T = rnd(n - 1)
        return rnd(L - (n - 1) - k * n) + [t for i in range(k) for t in T + [abc[i % 3]]] + T

    for n in (1, 2, 3, 8):
        for L in sorted({0, 1, max(n - 2, 0), n - 1, n, max_len}):
            row(pat(L, n), ngram=n)
        row(pat(max_len // 2, n), ngram=n, start=5)
    # a match that straddles s0 must not count: the bigram (a, b) lies at positions 1, 2 and s0 = 2
    row([c, a, b, c, c, a], ngram=2, start=2)
    row([c, a, b, c, c, a], ngram=2, start=1)            # ... and counts from s0 = 1
    row([a, b, a, b, a], ngram=3, start=9)               # s0 > L
    row([a, b, a, b, a], ngram=3, start=-4)              # negative s0
    row([a, eos_id, c, a], ngram=2)                      # the banned position holds eos: exempt
    row([a, -1, c, a, V, a, -1], ngram=2)                # entries outside [0, V) ban nothing, match themselves
    row([a, V, a], ngram=2)
    row([a, b, a, b], ngram=9)                           # n above the bound: off
    row([a, b, a, b], ngram=-2)
    # bad words
    row(rnd(6), bad=[(a,), (c,), (eos_id,)])                            # one-token words; eos is exempt
    row([c, c, a, b], bad=[(a, b, c)])                                  # the prefix is the tail
    row([c, a, b, c], bad=[(a, b, c)])                                  # one position off
    row([b], bad=[(a, b, c)])                                           # longer than the history
    row([], bad=[(a, b)], length=0)
    row([a], bad=[(a, b), (a, V), (a, -1)])                             # tokens outside the vocabulary ban nothing
    full = [(a,)] * (cap // 2) if cap % 2 == 0 else [(a,)] * ((cap - 3) // 2) + [(b, c)]
    row([b], bad=full)                                                  # a full pool without terminator
    assert len(pool(full, cap)) == cap and 0 not in pool(full, cap)
    row(rnd(5), raw_pool=[0, 1, a] + [1, c] * ((cap - 3) // 2) + [0] * ((cap - 3) % 2))   # a zero length in first place
    row(rnd(5), raw_pool=([1, a, 9, c] + [1, c] * cap)[:cap])           # a length above 8 ends the run
    row(rnd(5), raw_pool=([1, a] + [0] * cap)[:cap - 3] + [3, c, c])    # stray entries behind the terminator
    row([a, b], raw_pool=([1, a] * cap)[:cap - 2] + [2, b])             # the pool cuts the last sequence off
    row([c, a, b, a], ngram=2, bad=[(b, c), (a,)])                      # both rules in one row
    # row state
    row(rnd(9), ngram=2, bad=[(a,)], finished=1)                        # finished: untouched
    row(rnd(9))                                                         # everything off: untouched
    row(rnd(9), ngram=1, length=-5)
    row(rnd(max_len), ngram=1, length=max_len + 7)
    row(rnd(max_len), ngram=2, length=max_len + 7, bad=[(a, b)])
    return out
