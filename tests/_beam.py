"""The beam-search rule of include/ergm_hip.h (ergm_beam_select) restated with numpy, for the tests: log-probabilities in
fp64 from the f32 logits, the selection and the slot assignment as the header states them, and the margin of each group:
the fp64 gap between its W-th and its (W+1)-th candidate (inf when there is no (W+1)-th).  ``strict`` is the gap from the
W-th candidate to the next smaller value, for the cases built around exact ties (bitwise-equal inputs, where fp64 and
f32 agree that the values are equal and only the tie rule decides)."""
import math

import numpy as np


def select(logits, scores, finished, W, eos_id):
    """logits [R, V] f32, scores [R] f32, finished [R] -> dict of parent, token (int64 [R]), score (f64 [R]), finished
    (uint8 [R]), pairs (per group: the set of selected (parent row, token)), margin (per group)."""
    logits = np.asarray(logits, dtype=np.float32)
    R, V = logits.shape
    scores = np.asarray(scores, dtype=np.float64)
    finished = np.asarray(finished).astype(bool)
    parent = np.arange(R, dtype=np.int64)
    token = np.full(R, eos_id, dtype=np.int64)
    new_score = np.full(R, -np.inf)
    new_fin = np.ones(R, dtype=np.uint8)
    pairs, margins, strict = [], [], []
    for g0 in range(0, R, W):
        cands = []   # (c, beam, token): of a live beam its best W + 1, more cannot reach the first W + 1 of the group
        for w in range(W):
            r = g0 + w
            if not scores[r] > -np.inf:
                continue
            if finished[r]:
                cands.append((scores[r], w, eos_id))
                continue
            x = logits[r].astype(np.float64)
            ok = np.isfinite(x)
            if not ok.any():
                continue
            mx = x[ok].max()
            lse = mx + math.log(np.exp(x[ok] - mx).sum())
            c = np.where(ok, scores[r] + x - lse, -np.inf)
            idx = np.nonzero(ok)[0]
            # every candidate tied with the (W+1)-th best value, so that ties are ranked by token among all of them
            kth = np.sort(c[idx])[::-1][min(W, len(idx) - 1)]
            for j in idx[c[idx] >= kth]:
                cands.append((float(c[j]), w, int(j)))
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        sel = cands[:W]
        margins.append(sel[-1][0] - cands[W][0] if len(cands) > W else math.inf)
        below = [t[0] for t in cands if sel and t[0] < sel[-1][0]]
        strict.append(sel[-1][0] - below[0] if below else math.inf)
        pairs.append({(g0 + w, j) for _, w, j in sel})
        # slot assignment: by (beam, token); a beam's first child stays, the rest fill the childless rows in order
        sel.sort(key=lambda t: (t[1], t[2]))
        has = sorted({w for _, w, _ in sel})
        free = [w for w in range(W) if w not in has]
        seen = set()
        for c, w, j in sel:
            if w not in seen:
                seen.add(w)
                dst = w
            else:
                dst = free.pop(0)
            r = g0 + dst
            parent[r], token[r], new_score[r] = g0 + w, j, c
            new_fin[r] = 1 if (finished[g0 + w] or j == eos_id) else 0
    return dict(parent=parent, token=token, score=new_score, finished=new_fin, pairs=pairs, margin=margins, strict=strict)


def slot_property(parent, token, W):
    """The slot-assignment property of a select's output: within each group, with the children ordered by (parent,
    token), a parent's first child sits in the parent's own row, and the others fill the childless rows in ascending
    order.  Rows that died (parent == self with score -inf) are passed as the caller filters them."""
    parent, token = [int(p) for p in parent], [int(t) for t in token]
    for g0 in range(0, len(parent), W):
        rows = list(range(g0, g0 + W))
        kids = sorted((parent[r], token[r], r) for r in rows)
        firsts, rest = {}, []
        for p, t, r in kids:
            if p not in firsts:
                firsts[p] = r
            else:
                rest.append(r)
        if any(p != r for p, r in firsts.items()):
            return False
        free = [r for r in rows if r not in firsts]
        if rest != free[:len(rest)]:
            return False
    return True
