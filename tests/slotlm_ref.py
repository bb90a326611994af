"""Plain-Python restatement of the LM-weighted slot vote (test infrastructure only): the checker for
``SlotTable.position_candidates`` and ``cnet.slot_lm_vote`` (asr-rescoring_amd/cnet.py).

A table is ``cnet_ref.table_tokens(hyps, cnet_ref.closed_form(hyps, EXACT))``: slots of N entries, "*" the
gap, column 0 the top-1.  Everything is a Python float (float64) loop in ascending column order.

The rule, per slot that has LM scores (one log-prob per distinct non-gap entry, in order of first column):
  m_c    = sum of w over the columns holding c (the plain vote's masses, ``cnet_ref.vote``)
  T      = the non-gap candidates with m_c > 0,  M = sum of m_c over T
  s_c    = (1 - lam) ln m_c + lam (lp_c - logsumexp_T lp)        (lam == 1: the second term alone)
  m''_c  = M exp(s_c - logsumexp_T s)
The gap keeps its mass and its verdict: it wins exactly when it wins the plain vote.  Otherwise the
winner is the largest m''_c, equal ones by the lowest first column.  A slot without scores, or with
M == 0, keeps the plain vote; lam == 0 is the plain vote.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import cnet_ref as C

GAP = C.GAP


def position_candidates(table: List[list], min_distinct: int = 2):
    """[(slot, g, tokens, first columns)] of the slots whose column 0 is a top-1 token and that hold at
    least ``min_distinct`` distinct non-gap entries; g = that token's position in the top-1."""
    out, g = [], 0
    for s, slot in enumerate(table):
        if slot[0] == GAP:
            continue
        cands = [(c, t) for c, t in C._candidates(slot) if t != GAP]
        if len(cands) >= min_distinct:
            out.append((s, g, [t for _, t in cands], [c for c, _ in cands]))
        g += 1
    return out


def masses(slot: Sequence, w: Sequence[float]):
    """[(first column, entry, mass)] in order of first column, the gap included."""
    out = []
    for c, t in C._candidates(slot):
        m = 0.0
        for n in range(len(slot)):
            if slot[n] == t:
                m += float(w[n])
        out.append((c, t, m))
    return out


def lse(xs: Sequence[float]) -> float:
    mx = max(xs)
    tot = 0.0
    for x in xs:
        tot += math.exp(x - mx)
    return mx + math.log(tot)


def plain_winner(ms):
    best = None
    for c, t, m in ms:
        if best is None or m > best[2]:
            best = (c, t, m)
    return best


def redistributed(slot: Sequence, w: Sequence[float], lps: Sequence[float], lam: float):
    """(T as [(first column, token, m, m'')], M) of a scored slot; T empty when no token has mass."""
    toks = [(c, t, m) for c, t, m in masses(slot, w) if t != GAP]
    assert len(lps) == len(toks)
    T = [(c, t, m, float(lp)) for (c, t, m), lp in zip(toks, lps) if m > 0.0]
    if not T:
        return [], 0.0
    M = 0.0
    for _, _, m, _ in T:
        M += m
    L = lse([lp for *_, lp in T])
    s = [lp - L if lam == 1 else (1.0 - lam) * math.log(m) + lam * (lp - L) for _, _, m, lp in T]
    Ls = lse(s)
    return [(c, t, m, M * math.exp(x - Ls)) for (c, t, m, _), x in zip(T, s)], M


def slot_vote(slot: Sequence, w: Sequence[float], lps, lam: float):
    """(winning entry, its first column, its mass) of one slot; ``lps`` None = no LM scores."""
    ms = masses(slot, w)
    pc, pt, pm = plain_winner(ms)
    if lps is None or lam == 0 or pt == GAP:
        return pt, pc, pm
    T, _ = redistributed(slot, w, lps, lam)
    if not T:
        return pt, pc, pm
    best = None
    for c, t, _, m2 in T:
        if best is None or m2 > best[2]:
            best = (c, t, m2)
    return best[1], best[0], best[2]


def slot_lm_vote(table: List[list], weights: Sequence[float], slot_lp: Dict[int, Sequence[float]], lam: float):
    """(win, col, share, decode) like ``cnet_ref.vote``; ``slot_lp``: {slot: log-probs in
    ``position_candidates`` order}."""
    N = len(table[0]) if table else 0
    w = [1.0] * N if weights is None else [float(x) for x in weights]
    total = 0.0
    for n in range(N):
        total += w[n]
    win, col, share = [], [], []
    for s, slot in enumerate(table):
        t, c, m = slot_vote(slot, w, slot_lp.get(s), lam)
        win.append(t)
        col.append(c)
        share.append(m / total)
    return win, col, share, [t for t in win if t != GAP]


def sort_candidates(c_off: Sequence[int], cand: Sequence[int]):
    """The order ``rs_masked_logprob_cands`` gives every list: (sorted ids, perm) with each list sorted by
    (id, original index) and perm the original index of every entry."""
    ids, perm = [], []
    for a, b in zip(c_off[:-1], c_off[1:]):
        order = sorted(range(a, b), key=lambda t: (cand[t], t))
        perm += order
        ids += [cand[t] for t in order]
    return ids, perm
