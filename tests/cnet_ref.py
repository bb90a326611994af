"""Plain-Python restatement of the N-best confusion network (test infrastructure only): the checker
for ``rs_cn_merge`` / ``rs_cn_oracle`` / ``rs_cn_vote`` (asr-rescoring_amd/csrc/k_cnet.hip).

* ``fold``         the sequential merge of Nbest_Align/preprocess.py:41-64,103-108, written from its
                   rules (two cursors, column 0 compared by value, the "*" branch that appends the other
                   alignment's entry without advancing it);
* ``closed_form``  the same table from per-gap counts (DESIGN "Confusion network"), in both modes, as
                   indices into the hypotheses (-1 = gap);
* ``brute_oracle`` every path through the slots, plain DP Levenshtein, lexicographic minimum of labels;
* ``dp_oracle``    suffix table E[s][j] + forward walk (what the kernel does);
* ``vote``         per-slot weighted vote, a Python float loop in ascending column order.

A hypothesis list is ``[top1, hyp2, ..., hypN]`` of token lists (any hashables except the gap "*").
"""
from __future__ import annotations

import itertools
from typing import List, Sequence

from oracle.align_ref import levenshtein_distance_alignment as ref_align

GAP = "*"
REFERENCE, EXACT = "reference", "exact"


def pair_alignments(hyps: Sequence[Sequence]) -> List[List[list]]:
    """[[top-1 token, hyp-n token], ...] per n >= 2, as preprocess.py:92-101."""
    out = []
    for h in hyps[1:]:
        a = ref_align(list(hyps[0]), list(h))
        out.append([[r, t] for r, t in zip(a[0], a[1])])
    return out


def fold_two(ai: List[list], aj: List[list]) -> List[list]:
    i, j, out = 0, 0, []
    while i < len(ai) and j < len(aj):
        if ai[i][0] == aj[j][0]:
            out.append(ai[i] + aj[j][1:])
            i += 1
            j += 1
        elif ai[i][0] == GAP:
            out.append(ai[i] + aj[j][1:])           # the quirk: j is not advanced
            i += 1
        else:
            out.append([GAP] * len(ai[i]) + aj[j][1:])
            j += 1
    while i < len(ai):
        out.append(ai[i] + [GAP] * len(aj[0][1:]))
        i += 1
    while j < len(aj):
        out.append([GAP] * len(ai[0]) + aj[j][1:])
        j += 1
    return out


def fold(hyps: Sequence[Sequence]) -> List[list]:
    """The reference's table (lists of tokens with "*"); raises IndexError where the reference does."""
    als = pair_alignments(hyps)
    merged = als.pop(0)
    for a in als:
        merged = fold_two(merged, a)
    return merged


def _pair_index_form(top1: Sequence, hyp: Sequence):
    """(k[g] for g = 0..L1, ins[g] = hyp indices inserted in gap g, a[g] = hyp index at position g or -1)."""
    al = ref_align(list(top1), list(hyp))
    L1 = len(top1)
    ins = [[] for _ in range(L1 + 1)]
    a = [-1] * L1
    g = hi = 0
    for r, t in zip(al[0], al[1]):
        idx = -1
        if t != GAP:
            idx = hi
            hi += 1
        if r == GAP:
            ins[g].append(idx)
        else:
            a[g] = idx
            g += 1
    assert g == L1 and hi == len(hyp)
    return ins, a


def closed_form(hyps: Sequence[Sequence], mode: str = EXACT) -> List[List[int]]:
    """src[slot][n]: index into hypothesis n, -1 for a gap; column 0 is the top-1."""
    N, L1 = len(hyps), len(hyps[0])
    forms = [_pair_index_form(hyps[0], h) for h in hyps[1:]]
    src = []
    for g in range(L1 + 1):
        K = max([len(ins[g]) for ins, _ in forms], default=0)
        for m in range(K):
            row, seen = [-1], 0
            for ins, a in forms:
                if m < len(ins[g]):
                    row.append(ins[g][m])
                elif mode == REFERENCE and m < seen and g < L1:
                    row.append(a[g])
                else:
                    row.append(-1)
                seen = max(seen, len(ins[g]))
            src.append(row)
        if g < L1:
            src.append([g] + [a[g] for _, a in forms])
    assert all(len(r) == N for r in src)
    return src


def table_tokens(hyps: Sequence[Sequence], src: List[List[int]]) -> List[list]:
    return [[hyps[n][i] if i >= 0 else GAP for n, i in enumerate(row)] for row in src]


def edit_distance(a: Sequence, b: Sequence) -> int:
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def _candidates(slot: Sequence):
    """Distinct entries of a slot in order of their first column: [(first column, entry)]."""
    seen, out = set(), []
    for c, t in enumerate(slot):
        if t not in seen:
            seen.add(t)
            out.append((c, t))
    return out


def n_paths(table: List[list]) -> int:
    n = 1
    for slot in table:
        n *= len(set(slot))
    return n


def brute_oracle(table: List[list], ref: Sequence):
    """(dist, labels) over every path; ties to the lexicographically smallest label vector."""
    best = None
    for path in itertools.product(*[_candidates(s) for s in table]):
        d = edit_distance([t for _, t in path if t != GAP], list(ref))
        key = (d, [c for c, _ in path])
        if best is None or key < best:
            best = key
    return best[0], best[1]


def dp_oracle(table: List[list], ref: Sequence):
    S, R = len(table), len(ref)
    ref = list(ref)
    E = [[0] * (R + 1) for _ in range(S + 1)]
    E[S] = [R - j for j in range(R + 1)]
    for s in range(S - 1, -1, -1):
        toks = set(table[s]) - {GAP}
        gap = GAP in table[s]
        skip = 0 if gap else 1                      # leave the slot without consuming ref[j]
        E[s][R] = E[s + 1][R] + skip
        for j in range(R - 1, -1, -1):
            v = min(E[s][j + 1] + 1, E[s + 1][j] + skip)
            if toks:
                v = min(v, E[s + 1][j + 1] + (ref[j] not in toks))
            E[s][j] = v
    dist = E[0][0]
    F = list(range(R + 1))
    labels = []
    for s in range(S):
        pick = -1
        for c, t in _candidates(table[s]):
            if t == GAP:
                Fn = F
            else:
                Fn = [F[0] + 1]
                for j in range(1, R + 1):
                    Fn.append(min(F[j] + 1, F[j - 1] + (t != ref[j - 1]), Fn[j - 1] + 1))
            if min(Fn[j] + E[s + 1][j] for j in range(R + 1)) == dist:
                pick, F = c, Fn
                break
        labels.append(pick)
    return dist, labels


def vote(table: List[list], weights: Sequence[float] = None):
    """Per slot (winning entry, its first column, its share of the weight), then the decode without gaps."""
    N = len(table[0]) if table else 0
    w = [1.0] * N if weights is None else [float(x) for x in weights]
    total = 0.0
    for n in range(N):
        total += w[n]
    win, col, share = [], [], []
    for slot in table:
        best = None
        for c, t in _candidates(slot):
            mass = 0.0
            for n in range(N):
                if slot[n] == t:
                    mass += w[n]
            if best is None or mass > best[0]:
                best = (mass, c, t)
        win.append(best[2])
        col.append(best[1])
        share.append(best[0] / total)
    return win, col, share, [t for t in win if t != GAP]


def oracle_cases(lists, cap: int = 20000, seed: int = 3):
    """(hyps, table, transcript) for both modes of every list whose table has at most ``cap`` paths; the
    transcript is a noisy copy of one hypothesis."""
    import random
    rng = random.Random(seed)
    out = []
    for hyps in lists:
        for mode in (REFERENCE, EXACT):
            table = table_tokens(hyps, closed_form(hyps, mode))
            if n_paths(table) > cap:
                continue
            alpha = sorted({t for h in hyps for t in h}) or ["a"]
            ref = [t if rng.random() < 0.7 else rng.choice(alpha) for t in rng.choice(hyps)]
            if rng.random() < 0.3:
                ref = ref[1:]
            out.append((hyps, mode, table, ref))
    return out
