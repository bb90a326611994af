"""The LM-weighted slot vote on the host: the restatement (tests/slotlm_ref.py) against the properties the
rule promises, and ``SlotTable.position_candidates`` / ``cnet.slot_lm_vote`` against the restatement, on
the hypothesis lists of tests/golden/cnet_merge.json with seeded synthetic weights and log-probs.

The product's table and plain vote come from the GPU; here a ``SlotTable`` is filled from the closed form
(``cnet_ref.closed_form``) and its ``vote`` answered by ``cnet_ref.vote``, so that the host code of
``position_candidates`` and ``slot_lm_vote`` runs as it is (tests/test_gpu_slotlm.py repeats the agreement
on a device-built table)."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import cnet_ref as C
import slotlm_ref as S
from asr_rescoring_amd import cnet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnet_merge.json")
LAMS = (0.3, 0.7, 1.0)


class HostTable(cnet.SlotTable):
    """A ``SlotTable`` over closed-form tables, voting through the restatement."""

    def __init__(self, lists):
        srcs = [C.closed_form(h, C.EXACT) for h in lists]
        vocab = {}
        ids = [[[vocab.setdefault(t, len(vocab)) for t in hyp] for hyp in h] for h in lists]
        n_slots = np.asarray([len(s) for s in srcs], np.int64)
        n_hyp = np.asarray([len(h) for h in lists], np.int64)
        flat = np.asarray([i for s in srcs for row in s for i in row] + [0], np.int32)
        d = {"utt_off_h": cnet._off(n_hyp), "slot_off": torch.from_numpy(cnet._off(n_slots)),
             "cell_off": torch.from_numpy(cnet._off(n_slots * n_hyp, np.int64)), "src": torch.from_numpy(flat)}
        super().__init__([[list(t) for t in h] for h in lists], ids, vocab, "exact", torch.device("cpu"), d)
        self.tables = [C.table_tokens(h, s) for h, s in zip(lists, srcs)]

    def vote(self, weights=None):
        w = cnet._flat_weights(self, weights)
        dec, cols, shares = [], [], []
        for u, t in enumerate(self.tables):
            _, col, share, d = C.vote(t, w[self.utt_off[u]:self.utt_off[u + 1]]) if t else ([], [], [], [])
            dec.append(d)
            cols.append(np.asarray(col, np.int32))
            shares.append(np.asarray(share, np.float64))
        return dec, cols, shares


@pytest.fixture(scope="module")
def setup():
    """(lists, tables, weights per list, {(u, s): lp}) over the fixture's lists with N >= 2: weights in
    (0, 1] with every fifth hypothesis at weight 0, log-probs uniform in [-12, 0]."""
    with open(GOLDEN, encoding="utf-8") as f:
        lists = [[list(h) for h in c["h"]] for c in json.load(f)["cases"]]
    lists = [h for h in lists if len(h) >= 2 and len(h[0]) >= 1]
    rng = random.Random(11)
    tables = [C.table_tokens(h, C.closed_form(h, C.EXACT)) for h in lists]
    weights = [[0.0 if (n + u) % 5 == 4 else rng.uniform(0.05, 1.0) for n in range(len(h))]
               for u, h in enumerate(lists)]
    lp = {}
    for u, t in enumerate(tables):
        for s, _, toks, _ in S.position_candidates(t):
            lp[(u, s)] = [rng.uniform(-12.0, 0.0) for _ in toks]
    assert len(lp) > 300
    return lists, tables, weights, lp


def lp_of(lp, u):
    return {s: v for (uu, s), v in lp.items() if uu == u}


def test_lam_zero_is_the_plain_vote(setup):
    _, tables, weights, lp = setup
    for u, t in enumerate(tables):
        assert S.slot_lm_vote(t, weights[u], lp_of(lp, u), 0.0) == C.vote(t, weights[u])


@pytest.mark.parametrize("lam", LAMS)
def test_gap_wins_exactly_when_it_wins_the_plain_vote(setup, lam):
    _, tables, weights, lp = setup
    n_gap = 0
    for u, t in enumerate(tables):
        plain = C.vote(t, weights[u])[0]
        got = S.slot_lm_vote(t, weights[u], lp_of(lp, u), lam)[0]
        assert [x == C.GAP for x in got] == [x == C.GAP for x in plain]
        n_gap += sum(x == C.GAP and (u, s) in lp for s, x in enumerate(plain))
    assert n_gap > 0                                # scored slots whose gap wins exist in the set


def test_lam_one_is_the_lm_argmax_among_the_massive_tokens(setup):
    _, tables, weights, lp = setup
    n = 0
    for (u, s), lps in lp.items():
        slot, w = tables[u][s], weights[u]
        T, _ = S.redistributed(slot, w, lps, 1.0)
        if not T or S.plain_winner(S.masses(slot, w))[1] == C.GAP:
            continue
        toks = [t for _, t in C._candidates(slot) if t != C.GAP]
        want = max(((lps[toks.index(t)], -c, t) for c, t, _, _ in T))[2]
        assert S.slot_vote(slot, w, lps, 1.0)[0] == want
        n += 1
    assert n > 100


@pytest.mark.parametrize("lam", LAMS)
def test_token_mass_is_redistributed_not_created(setup, lam):
    _, tables, weights, lp = setup
    for (u, s), lps in lp.items():
        T, M = S.redistributed(tables[u][s], weights[u], lps, lam)
        if T:
            assert abs(math.fsum(m2 for *_, m2 in T) - M) <= 1e-12 * M


@pytest.mark.parametrize("lam", LAMS)
def test_zero_mass_candidates_never_win(setup, lam):
    _, tables, weights, lp = setup
    n_zero = 0
    for (u, s), lps in lp.items():
        slot, w = tables[u][s], weights[u]
        ms = {t: m for _, t, m in S.masses(slot, w)}
        zero = [t for t, m in ms.items() if t != C.GAP and m == 0.0]
        if not zero or all(m == 0.0 for m in ms.values()):
            continue
        # the LM prefers a candidate nobody with weight proposed: it still cannot win
        toks = [t for _, t in C._candidates(slot) if t != C.GAP]
        boosted = [0.0 if t in zero else v - 30.0 for t, v in zip(toks, lps)]
        assert S.slot_vote(slot, w, boosted, lam)[0] not in zero
        n_zero += 1
    assert n_zero > 10


def test_ties_go_to_the_lower_first_column():
    slot = ["a", "b", "c", C.GAP, "b", "a"]
    w = [0.2, 0.1, 0.3, 0.05, 0.1, 0.0]
    # a and b: equal mass (0.2) and equal log-probs, c behind both at lam = 1
    for lam in (0.5, 1.0):
        assert S.slot_vote(slot, w, [-1.0, -1.0, -3.0], lam)[:2] == ("a", 0)
    assert S.slot_vote(["b", "a", "a", "b"], [0.25] * 4, [-2.0, -2.0], 0.4)[:2] == ("b", 0)
    # the plain vote's own tie rule decides the gap: a token in an earlier column with the gap's mass
    # beats it, and the LM then chooses among the tokens; a heavier gap stays the winner
    assert S.slot_vote(["a", C.GAP, "b"], [0.25, 0.25, 0.1], [-5.0, -0.1], 1.0)[:2] == ("b", 2)
    assert S.slot_vote(["a", C.GAP, "b"], [0.2, 0.4, 0.3], [-5.0, -0.1], 1.0)[:2] == (C.GAP, 1)


def test_slot_without_scores_or_without_token_mass_keeps_the_plain_vote():
    slot, w = ["a", "b", C.GAP], [0.0, 0.0, 0.0]
    assert S.slot_vote(slot, w, [-1.0, -0.5], 0.7) == S.slot_vote(slot, w, None, 0.7)
    assert S.slot_vote(["a", "b", "b"], [0.5, 0.3, 0.3], None, 1.0)[0] == "b"


def test_position_candidates_match_the_restatement(setup):
    lists, tables, _, _ = setup
    got = HostTable(lists).position_candidates()
    want = [(u, s, g, toks, cols) for u, t in enumerate(tables) for s, g, toks, cols in S.position_candidates(t)]
    assert got == want
    # g is the position in the top-1, and column 0 is always the first candidate
    for u, s, g, toks, cols in got:
        assert lists[u][0][g] == toks[0] and cols[0] == 0 and len(set(toks)) == len(toks) >= 2
    assert HostTable(lists).position_candidates(min_distinct=3) == \
        [(u, s, g, toks, cols) for u, t in enumerate(tables) for s, g, toks, cols in S.position_candidates(t, 3)]


@pytest.mark.parametrize("lam", (0.0,) + LAMS)
def test_slot_lm_vote_agrees_with_the_restatement_on_every_slot(setup, lam):
    lists, tables, weights, lp = setup
    table = HostTable(lists)
    dec, cols, shares = cnet.slot_lm_vote(table, weights, lp, lam)
    for u, t in enumerate(tables):
        _, col, share, want = S.slot_lm_vote(t, weights[u], lp_of(lp, u), lam)
        assert dec[u] == want
        assert list(cols[u]) == col
        np.testing.assert_allclose(shares[u], share, rtol=1e-12, atol=0)


def test_slot_lm_vote_rejects_a_wrong_number_of_scores(setup):
    lists, _, weights, lp = setup
    bad = dict(lp)
    k = next(iter(bad))
    bad[k] = list(bad[k]) + [-1.0]
    with pytest.raises(ValueError, match="log-probs"):
        cnet.slot_lm_vote(HostTable(lists), weights, bad, 0.5)


def test_candidate_sort_round_trips_lists_with_duplicates():
    rng = random.Random(5)
    lens = [0, 1, 2, 7, 0, 64, 3]
    c_off = [0]
    for n in lens:
        c_off.append(c_off[-1] + n)
    cand = [rng.choice([0, 5, 5, 63, 64, 999]) for _ in range(c_off[-1])]
    ids, perm = S.sort_candidates(c_off, cand)
    assert sorted(perm) == list(range(len(cand)))
    for a, b in zip(c_off[:-1], c_off[1:]):
        assert ids[a:b] == sorted(cand[a:b]) and all(a <= p < b for p in perm[a:b])
        # equal ids keep their original order
        assert all(perm[t] < perm[t + 1] for t in range(a, b - 1) if ids[t] == ids[t + 1])
    out = [None] * len(cand)
    for t, p in enumerate(perm):
        out[p] = ids[t]
    assert out == cand
