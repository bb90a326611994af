"""The confusion-network restatement (tests/cnet_ref.py) against itself and against the reference's own
outputs (tests/golden/cnet_merge.json, written by tests/golden/make_cnet_golden.py): sequential fold ==
closed form (reference mode) == fixture; exact mode holds every hypothesis token exactly once, in order;
DP oracle == exhaustive search; oracle distance <= every single hypothesis; majority vote of N identical
hypotheses returns it."""
import json
import os

import pytest

import cnet_ref as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnet_merge.json")


@pytest.fixture(scope="module")
def fixture():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


def cases_of(fx):
    return [([list(h) for h in c["h"]], None if c["t"] is None else [list(s) for s in c["t"]]) for c in fx["cases"]]


def test_fold_equals_closed_form_equals_fixture(fixture):
    n_tab = n_quirk = 0
    for hyps, want in cases_of(fixture):
        closed = C.table_tokens(hyps, C.closed_form(hyps, C.REFERENCE))
        if want is None:                       # the reference raises IndexError: the closed form defines it
            with pytest.raises(IndexError):
                C.fold(hyps)
            continue
        assert C.fold(hyps) == want
        assert closed == want, hyps
        n_tab += 1
        n_quirk += closed != C.table_tokens(hyps, C.closed_form(hyps, C.EXACT))
    assert n_tab > 300 and n_quirk > 50       # the copies are common, so the fixture pins them


def test_fixture_known_answers(fixture):
    cs = cases_of(fixture)
    assert cs[0][1] == [["how", "how"], ["are", "are"], ["you", "you"], ["*", "doing"]]
    assert cs[1][1] == [["你", "你"], ["好", "好"], ["*", "不"], ["嗎", "好"]]


def test_exact_mode_holds_every_token_once_in_order(fixture):
    for hyps, _ in cases_of(fixture):
        src = C.closed_form(hyps, C.EXACT)
        for n, h in enumerate(hyps):
            assert [row[n] for row in src if row[n] >= 0] == list(range(len(h)))
        assert [row[0] >= 0 for row in src].count(True) == len(hyps[0])


def _oracle_cases(fixture):
    return C.oracle_cases([h for h, _ in cases_of(fixture)[:200]])


def test_dp_oracle_equals_brute_force(fixture):
    cs = _oracle_cases(fixture)
    assert len(cs) > 150
    for hyps, _, table, ref in cs:
        assert C.dp_oracle(table, ref) == C.brute_oracle(table, ref), (hyps, ref)
        assert C.dp_oracle(table, []) == C.brute_oracle(table, [])


def test_oracle_bounds_every_hypothesis(fixture):
    for hyps, _, table, ref in _oracle_cases(fixture):
        d, labels = C.dp_oracle(table, ref)
        assert d <= min(C.edit_distance(h, ref) for h in hyps)
        path = [slot[c] for slot, c in zip(table, labels)]
        assert C.edit_distance([t for t in path if t != C.GAP], ref) == d


def test_uniform_vote_of_identical_hypotheses():
    for n in (1, 2, 5):
        hyps = [list("abcab")] * n
        for mode in (C.REFERENCE, C.EXACT):
            table = C.table_tokens(hyps, C.closed_form(hyps, mode))
            win, col, share, dec = C.vote(table)
            assert dec == list("abcab") and col == [0] * 5 and share == [1.0] * 5
