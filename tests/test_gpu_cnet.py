"""GPU parity of the confusion-network kernels (rs_cn_merge / rs_cn_oracle / rs_cn_vote,
csrc/k_cnet.hip) with the restatement (tests/cnet_ref.py) and with the reference's own outputs
(tests/golden/cnet_merge.json): element for element for the table and the labels, bit for bit for the
vote's float64 share (the sum order is fixed)."""
import json
import os

import numpy as np
import pytest

import cnet_ref as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnet_merge.json")
MODES = (C.REFERENCE, C.EXACT)


@pytest.fixture(scope="module")
def fixture():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


def _rand(rng, n, alpha=30):
    return [chr(0x4e00 + int(c)) for c in rng.integers(0, alpha, n)]


def _edited(rng, base, k, alpha=30):
    h = list(base)
    for _ in range(k):
        op, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(h) + 1))
        if op == 0 and h:
            h[min(pos, len(h) - 1)] = _rand(rng, 1, alpha)[0]
        elif op == 1:
            h.insert(pos, _rand(rng, 1, alpha)[0])
        elif h:
            del h[min(pos, len(h) - 1)]
    return h


def _nbest(rng, n, length, alpha=30, edits=4):
    base = _rand(rng, length, alpha)
    return [base] + [_edited(rng, base, int(rng.integers(0, edits + 1)), alpha) for _ in range(n - 1)]


@pytest.fixture(scope="module")
def lists(fixture):
    """Every utterance of the merge tests, merged in ONE launch per mode (different N per utterance)."""
    rng = np.random.default_rng(11)
    fx = [[list(h) for h in c["h"]] for c in fixture["cases"]]
    ins = lambda k: list("a") + [f"x{i}" for i in range(k)] + list("b")      # noqa: E731
    extra = [
        [list("abcde")],                                        # N = 1
        [[]],                                                   # N = 1, empty
        [list("abcde"), list("abde")],                          # N = 2
        _nbest(rng, 65, 9, alpha=5),                            # past one wave of columns
        [[], list("ab"), list("c"), []],                        # empty top-1, non-empty others
        [[], [], []],                                           # all empty
        _nbest(rng, 4, 70, alpha=6, edits=9),                   # top-1 either side of a 64-lane strip
        _nbest(rng, 5, 130, alpha=6, edits=12),
        _nbest(rng, 3, 300, alpha=4, edits=30),                 # more gaps than one block of lanes
        [list("ab"), ins(0), ins(1), ins(65), ins(2)],          # one gap holding 0 / 1 / 65 inserted tokens
        [list("ab"), ins(65), ins(1), ins(0)],
    ]
    return fx, extra


@pytest.fixture(scope="module")
def merged(lists):
    from asr_rescoring_amd import cnet
    fx, extra = lists
    return {m: cnet.merge_nbest(fx + extra, mode=m, slack=4096, sentinel=-77) for m in MODES}


def test_merge_matches_restatement_and_fixture(fixture, lists, merged):
    fx, extra = lists
    for mode in MODES:
        t = merged[mode]
        toks = t.tokens()
        for u, hyps in enumerate(fx + extra):
            want = np.asarray(C.closed_form(hyps, mode), np.int32).reshape(-1, len(hyps))
            got = t.src_of(u)
            assert got.shape == want.shape and (got == want).all(), (mode, u, hyps)
        if mode == C.REFERENCE:
            n = 0
            for u, c in enumerate(fixture["cases"]):
                if c["t"] is not None:
                    assert toks[u] == [list(s) for s in c["t"]], (u, c["h"])
                    n += 1
            assert n > 300
    # N = 1: L1 slots of one column; all empty: no slot
    assert merged[C.EXACT].src_of(len(fx)).tolist() == [[0], [1], [2], [3], [4]]
    assert merged[C.EXACT].n_slots(len(fx) + 1) == 0 and merged[C.EXACT].n_slots(len(fx) + 5) == 0
    assert merged[C.REFERENCE].src.tobytes() != merged[C.EXACT].src.tobytes()


def test_merge_writes_only_its_table_and_repeats(lists, merged):
    from asr_rescoring_amd import cnet
    fx, extra = lists
    for mode in MODES:
        t = merged[mode]
        raw = t._d["src"].cpu().numpy()
        cap = int(t.cell_off[-1])
        assert raw.size == cap + 4096
        assert (raw[cap:] == -77).all() and (raw[:cap] != -77).all()     # every cell written, nothing behind
        k = t._d["K"].cpu().numpy()
        n_gap = sum(len(h[0]) + 1 for h in fx + extra)
        assert (k[n_gap:] == -77).all() and (k[:n_gap] >= 0).all()
        again = cnet.merge_nbest(fx + extra, mode=mode, slack=4096, sentinel=-77)
        assert again._d["src"].cpu().numpy().tobytes() == raw.tobytes()
        assert (again.slot_off == t.slot_off).all()


def test_merge_limits():
    from asr_rescoring_amd import _lib, cnet
    with pytest.raises(ValueError):
        cnet.merge_nbest([[["a"] * 4097, ["a"]]])
    lib = _lib.load()
    assert lib.rs_cn_merge(None, None, None, None, None, None, 1, 4097, None, None, None, None, None, None, 0, 1,
                           None) == -5                                     # RS_EUNSUP
    assert lib.rs_cn_oracle(None, None, None, None, None, None, 1, 1025, None, None, 1, None, None, None, None,
                            None) == -5
    assert lib.rs_cn_vote(None, None, None, None, None, None, 1, 1025, None, None, None, None, None, None,
                          None) == -5


def _check_oracle(table, refs, mode_tables):
    dist, labels = table.oracle(refs)
    for u, (tab, ref) in enumerate(zip(mode_tables, refs)):
        want_d, want_l = C.dp_oracle(tab, ref)
        assert int(dist[u]) == want_d and labels[u].tolist() == want_l, (u, ref)
    return dist, labels


def test_oracle_equals_brute_force(fixture):
    from asr_rescoring_amd import cnet
    cases = C.oracle_cases([[list(h) for h in c["h"]] for c in fixture["cases"][:200]])
    assert len(cases) > 150
    for mode in MODES:
        cs = [c for c in cases if c[1] == mode]
        t = cnet.merge_nbest([c[0] for c in cs], mode=mode)
        dist, labels = t.oracle([c[3] for c in cs])
        assert t.tokens() == [c[2] for c in cs]
        for u, (hyps, _, table, ref) in enumerate(cs):
            assert (int(dist[u]), labels[u].tolist()) == C.brute_oracle(table, ref), (hyps, ref)
        d0, l0 = t.oracle([[] for _ in cs])                                  # empty transcripts
        for u, (_, _, table, _) in enumerate(cs):
            assert (int(d0[u]), l0[u].tolist()) == C.dp_oracle(table, [])
            assert int(d0[u]) == sum(C.GAP not in s for s in table)


def test_oracle_large_lists():
    from asr_rescoring_amd import cnet
    rng = np.random.default_rng(5)
    hyps = [_nbest(rng, 50, int(rng.integers(30, 41)), alpha=40, edits=5) for _ in range(4)]
    hyps.append(_nbest(rng, 6, 130, alpha=8, edits=10))                      # a 130-token transcript
    hyps.append(_nbest(rng, 70, 12, alpha=4, edits=5))                       # more than 64 columns
    refs = [_edited(rng, h[0], 3, 40) for h in hyps]
    refs[4] = list(hyps[4][0])
    for p in (3, 40, 77, 100, 129):
        refs[4][p] = "Z"
    assert len(refs[4]) == 130
    refs[1] = list(hyps[1][7])                                               # the transcript is hypothesis 8
    for mode in MODES:
        t = cnet.merge_nbest(hyps, mode=mode)
        tabs = [C.table_tokens(h, C.closed_form(h, mode)) for h in hyps]
        dist, labels = _check_oracle(t, refs, tabs)
        assert int(dist[1]) == 0
        path = [slot[c] for slot, c in zip(tabs[1], labels[1])]
        assert [x for x in path if x != C.GAP] == refs[1]
        assert int(dist[4]) <= min(C.edit_distance(h, refs[4]) for h in hyps[4])


def _check_vote(hyps_list, mode, weights):
    from asr_rescoring_amd import cnet
    t = cnet.merge_nbest(hyps_list, mode=mode)
    dec, col, share = t.vote(weights)
    out = []
    for u, hyps in enumerate(hyps_list):
        table = C.table_tokens(hyps, C.closed_form(hyps, mode))
        w = None if weights is None else weights[u]
        _, want_col, want_share, want_dec = C.vote(table, w)
        assert dec[u] == want_dec and col[u].tolist() == want_col, (mode, u)
        assert share[u].tobytes() == np.asarray(want_share, np.float64).tobytes(), (mode, u)   # bitwise
        out.append((dec[u], col[u], share[u], table))
    return out


def test_vote_uniform_and_random_weights(fixture):
    rng = np.random.default_rng(9)
    lists_ = [[list(h) for h in c["h"]] for c in fixture["cases"][:120]]
    lists_ += [_nbest(rng, 65, 10, alpha=4), _nbest(rng, 50, 35, alpha=40), [list("abc")]]
    for mode in MODES:
        _check_vote(lists_, mode, None)
        w = []
        for h in lists_:
            x = np.exp(rng.normal(0, 3, len(h)))
            w.append((x / x.sum()).tolist())
        _check_vote(lists_, mode, w)


def test_vote_one_hot_ties_and_gap_winner():
    rng = np.random.default_rng(2)
    hyps = _nbest(rng, 7, 12, alpha=6, edits=5)
    for n in range(7):                                                       # one-hot: that hypothesis
        w = [[1.0 if k == n else 0.0 for k in range(7)]]
        (dec, _, share, _), = _check_vote([hyps], C.EXACT, w)
        assert dec == hyps[n] and (share == 1.0).all()
    # exact mass ties: 0.5 == 0.25 + 0.25, the first column wins
    tie = [list("ab"), list("ac"), list("ac")]
    (dec, col, share, _), = _check_vote([tie], C.EXACT, [[0.5, 0.25, 0.25]])
    assert dec == list("ab") and col.tolist() == [0, 0] and share.tolist() == [1.0, 0.5]
    (dec, col, _, _), = _check_vote([tie], C.EXACT, [[0.25, 0.5, 0.25]])
    assert dec == list("ac") and col.tolist() == [0, 1]
    # a slot whose winner is the gap: one hypothesis inserts a token the others do not have
    gap = [list("ab"), list("ab"), list("axb")]
    (dec, col, share, table), = _check_vote([gap], C.EXACT, None)
    assert table[1] == ["*", "*", "x"] and dec == list("ab") and col.tolist() == [0, 0, 0]
    assert share[1] == 2.0 / 3.0


def test_vote_reference_copy_changes_the_winner(fixture):
    """In reference mode the fold's copies count a token twice; exact mode does not."""
    lists_ = [[list(h) for h in c["h"]] for c in fixture["cases"] if c["t"] is not None]
    ref_out = _check_vote(lists_, C.REFERENCE, None)
    ex_out = _check_vote(lists_, C.EXACT, None)
    assert sum(a[0] != b[0] for a, b in zip(ref_out, ex_out)) > 0


def test_consensus_decode_cer():
    from asr_rescoring_amd import cnet, data as D, rerank
    from oracle import rescore_ref
    nb = D.synthetic_nbest(12, 8, seed=4, vocab=150, len_lo=3, len_hi=14, max_edits=3)
    rng = np.random.default_rng(1)
    lm = rng.normal(-30, 6, nb.n_hyp)
    for mode in MODES:
        for weight in (0.0, 0.37, 1.0):
            cer, dec = rerank.consensus_decode(nb, lm, weight, scale=2.0, mode=mode)
            w = cnet.consensus_weights(nb.am, lm, nb.hyp_len(), nb.utt_off, weight, 2.0)
            want = []
            for u in range(nb.n_utt):
                a, b = int(nb.utt_off[u]), int(nb.utt_off[u + 1])
                hyps = [nb.hyp_words(h).tolist() for h in range(a, b)]
                want.append(C.vote(C.table_tokens(hyps, C.closed_form(hyps, mode)), w[a:b])[3])
            assert [d.tolist() for d in dec] == want
            assert cer == rescore_ref.corpus_cer([list(r) for r in nb.refs], want)
    best_w, best_cer, cers = rerank.find_best_weight_consensus(nb, lm, n_best=8, scale=2.0)
    assert len(cers) == 101 and best_cer == cers.min() and cers[37] == rerank.consensus_decode(nb, lm, float(rerank.weight_grid()[37]), 2.0)[0]


def test_align_features_layout(fixture):
    from asr_rescoring_amd import cnet, data as D
    f = fixture["features"]
    tok = D.CharTokenizer(f["charset"])
    uids = list(f["refs"])
    hyps = [[tok.tokenize(t) for t in f["hyps"][u].values()] for u in uids]
    t = cnet.merge_nbest(hyps, mode="reference")
    dist, labels = t.oracle([tok.tokenize(f["refs"][u]) for u in uids])
    rows = cnet.align_features(t, labels, tok, utt_ids=uids)
    for got, want, u in zip(rows, f["rows"], uids):
        for k in ("utt_id", "input_ids", "attention_masks", "token_type_ids", "prediction_pos"):
            assert got[k] == want[k], (u, k)
        assert len(got["labels"]) == len(want["labels"]) == len(got["prediction_pos"])
        # the reference's own pick (its exhaustive search) reaches the distance the DP reports
        table, ref = t.tokens()[uids.index(u)], tok.tokenize(f["refs"][u])
        path = [slot[c] for slot, c in zip(table, want["labels"])]
        assert C.edit_distance([x for x in path if x != C.GAP], ref) == int(dist[uids.index(u)])
