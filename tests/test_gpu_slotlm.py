"""LM-weighted consensus decode (rerank.consensus_decode_lm, cnet.slot_lm_vote, cli consensus_lm) on a
tiny BERT: 6 synthetic utterances x N = 5 over a 30-symbol alphabet, one utterance with N = 1 and one whose
top-1 is a single token.  The rule is checked exactly: the decode must equal the CPU restatement
(tests/slotlm_ref.py) fed with the log-probs the GPU call itself returned; the log-probs are covered by
tests/test_gpu_cands.py."""
import json

import numpy as np
import pytest
import yaml

from asr_rescoring_amd import cnet, rerank
from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_TINY, make_weights
import cnet_ref as C
import slotlm_ref as S

pytestmark = pytest.mark.gpu

ALPHA = list(range(106, 136))                      # 30 symbols of the scorer's vocabulary
WEIGHT, SCALE = 0.4, 2.0


def _nbest(seed=2):
    """6 utterances: N = 5 hypotheses (edits of a base string), utterance 2 with N = 1, utterance 4 with a
    one-token top-1; AM scores descending, the transcript the unedited base."""
    rng = np.random.default_rng(seed)
    hyps, am, refs = [], [], []
    for u in range(6):
        base = rng.choice(ALPHA, size=1 if u == 4 else int(rng.integers(6, 12))).tolist()
        utt = []
        for k in range(1 if u == 2 else 5):
            w = list(base)
            for _ in range(int(rng.integers(1, 4))):
                op, i = int(rng.integers(0, 3)), int(rng.integers(0, len(w) + 1))
                if op == 0 and w:
                    w[min(i, len(w) - 1)] = int(rng.choice(ALPHA))
                elif op == 1:
                    w.insert(i, int(rng.choice(ALPHA)))
                elif len(w) > 1:
                    del w[min(i, len(w) - 1)]
            utt.append(w if u != 4 or k else list(base))
        hyps.append(utt)
        am.append(sorted((-rng.uniform(1, 9, size=len(utt))).tolist(), reverse=True))
        refs.append(base)
    nb = D.from_lists(hyps, am, refs)
    lm = -rng.uniform(5, 40, size=nb.n_hyp)
    return nb, lm, hyps


@pytest.fixture(scope="module")
def scorer():
    from asr_rescoring_amd.scorer import PLLScorer
    s = PLLScorer(make_weights(BERT_TINY, seed=7), BERT_TINY, device=0, max_rows=2048)
    yield s
    s.close()


@pytest.fixture(scope="module")
def setup(scorer):
    nb, lm, hyps = _nbest()
    tables = [C.table_tokens(h, C.closed_form(h, C.EXACT)) for h in hyps]
    w = cnet.consensus_weights(nb.am, lm, nb.hyp_len(), nb.utt_off, WEIGHT, SCALE)
    weights = [w[a:b].tolist() for a, b in zip(nb.utt_off[:-1], nb.utt_off[1:])]
    assert len(hyps[2]) == 1 and len(hyps[4][0]) == 1
    return nb, lm, hyps, tables, weights


def _cer(decodes, refs):
    return sum(C.edit_distance(list(d), list(r)) for d, r in zip(decodes, refs)) / sum(len(r) for r in refs)


def test_lam_zero_is_the_consensus_decode(scorer, setup):
    nb, lm = setup[:2]
    cer0, dec0 = rerank.consensus_decode(nb, lm, WEIGHT, SCALE)
    cer, dec, info = rerank.consensus_decode_lm(nb, lm, scorer, WEIGHT, 0.0, SCALE, return_info=True)
    assert cer == cer0 and [d.tolist() for d in dec] == [d.tolist() for d in dec0]
    assert info["n_forwards"] == 0


@pytest.mark.parametrize("lam", [0.3, 1.0])
def test_decode_equals_the_restatement_on_the_returned_logprobs(scorer, setup, lam):
    nb, lm, hyps, tables, weights = setup
    cer, dec, info = rerank.consensus_decode_lm(nb, lm, scorer, WEIGHT, lam, SCALE, return_info=True)
    contested = [(u, s) for u, t in enumerate(tables) for s, *_ in S.position_candidates(t)]
    assert info["n_forwards"] == info["n_contested"] == len(contested) > 10
    assert sorted(info["slot_lp"]) == contested
    assert not any(u in (2, 4) and len(tables[u]) == 1 for u, _ in contested)
    want, changed = [], 0
    for u, t in enumerate(tables):
        lp = {s: [float(x) for x in v] for (uu, s), v in info["slot_lp"].items() if uu == u}
        for s, v in lp.items():
            assert all(np.isfinite(v)) and max(v) < 0.0
        want.append(S.slot_lm_vote(t, weights[u], lp, lam)[3])
        changed += want[-1] != C.vote(t, weights[u])[3]
    assert [d.tolist() for d in dec] == want
    assert cer == _cer(want, nb.refs)
    print(f"SLOTLM lam {lam}: {len(contested)} contested positions, {changed} of 6 decodes differ from the plain vote, "
          f"CER {cer:.4f}")


@pytest.mark.parametrize("lam", [0.3, 1.0])
def test_slot_lm_vote_on_a_device_table_agrees_slot_by_slot(scorer, setup, lam):
    nb, lm, hyps, tables, weights = setup
    table = cnet.merge_nbest(hyps, "exact", 0)
    assert table.position_candidates() == \
        [(u, s, g, toks, cols) for u, t in enumerate(tables) for s, g, toks, cols in S.position_candidates(t)]
    rng = np.random.default_rng(1)
    slot_lp = {(u, s): (-rng.uniform(0, 12, size=len(toks))).tolist() for u, s, _, toks, _ in table.position_candidates()}
    dec, cols, shares = cnet.slot_lm_vote(table, weights, slot_lp, lam)
    for u, t in enumerate(tables):
        _, col, share, want = S.slot_lm_vote(t, weights[u], {s: v for (uu, s), v in slot_lp.items() if uu == u}, lam)
        assert dec[u] == want and list(cols[u]) == col
        np.testing.assert_allclose(shares[u], share, rtol=1e-12, atol=0)


def test_lam_sweep_reuses_one_set_of_forwards(scorer, setup, monkeypatch):
    nb, lm = setup[:2]
    calls = []
    real = type(scorer).score_cands
    monkeypatch.setattr(type(scorer), "score_cands", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    grid = (0.0, 0.3, 1.0)
    best, best_cer, cers = rerank.find_best_weight_consensus_lm(nb, lm, scorer, WEIGHT, grid, SCALE)
    assert len(calls) == 1 and len(cers) == 3 and best in grid and best_cer == cers.min()
    for lam, c in zip(grid, cers):
        assert c == rerank.consensus_decode_lm(nb, lm, scorer, WEIGHT, lam, SCALE)[0]


def test_cli_consensus_lm(tmp_path, monkeypatch):
    """Three utterances through the command (BERT-base shape, seeded weights, the per-character tokenizer):
    its JSON holds the numbers the API gives on the same inputs (with the command's own scorer, kept open)."""
    from asr_rescoring_amd import cli
    from asr_rescoring_amd.scorer import PLLScorer
    hyps = {"u1": {"h1": "abcdef", "h2": "abxdef", "h3": "abcdf", "h4": "abcdefg"},
            "u2": {"h1": "hello", "h2": "hallo", "h3": "helo"},
            "u3": {"h1": "kmn", "h2": "kmn", "h3": "kn"}}
    refs = {"u1": "abcdef", "u2": "hallo", "u3": "kmn"}
    rng = np.random.default_rng(4)
    am = {u: {h: -float(i) - 1.0 for i, h in enumerate(hs)} for u, hs in hyps.items()}
    lm = {u: {h: -float(rng.uniform(3, 20)) for h in hs} for u, hs in hyps.items()}
    for name, obj in (("hyps", hyps), ("refs", refs), ("am", am), ("lm", lm)):
        json.dump(obj, open(tmp_path / f"{name}.json", "w", encoding="utf-8"))
    paths = {f"{s}_{k}_path": str(tmp_path / f"{f}.json") for s in ("dev", "test")
             for k, f in (("am", "am"), ("hyps_text", "hyps"), ("ref_text", "refs"), ("lm", "lm"))}
    cfg = tmp_path / "consensus_lm.yaml"
    grid = [0.5, 1.0]
    cfg.write_text(yaml.safe_dump({**paths, "n_best": 4, "device": "cuda:0", "random_init_seed": 1234, "max_rows": 4096,
                                   "consensus_weight": 0.5, "consensus_scale": 2.0, "slot_lm_grid": grid,
                                   "output_path": str(tmp_path / "out")}), encoding="utf-8")
    made, init, close = [], PLLScorer.__init__, PLLScorer.close
    monkeypatch.setattr(PLLScorer, "__init__", lambda self, *a, **k: made.append(self) or init(self, *a, **k))
    monkeypatch.setattr(PLLScorer, "close", lambda self: None)
    try:
        assert cli.main(["consensus_lm", "--config", str(cfg)]) == 0
        res = json.load(open(tmp_path / "out" / "consensus_lm.json", encoding="utf-8"))
        log = (tmp_path / "out" / "consensus_lm.log").read_text()
        assert "slot_lm_weight: " in log and "test_cer: " in log and len(made) == 1
        # the same inputs through the API
        tok = D.CharTokenizer(sorted({c for h in hyps.values() for t in h.values() for c in t} | set("".join(refs.values()))))
        nb = D.from_lists([[tok.encode_words(t) for t in h.values()] for h in hyps.values()],
                          [list(a.values()) for a in am.values()], [tok.encode_words(r) for r in refs.values()], list(hyps))
        lmv = np.asarray([v for u in lm.values() for v in u.values()], np.float64)
        lam, cer, cers = rerank.find_best_weight_consensus_lm(nb, lmv, made[0], 0.5, grid, 2.0, 4)
        _, _, info = rerank.consensus_decode_lm(nb, lmv, made[0], 0.5, lam, 2.0, 4, return_info=True)
    finally:
        for s in made:
            close(s)
    assert res["weight"] == 0.5 and res["slot_lm_weight"] == lam and lam in grid
    assert res["dev_cer"] == cer == res["test_cer"]                  # dev and test are the same files
    assert res["consensus_test_cer"] == rerank.consensus_decode(nb, lmv, 0.5, 2.0, 4)[0] == res["consensus_dev_cer"]
    tables = [C.table_tokens(h, C.closed_form(h, C.EXACT)) for h in ([list(t) for t in u.values()] for u in hyps.values())]
    assert res["test_contested"] == info["n_contested"] == sum(len(S.position_candidates(t)) for t in tables) == 2
    assert res["test_forwards"] == info["n_forwards"] == 2
