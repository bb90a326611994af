"""GPU: span-masked PLL (``rs_pll_score_spans``; PLL-word-l2r and PLL-whole-word of Kauf & Ivanova
2023) against the row path that is pinned already (``masked_logprob`` on rows masked on the
host), against the CPU oracle, and against itself with the layer-0 dedup off.

Inputs: "short" — hypotheses of L in SHORT_L word pieces (every T <= 64, so fp16x3 keeps its
layer-0 dedup), "mixed" — the same plus L = 63 (T = 65: the first length past the 16-query
attention kernels) and L = 130 (three key blocks).  Word lengths are seeded in 1..5, with forced
words across the 16-key tile edges (positions 15-17, 31-33, 47-49), a first word of three pieces,
a last word ending at L and one hypothesis that is a single word.
"""
import json
import os

import numpy as np
import pytest
import torch

from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_BASE, BERT_TINY, make_weights

pytestmark = pytest.mark.gpu

REL = 1e-3          # against the fp32 reference (test_gpu_bert.py)
REL_BATCH = 1e-5    # the same rows in another batch composition (test_batch_invariance_and_determinism)
SHORT_L = [1, 2, 14, 15, 16, 17, 18, 31, 33, 46, 47, 62]
MIXED_L = SHORT_L + [63, 130]
ONE_WORD = 4        # index of the hypothesis (L = 16) that is a single word
PRECS = ["fp16", "fp16x3"]
VARIANTS = ["word_l2r", "whole_word"]


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


def _make_set(lengths, seed, vocab=BERT_TINY.vocab):
    rng = np.random.default_rng(seed)
    toks, off, ws = [], [0], []
    for i, L in enumerate(lengths):
        toks += [D.CLS_ID] + rng.integers(D.FIRST_WORD_ID, vocab, size=L).tolist() + [D.SEP_ID]
        w = np.zeros(L + 2, np.uint8)                       # position-indexed: w[p] = 1 where a word begins
        p = 1
        while p <= L:
            w[p] = 1
            p += int(rng.integers(1, 6))
        if L >= 2:
            w[L] = 0                                        # a last word of >= 2 pieces ending at L
            w[L - 1] = 1
        for a, b in ((1, 3), (15, 17), (31, 33), (47, 49)):  # forced words [a, b]
            if b <= L:
                w[a] = 1
                w[a + 1:b + 1] = 0
                if b + 1 <= L:
                    w[b + 1] = 1
        if i == ONE_WORD:
            w[2:L + 1] = 0
        w[0] = w[1] = w[L + 1] = 1
        ws += w.tolist()
        off.append(len(toks))
    return np.asarray(toks, np.int32), np.asarray(off, np.int32), np.asarray(ws, np.uint8)


SETS = {"short": _make_set(SHORT_L, 11), "mixed": _make_set(MIXED_L, 12)}


def _host_rows(tokens, hyp_off, row_off, lo, hi, query, mask_id=D.MASK_ID):
    """The rows masked on the host as a padded batch: (input_ids, attention_mask, labels) int64."""
    R = len(lo)
    hyp = np.repeat(np.arange(len(hyp_off) - 1), np.diff(row_off))
    T = np.diff(hyp_off)[hyp]
    tmax = int(T.max())
    ids = np.zeros((R, tmax), np.int64)
    am = np.zeros((R, tmax), np.int64)
    for r in range(R):
        seg = tokens[hyp_off[hyp[r]]:hyp_off[hyp[r] + 1]]
        ids[r, :T[r]] = seg
        am[r, :T[r]] = 1
    lab = ids.copy()
    for r in range(R):
        ids[r, lo[r]:hi[r]] = mask_id
    return ids, am, lab


@pytest.fixture(scope="module")
def w_tiny():
    return make_weights(BERT_TINY, seed=7, with_cls_linear=True, with_pooler=True)


@pytest.fixture(scope="module")
def scorers(w_tiny):
    """BERT_TINY scorers by (precision, max_rows), made on first use."""
    from asr_rescoring_amd.scorer import PLLScorer
    made = {}

    def get(prec, max_rows):
        if (prec, max_rows) not in made:
            made[(prec, max_rows)] = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=max_rows, precision=prec)
        return made[(prec, max_rows)]
    yield get
    for s in made.values():
        s.close()


_row_ref = {}


def _masked_rows(scorers, prec, max_rows, tokens, hyp_off, spans, key):
    """``masked_logprob`` of the rows masked on the host, computed once per key, on the scorer that
    scores the spans: the rows then fall into the same chunks, and a chunk's longest sequence picks
    its attention kernel.  (Across chunk sizes the fp16 mode moves by ~1e-4 where a chunk of short
    sequences takes the 16-query kernel and the one big chunk the 32-query kernel; rs_pll_score
    does the same)"""
    key = key + (prec, max_rows)
    if key not in _row_ref:
        ids, am, lab = _host_rows(tokens, hyp_off, *spans)
        out = scorers(prec, max_rows).masked_logprob(torch.from_numpy(ids), torch.from_numpy(am), torch.from_numpy(lab),
                                                  spans[3])
        _row_ref[key] = out.cpu().numpy()
    return _row_ref[key]


def _sum_rows(rows, row_off):
    out = np.zeros(len(row_off) - 1, np.float64)
    for h in range(len(out)):
        acc = 0.0
        for r in range(row_off[h], row_off[h + 1]):
            acc += float(rows[r])
        out[h] = acc
    return out


# ---- 1. degenerate spans are rs_pll_score ----------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_rows", [512, 65536])
@pytest.mark.parametrize("name", ["short", "mixed"])
def test_degenerate_spans_are_pll_score(scorers, name, max_rows, prec):
    tokens, off, _ = SETS[name]
    s = scorers(prec, max_rows)
    pll, rows = s.score_nbest(tokens, off, return_rows=True)
    spans = D.pll_spans(off, None, "original")
    pll_s, rows_s = s.score_spans(tokens, off, *spans, return_rows=True)
    assert np.array_equal(rows.cpu().numpy(), rows_s.cpu().numpy())
    assert np.array_equal(pll.cpu().numpy(), pll_s.cpu().numpy())
    # score_nbest's variants route the same way
    ones = np.ones(len(tokens), np.uint8)
    assert np.array_equal(s.score_nbest(tokens, off, variant="whole_word", word_start=ones).cpu().numpy(), pll.cpu().numpy())
    with pytest.raises(ValueError):
        s.score_nbest(tokens, off, variant="word_l2r")


# ---- 2. against masked_logprob on rows masked on the host -------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_rows", [512, 65536])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["short", "mixed"])
def test_spans_match_host_masked_rows(scorers, name, variant, max_rows, prec):
    tokens, off, ws = SETS[name]
    spans = D.pll_spans(off, ws, variant)
    s = scorers(prec, max_rows)
    pll, rows = s.score_nbest(tokens, off, return_rows=True, variant=variant, word_start=ws)
    pll, rows = pll.cpu().numpy(), rows.cpu().numpy()
    ref = _masked_rows(scorers, prec, max_rows, tokens, off, spans, (name, variant))
    err = rel_err(rows, ref).max()
    print(f"{name} {variant} {prec} max_rows={max_rows}: rows vs masked_logprob max rel {err:.3e}")
    assert err < REL_BATCH
    assert np.array_equal(pll, _sum_rows(rows, spans[0]))
    orig = s.score_nbest(tokens, off, return_rows=True)[1].cpu().numpy()
    assert (rows != orig).any()                           # the spans took effect


# ---- 3. against the CPU oracle ---------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_spans_match_oracle(scorers, w_tiny, variant, prec):
    from oracle.bert_ref import TorchBert, masked_logprob_ref
    tokens, off, ws = SETS["mixed"]
    spans = D.pll_spans(off, ws, variant)
    key = ("oracle", variant)
    if key not in _row_ref:
        ids, am, lab = _host_rows(tokens, off, *spans)
        _row_ref[key] = masked_logprob_ref(TorchBert(w_tiny, BERT_TINY), ids, am, lab, spans[3])
    ref = _row_ref[key]
    pll, rows = scorers(prec, 65536).score_spans(tokens, off, *spans, return_rows=True)
    e_row = rel_err(rows.cpu().numpy(), ref).max()
    e_hyp = rel_err(pll.cpu().numpy(), _sum_rows(ref, spans[0])).max()
    print(f"{variant} {prec}: vs oracle max rel rows {e_row:.3e}, hypotheses {e_hyp:.3e}")
    assert e_row < REL and e_hyp < REL


def test_whole_word_bert_base_matches_oracle():
    """H = 768 and the ten middle layers: 2 hypotheses (L = 17, 33), whole_word, fp16x3."""
    from asr_rescoring_amd.scorer import PLLScorer
    from oracle.bert_ref import TorchBert, masked_logprob_ref
    w = make_weights(BERT_BASE, seed=1234)
    tokens, off, ws = _make_set([17, 33], 13, vocab=BERT_BASE.vocab)
    spans = D.pll_spans(off, ws, "whole_word")
    assert (spans[2] - spans[1] > 1).any()
    ids, am, lab = _host_rows(tokens, off, *spans)
    ref = masked_logprob_ref(TorchBert(w, BERT_BASE), ids, am, lab, spans[3])
    s = PLLScorer(w, BERT_BASE, device=0, max_rows=4096, precision="fp16x3")
    try:
        pll, rows = s.score_spans(tokens, off, *spans, return_rows=True)
        pll, rows = pll.cpu().numpy(), rows.cpu().numpy()
    finally:
        s.close()
    e_row, e_hyp = rel_err(rows, ref).max(), rel_err(pll, _sum_rows(ref, spans[0])).max()
    print(f"bert-base whole_word fp16x3: vs oracle max rel rows {e_row:.3e}, hypotheses {e_hyp:.3e}")
    assert e_row < REL and e_hyp < REL


# ---- 4. the dedup is exact and really on -----------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_rows", [512, 65536])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["short", "mixed"])
def test_span_dedup_is_exact(scorers, name, variant, max_rows, prec, monkeypatch):
    tokens, off, ws = SETS[name]
    spans = D.pll_spans(off, ws, variant)
    s = scorers(prec, max_rows)
    out, flops = {}, {}
    for dd in ("1", "0"):
        monkeypatch.setenv("RS_DEDUP", dd)
        s.profile(True)
        pll, rows = s.score_spans(tokens, off, *spans, return_rows=True)
        out[dd] = (pll.cpu().numpy(), rows.cpu().numpy())
        flops[dd] = s.profile_read()["qkv"][2]
        s.profile(False)
    assert np.array_equal(out["1"][1], out["0"][1]) and np.array_equal(out["1"][0], out["0"][0])
    if name == "short" and max_rows == 65536:
        print(f"{variant} {prec}: QKV flops dedup {flops['1']:.4g}, plain {flops['0']:.4g}")
        assert 0 < flops["1"] < flops["0"]               # the plan did not fall back everywhere


# ---- 5. a free plan --------------------------------------------------------------------------

def _free_plan(off):
    """Rows in descending order; a repeated row; the last 5 positions of the L = 33 hypothesis only;
    a span [1, T - 1) scored in its middle; a hypothesis without rows between two scored ones."""
    row_off, lo, hi, q = [0], [], [], []
    for h in range(len(off) - 1):
        T = int(off[h + 1] - off[h])
        L = T - 2
        rows = []
        if L == 14:
            rows = [(p, min(p + 2, T - 1), p) for p in range(L, 0, -1)]
        elif L == 15:
            rows = []                                       # no rows: PLL 0.0
        elif L == 16:
            rows = [(3, 6, 4), (3, 6, 4), (1, 2, 1), (3, 6, 4)]
        elif L == 33:
            rows = [(p, p + 1, p) for p in range(L - 4, L + 1)]
        elif L == 47:
            rows = [(1, T - 1, 24), (1, T - 1, 1), (1, T - 1, T - 2)]
        elif L in (63, 130):
            rows = [(p, min(p + 3, T - 1), p) for p in range(1, L + 1, 7)]
        else:
            rows = [(p, p + 1, p) for p in range(1, L + 1, 2)]
        for a, b, c in rows:
            lo.append(a); hi.append(b); q.append(c)
        row_off.append(len(lo))
    return tuple(np.asarray(x, np.int32) for x in (row_off, lo, hi, q))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_rows", [512, 65536])
def test_free_plan(scorers, max_rows, prec):
    tokens, off, _ = SETS["mixed"]
    spans = _free_plan(off)
    pll, rows = scorers(prec, max_rows).score_spans(tokens, off, *spans, return_rows=True)
    pll, rows = pll.cpu().numpy(), rows.cpu().numpy()
    ref = _masked_rows(scorers, prec, max_rows, tokens, off, spans, ("free",))
    err = rel_err(rows, ref).max()
    print(f"free plan {prec} max_rows={max_rows}: rows vs masked_logprob max rel {err:.3e}")
    assert err < REL_BATCH
    assert np.array_equal(pll, _sum_rows(rows, spans[0]))
    h0 = MIXED_L.index(15)
    assert spans[0][h0] == spans[0][h0 + 1] and pll[h0] == 0.0 and pll[h0 - 1] != 0.0 and pll[h0 + 1] != 0.0
    r16 = spans[0][MIXED_L.index(16)]
    assert rows[r16] == rows[r16 + 1] == rows[r16 + 3]    # the repeated row


# ---- 6. arguments ----------------------------------------------------------------------------

def test_span_arguments(scorers, w_tiny):
    from asr_rescoring_amd import _lib
    from asr_rescoring_amd.scorer import PLLScorer, RescoreBertScorer
    s = scorers("fp16x3", 65536)
    tokens = np.asarray([D.CLS_ID, 200, 201, 202, D.SEP_ID, D.CLS_ID, 203, D.SEP_ID], np.int32)
    off = np.asarray([0, 5, 8], np.int32)
    good = ([0, 2, 3], [1, 2, 1], [3, 4, 2], [2, 3, 1])
    pll, rows = s.score_spans(tokens, off, *good, return_rows=True)
    assert pll.shape == (2,) and rows.shape == (3,) and bool(torch.isfinite(rows).all())
    bad = {"lo = 0": ([0, 1, 1], [0], [2], [1]), "hi = T": ([0, 1, 1], [1], [5], [1]),
           "query < lo": ([0, 1, 1], [2], [4], [1]), "query = hi": ([0, 1, 1], [2], [3], [3]),
           "row_off descending": ([0, 3, 2], [1, 1], [2, 2], [1, 1]),
           "row_off[0] != 0": ([1, 2, 2], [1, 1], [2, 2], [1, 1])}
    for what, (ro, lo, hi, q) in bad.items():
        with pytest.raises(_lib.RescoreError, match="librescore error -1"):     # RS_EARG
            s.score_spans(tokens, off, ro, lo, hi, q)
    with pytest.raises(_lib.RescoreError, match=r"error -1: row 1 \(hypothesis 0"):
        s.score_spans(tokens, off, [0, 2, 2], [1, 1], [3, 5], [2, 3])
    with pytest.raises(_lib.RescoreError, match="librescore error -1"):         # null h_lo
        s.score_spans(tokens, off, good[0], None, good[2], good[3])
    empty = s.score_spans(np.zeros(0, np.int32), [0], [0], [], [], [], return_rows=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0,)
    none = s.score_spans(tokens, off, [0, 0, 0], [], [], [])                    # no rows at all
    assert none.cpu().tolist() == [0.0, 0.0]
    cs = RescoreBertScorer(w_tiny, BERT_TINY, device=0, max_rows=2048)
    try:
        with pytest.raises(_lib.RescoreError, match="librescore error -3"):     # RS_ESTATE
            PLLScorer.score_spans(cs, tokens, off, *good)
    finally:
        cs.close()


# ---- 7. CLI ----------------------------------------------------------------------------------

VOCAB = (["[PAD]"] + [f"[unused{i}]" for i in range(1, 100)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]", "[unused104]", "[unused105]"]
         + list("你好嗎今天") + ["hello", "##llo", "he", "##l", "world", "##s", "play", "##ing", "un", "##able"])
HYPS = {"utt_1": {"hyp_1": "你好 hello worlds", "hyp_2": "你好 hell world"},
        "utt_2": {"hyp_1": "今天 unable playing", "hyp_2": "今天 playing"}}


def test_cli_pll_variant(tmp_path, capsys):
    import yaml
    from asr_rescoring_amd import cli
    from asr_rescoring_amd.frontend import NativeTokenizer
    from asr_rescoring_amd.scorer import PLLScorer
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n", encoding="utf-8")
    json.dump(HYPS, open(tmp_path / "hyps.json", "w", encoding="utf-8"), ensure_ascii=False)
    base = {"task": "scoring", "device": "cuda:0", "random_init_seed": 1234, "max_rows": 4096,
            "train_hyps_text_path": str(tmp_path / "hyps.json")}

    def run(name, extra):
        out = tmp_path / name
        out.mkdir()
        cfg = tmp_path / f"{name}.yaml"
        cfg.write_text(yaml.safe_dump({**base, "output_path": str(out) + "/", **extra}, allow_unicode=True), encoding="utf-8")
        assert cli.main(["mlm_pll", "--config", str(cfg)]) == 0
        lm = json.load(open(out / "train_lm.json", encoding="utf-8"))
        assert {u: list(v) for u, v in lm.items()} == {u: list(v) for u, v in HYPS.items()}
        return np.asarray([x for u in lm for x in lm[u].values()], np.float64)

    model = {"model": {"bert": "bert-base-chinese", "vocab": str(tmp_path / "vocab.txt")}}
    got = run("l2r", {**model, "pll_variant": "word_l2r"})
    capsys.readouterr()
    plain = run("plain", {"pll_variant": "word_l2r"})         # no vocabulary: per-character tokens
    assert "scores are those of pll_variant original" in capsys.readouterr().err

    tok = NativeTokenizer(str(tmp_path / "vocab.txt"))
    tokens, off, _, _, ws = tok.encode_nbest(HYPS, return_word_start=True)
    assert (ws == 0).sum() >= 5
    chars = D.CharTokenizer(sorted({c for h in HYPS.values() for t in h.values() for c in t}))
    nb_char, _ = cli._nbest_tokens(HYPS, chars)
    s = PLLScorer(make_weights(BERT_BASE, seed=1234), BERT_BASE, device=0, max_rows=4096)
    try:
        want = s.score_nbest(tokens, off, variant="word_l2r", word_start=ws).cpu().numpy()
        orig = s.score_nbest(tokens, off).cpu().numpy()
        want_plain = s.score_nbest(nb_char.tokens, nb_char.hyp_off).cpu().numpy()
    finally:
        s.close()
    assert np.array_equal(got, want) and (want != orig).any()
    assert np.array_equal(plain, want_plain)
    with pytest.raises(ValueError):
        run("bad", {**model, "pll_variant": "left"})
    json.dump([], open(tmp_path / "rows.json", "w"))
    with pytest.raises(ValueError, match="needs train_hyps_text_path"):
        run("rows", {**model, "pll_variant": "whole_word", "train_data_path": str(tmp_path / "rows.json")})
