"""Host-only: ``data.with_context`` (sentence pairs ``[CLS] context [SEP] hypothesis [SEP]`` with
segment ids), ``data.pll_spans(score_from=...)`` and the ``NBest`` fields that carry both."""
import numpy as np
import pytest

from asr_rescoring_amd import data as D

from test_pll_spans import LENGTHS, _brute, _hyps

C, S = D.CLS_ID, D.SEP_ID


def _nb():
    # utterance 0: two hypotheses, context [300, 301]; utterance 1: one hypothesis, no context;
    # utterance 2: one hypothesis of a single word piece, context [310]
    nb = D.from_lists([[[200, 201, 202], [203]], [[204, 205]], [[206]]])
    ctx = np.asarray([300, 301, 310], np.int32)
    ctx_off = np.asarray([0, 2, 2, 3], np.int32)
    return nb, ctx, ctx_off


def test_with_context_layout_types_and_score_from():
    nb, ctx, ctx_off = _nb()
    tok, off, tt, sf, ws = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, ctx_off)
    assert tok.dtype == np.int32 and off.dtype == np.int32 and tt.dtype == np.uint8 and sf.dtype == np.int32
    assert ws is None
    rows = [tok[off[h]:off[h + 1]].tolist() for h in range(4)]
    assert rows == [[C, 300, 301, S, 200, 201, 202, S], [C, 300, 301, S, 203, S], [C, 204, 205, S], [C, 310, S, 206, S]]
    types = [tt[off[h]:off[h + 1]].tolist() for h in range(4)]
    assert types == [[0, 0, 0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 0, 0], [0, 0, 0, 1, 1]]
    assert sf.tolist() == [4, 4, 1, 3]
    for h in range(4):                                    # score_from points at w_1
        assert rows[h][sf[h]] == nb.hyp_words(h)[0]


def test_with_context_carries_word_start():
    nb, ctx, ctx_off = _nb()
    ws = np.asarray([1, 1, 0, 0, 1,  1, 1, 1,  1, 1, 0, 1,  1, 0, 1], np.uint8)     # 206 flagged 0: still begins a word
    cws = np.asarray([1, 0, 1], np.uint8)
    *_, out = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, ctx_off, word_start=ws, ctx_word_start=cws)
    assert out.dtype == np.uint8
    assert out.tolist() == [1, 1, 0, 1, 1, 0, 0, 1,  1, 1, 0, 1, 1, 1,  1, 1, 0, 1,  1, 1, 1, 1, 1]
    # without ctx_word_start every context token begins a word
    *_, out = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, ctx_off, word_start=ws)
    assert out[:8].tolist() == [1, 1, 1, 1, 1, 0, 0, 1]


def test_empty_context_is_the_input():
    nb, _, _ = _nb()
    ws = np.ones(len(nb.tokens), np.uint8)
    tok, off, tt, sf, out = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, np.zeros(0, np.int32),
                                           np.zeros(nb.n_utt + 1, np.int32), word_start=ws)
    assert np.array_equal(tok, nb.tokens) and np.array_equal(off, nb.hyp_off) and np.array_equal(out, ws)
    assert not tt.any() and (sf == 1).all()
    for variant in D.PLL_VARIANTS:                        # ... and scores every position, as today
        for a, b in zip(D.pll_spans(off, out, variant, score_from=sf), D.pll_spans(nb.hyp_off, ws, variant)):
            assert np.array_equal(a, b)


def test_left_truncation_and_the_hypothesis_that_does_not_fit():
    nb = D.from_lists([[[200, 201, 202, 203]]])
    ctx = np.arange(300, 310, dtype=np.int32)
    off = np.asarray([0, 10], np.int32)
    tok, hoff, tt, sf, _ = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, off, max_len=12)
    assert tok.tolist() == [C, 305, 306, 307, 308, 309, S, 200, 201, 202, 203, S] and len(tok) == 12
    assert tt.tolist() == [0] * 7 + [1] * 5 and sf.tolist() == [7]
    tok, hoff, tt, sf, _ = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, off, max_len=17)   # fits exactly
    assert len(tok) == 17 and tok[1] == 300
    tok, *_ = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, off, max_len=7)     # no room for any context
    assert tok.tolist() == [C, S, 200, 201, 202, 203, S]
    with pytest.raises(ValueError, match="does not fit"):
        D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, off, max_len=6)
    with pytest.raises(ValueError):
        D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, np.asarray([0, 5, 10], np.int32))


@pytest.mark.parametrize("variant", D.PLL_VARIANTS)
def test_score_from_gives_the_tail_of_the_rows(variant):
    rng = np.random.default_rng(5)
    off, ws = _hyps(LENGTHS, rng, 4, one_word=(3,))
    full = D.pll_spans(off, ws, variant)
    L = np.diff(off) - 2
    sf = np.asarray([1 + int(rng.integers(0, l + 1)) for l in L], np.int32)      # 1 .. L + 1 (no rows left)
    sf[0], sf[1] = 1, L[1] + 1
    row_off, lo, hi, q = D.pll_spans(off, ws, variant, score_from=sf)
    assert all(a.dtype == np.int32 for a in (row_off, lo, hi, q))
    assert np.diff(row_off).tolist() == (L - sf + 1).tolist()
    for h in range(len(L)):
        a, b = full[0][h] + sf[h] - 1, full[0][h + 1]
        for got, want in zip((lo, hi, q), full[1:]):
            assert got[row_off[h]:row_off[h + 1]].tolist() == want[a:b].tolist()
    with pytest.raises(ValueError):
        D.pll_spans(off, ws, variant, score_from=sf[:-1])


@pytest.mark.parametrize("variant", D.PLL_VARIANTS)
@pytest.mark.parametrize("max_word", [1, 4, 9])
def test_pll_spans_without_score_from_is_unchanged(variant, max_word):
    """The inputs of test_pll_spans.py: the default output still equals the brute-force definitions."""
    rng = np.random.default_rng(100 + max_word)
    off, ws = _hyps(LENGTHS, rng, max_word, one_word=(3, 10))
    for g, w in zip(D.pll_spans(off, ws, variant), _brute(off, ws, variant)):
        assert g.dtype == np.int32 and g.tolist() == w


def test_nbest_carries_token_type_and_score_from():
    nb, ctx, ctx_off = _nb()
    assert nb.token_type is None and nb.score_from is None
    assert nb.subset([1]).token_type is None and nb.slice_utts(0, 1).score_from is None
    nb.tokens, nb.hyp_off, nb.token_type, nb.score_from, _ = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, ctx_off)
    sub = nb.slice_utts(1, 3)
    assert sub.token_type.tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 1] and sub.score_from.tolist() == [1, 3]
    assert sub.token_type.dtype == np.uint8 and sub.score_from.dtype == np.int32
    sub = nb.subset([2, 0])
    assert sub.token_type.tolist() == [0, 0, 0, 1, 1] + [0, 0, 0, 0, 1, 1, 1, 1] + [0, 0, 0, 0, 1, 1]
    assert sub.score_from.tolist() == [3, 4, 4]


def test_sharded_scoring_slices_types_and_score_from():
    """shard.score_sharded hands the score function a slice that still carries both fields."""
    from asr_rescoring_amd import shard
    nb, ctx, ctx_off = _nb()
    nb.tokens, nb.hyp_off, nb.token_type, nb.score_from, _ = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, ctx_off)
    seen = {}

    def fn(sub):
        seen["tt"], seen["sf"] = sub.token_type, sub.score_from
        return np.zeros(sub.n_hyp)
    shard.score_sharded(nb, fn)
    assert np.array_equal(seen["tt"], nb.token_type) and np.array_equal(seen["sf"], nb.score_from)
