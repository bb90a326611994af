"""Span plans of the PLL variants (host-only, no GPU): ``data.pll_spans`` against a brute-force
restatement of the three definitions (original: [p, p + 1); word_l2r: [p, end of p's word);
whole_word: the whole word of p — Kauf & Ivanova 2023), and the word boundaries the native
tokenizer reports (``NativeTokenizer.word_starts``: a token begins a word unless its vocabulary
entry is a ``##`` continuation piece) against WordPiece pieces computed here."""
import os

import numpy as np
import pytest

from conftest import REPO  # noqa: F401

from asr_rescoring_amd import data as D


def _brute(hyp_off, ws, variant):
    row_off, lo, hi, q = [0], [], [], []
    for h in range(len(hyp_off) - 1):
        o, T = int(hyp_off[h]), int(hyp_off[h + 1] - hyp_off[h])
        for p in range(1, T - 1):
            b = p
            while b > 1 and not ws[o + b]:
                b -= 1
            e = p + 1
            while e < T - 1 and not ws[o + e]:
                e += 1
            lo.append({"original": p, "word_l2r": p, "whole_word": b}[variant])
            hi.append(p + 1 if variant == "original" else e)
            q.append(p)
        row_off.append(len(q))
    return row_off, lo, hi, q


def _hyps(lengths, rng, max_word, one_word=()):
    """hyp_off and word_start for hypotheses of the given word-piece counts; ``one_word``: indices of
    hypotheses that are a single word."""
    off, ws = [0], []
    for i, L in enumerate(lengths):
        ws.append(1)
        p = 0
        while p < L:
            w = L if i in one_word else int(rng.integers(1, max_word + 1))
            ws += [1] + [0] * (min(w, L - p) - 1)
            p += w
        ws.append(1)
        off.append(len(ws))
    return np.asarray(off, np.int32), np.asarray(ws, np.uint8)


LENGTHS = [1, 510, 2, 3, 7, 1, 16, 33, 64, 5, 510, 12]


@pytest.mark.parametrize("variant", D.PLL_VARIANTS)
@pytest.mark.parametrize("max_word", [1, 4, 9])
def test_pll_spans_match_definitions(variant, max_word):
    rng = np.random.default_rng(100 + max_word)
    off, ws = _hyps(LENGTHS, rng, max_word, one_word=(3, 10))     # L = 3 and L = 510 as one word
    got = D.pll_spans(off, ws, variant)
    want = _brute(off, ws, variant)
    for g, w, name in zip(got, want, ("row_off", "lo", "hi", "query")):
        assert g.dtype == np.int32 and g.tolist() == w, name
    row_off, lo, hi, q = got
    assert row_off.tolist() == np.concatenate([[0], np.cumsum(np.diff(off) - 2)]).tolist()
    T = np.repeat(np.diff(off), np.diff(off) - 2)
    assert ((1 <= lo) & (lo <= q) & (q < hi) & (hi <= T - 1)).all()
    if max_word > 1 and variant != "original":
        assert (hi - lo > 1).any()                                 # real multi-piece words
        one = slice(row_off[3], row_off[4])                        # the single-word hypothesis
        assert (hi[one] == 4).all() and (lo[one] == (1 if variant == "whole_word" else q[one])).all()


def test_all_words_single_token_is_original():
    rng = np.random.default_rng(3)
    off, _ = _hyps(LENGTHS, rng, 1)
    ones = np.ones(int(off[-1]), np.uint8)
    want = D.pll_spans(off, None, "original")
    for variant in D.PLL_VARIANTS:
        got = D.pll_spans(off, ones, variant)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    assert want[1].tolist() == want[3].tolist() and (want[2] == want[1] + 1).all()


def test_pll_spans_arguments():
    off = np.asarray([0, 5], np.int32)
    with pytest.raises(ValueError):
        D.pll_spans(off, None, "word_l2r")
    with pytest.raises(ValueError):
        D.pll_spans(off, np.ones(5, np.uint8), "left_to_right")
    with pytest.raises(ValueError):
        D.pll_spans(off, np.ones(4, np.uint8), "whole_word")
    empty = D.pll_spans(np.asarray([0], np.int32), np.zeros(0, np.uint8), "whole_word")
    assert [len(a) for a in empty] == [1, 0, 0, 0]
    # a hypothesis of [CLS] [SEP] only has no rows
    r = D.pll_spans(np.asarray([0, 2, 6], np.int32), np.asarray([1, 1, 1, 1, 0, 1], np.uint8), "whole_word")
    assert r[0].tolist() == [0, 0, 2] and r[1].tolist() == [1, 1] and r[2].tolist() == [3, 3]


def test_nbest_carries_word_start():
    nb = D.from_lists([[[200, 201, 202], [203]], [[204, 205]]])
    assert nb.word_start is None and nb.subset([1]).word_start is None and nb.slice_utts(0, 1).word_start is None
    nb.word_start = np.asarray([1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 1], np.uint8)
    assert nb.subset([1]).word_start.tolist() == [1, 1, 0, 1]
    assert nb.subset([1, 0]).word_start.tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert nb.slice_utts(1, 2).word_start.tolist() == [1, 1, 0, 1]
    assert nb.slice_utts(0, 1).word_start.tolist() == [1, 1, 0, 1, 1, 1, 1, 1]


# ---- word boundaries from the native tokenizer ----------------------------------------------

CJK = "你好嗎今天天氣很語音識別"
SPECIAL = ["[PAD]"] + [f"[unused{i}]" for i in range(1, 100)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
WORDS = ["hello", "##llo", "he", "##l", "world", "##s", "un", "##able", "play", "##ing", "ab", "##c", "x", "##y",
         "1", "##2", "##3", "3", "##", "#"]
PUNCT = list(",.!?-#") + ["，", "。"]


def _wordpieces(text, vocab):
    """BertTokenizer-style pieces of a lower-case text of ASCII words, CJK and punctuation: split on
    white space, CJK characters and punctuation stand alone, greedy longest-match WordPiece with
    ``##`` continuation pieces, a word with an unmatched rest becomes [UNK]."""
    words, cur = [], ""
    for c in text:
        if c.isspace() or c in CJK or c in PUNCT:
            if cur:
                words.append(cur)
            cur = ""
            if not c.isspace():
                words.append(c)
        else:
            cur += c
    if cur:
        words.append(cur)
    pieces = []
    for w in words:
        sub, start = [], 0
        while start < len(w):
            end = len(w)
            while end > start and (("##" if start else "") + w[start:end]) not in vocab:
                end -= 1
            if end == start:
                sub = ["[UNK]"]
                break
            sub.append(("##" if start else "") + w[start:end])
            start = end
        pieces += sub
    return pieces


def test_word_starts_follow_the_continuation_rule(tmp_path):
    from asr_rescoring_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librescore.so not built")
    from asr_rescoring_amd.frontend import NativeTokenizer
    toks = SPECIAL + sorted(set(CJK)) + WORDS + [p for p in PUNCT if p != "#"]
    path = tmp_path / "vocab.txt"
    path.write_text("\n".join(toks) + "\n", encoding="utf-8")
    vocab = {t: i for i, t in enumerate(toks)}
    nat = NativeTokenizer(str(path))
    texts = ["你好 hello worlds, 123 今天unable playing!", "hellollo zzz abc。語音xy 12-3", "qqq", "helloq 你", "",
             "hell # ab#c 1 2 3，識別"]
    ids, off = nat.encode_batch(texts, add_special=True)
    ws = nat.word_starts(ids)
    assert ws.dtype == np.uint8 and len(ws) == len(ids)
    n_cont = 0
    for i, t in enumerate(texts):
        pieces = ["[CLS]"] + _wordpieces(t, vocab) + ["[SEP]"]
        assert ids[off[i]:off[i + 1]].tolist() == [vocab[p] for p in pieces], (t, pieces)
        want = [0 if p.startswith("##") else 1 for p in pieces]
        assert ws[off[i]:off[i + 1]].tolist() == want, (t, pieces)
        n_cont += want.count(0)
    assert n_cont >= 8 and vocab["[UNK]"] in ids.tolist()
    # ids outside the vocabulary begin a word; the entry "##" itself is a continuation piece
    assert nat.word_starts([-1, len(toks), 1 << 30, vocab["##"], vocab["#"], vocab["##llo"]]).tolist() == [1, 1, 1, 0, 1, 0]
    assert nat.word_starts(np.zeros(0, np.int32)).tolist() == []
    # encode_nbest hands the boundaries out with the tokens
    hyps = {"u1": {"hyp_1": "hello worlds", "hyp_2": "你好 playing"}}
    tk, hoff, uoff, keys, wst = nat.encode_nbest(hyps, return_word_start=True)
    assert np.array_equal(wst, nat.word_starts(tk)) and len(nat.encode_nbest(hyps)) == 4
    spans = D.pll_spans(hoff, wst, "whole_word")
    assert spans[1].tolist() == [1, 2, 2, 1, 2, 3, 3] and spans[2].tolist() == [2, 4, 4, 2, 3, 5, 5]
