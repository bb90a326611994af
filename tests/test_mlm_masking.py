"""Host side of labelled-row MLM training (train.py): the dynamic-masking collator ``mask_tokens``
(transformers' DataCollatorForLanguageModeling.torch_mask_tokens rule on ragged rows), the label
padding of ``pad_rows`` and the label checks of ``MLMTrainer.step(ignore_index=...)``
(``labelled_rows``).  No GPU.

Statistical bounds: 5 binomial standard deviations, sqrt(p (1 - p) / n), of the share under test."""
import numpy as np
import pytest

from asr_rescoring_amd.train import labelled_rows, mask_tokens, pad_rows
from asr_rescoring_amd.weights import BERT_TINY

S = BERT_TINY


def _rows(seed, n_rows=720, len_lo=20, len_hi=40, pad_share=0.02):
    """[CLS] w.. [SEP] rows, ids in [104, vocab), with a few [PAD] ids among the words."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_rows):
        w = rng.integers(104, S.vocab, int(rng.integers(len_lo, len_hi + 1)))
        w[rng.random(len(w)) < pad_share] = S.pad_id
        rows.append([S.cls_id] + w.tolist() + [S.sep_id])
    return rows


def _eligible(rows):
    return [np.array([0 < p < len(r) - 1 and r[p] != S.pad_id for p in range(len(r))]) for r in rows]


def test_mask_tokens_follows_the_80_10_10_rule():
    rows = _rows(1)
    elig = _eligible(rows)
    n = int(sum(e.sum() for e in elig))
    assert 19000 < n < 23000
    out, lab = mask_tokens(rows, S, 7)
    assert [len(r) for r in out] == [len(r) for r in rows] == [len(r) for r in lab]
    n_sel = n_mask = n_keep = n_rand = 0
    for r, o, l, e in zip(rows, out, lab, elig):
        r, o, l = np.asarray(r), np.asarray(o), np.asarray(l)
        assert ((l == -100) | (l == r)).all()          # a label is -100 or the position's original id
        sel = l != -100                                # the selection, as the labels mark it
        assert not sel[~e].any()                       # never position 0, the last position or a [PAD]
        assert np.array_equal(o[~sel], r[~sel])        # every changed token lies on the selection
        assert ((o >= 0) & (o < S.vocab)).all()
        n_sel += int(sel.sum())
        n_mask += int((o[sel] == S.mask_id).sum())
        n_keep += int((o[sel] == r[sel]).sum())
        n_rand += int(((o[sel] != S.mask_id) & (o[sel] != r[sel])).sum())
    assert n_mask + n_keep + n_rand == n_sel
    sd = lambda p, m: np.sqrt(p * (1 - p) / m)
    assert abs(n_sel / n - 0.15) < 5 * sd(0.15, n), n_sel / n
    assert abs(n_mask / n_sel - 0.8) < 5 * sd(0.8, n_sel), n_mask / n_sel
    # a uniform random id equals the original with probability 1 / vocab and [MASK] likewise: the
    # expected shares move by 0.1 / vocab = 1e-4, far inside the bound (5 sd = 0.027 at n_sel = 3000)
    assert abs(n_rand / n_sel - 0.1) < 5 * sd(0.1, n_sel), n_rand / n_sel
    assert abs(n_keep / n_sel - 0.1) < 5 * sd(0.1, n_sel), n_keep / n_sel
    # seeded: the same seed gives the same output, another seed (int or sequence) another
    assert mask_tokens(rows, S, 7) == (out, lab)
    assert mask_tokens(rows, S, 8)[1] != lab
    a, b = mask_tokens(rows, S, (7, 1)), mask_tokens(rows, S, (7, 2))
    assert a == mask_tokens(rows, S, (7, 1)) and a[1] != b[1] and a[1] != lab


def test_mask_tokens_whole_word_selects_words_wholly():
    rows = _rows(2, n_rows=200, pad_share=0.0)
    rng = np.random.default_rng(3)
    cont = []
    for r in rows:
        c = (rng.random(len(r)) < 0.4).astype(int)
        c[[0, 1, -1]] = 0                              # [CLS], the first word's first piece, [SEP]
        cont.append(c.tolist())
    out, lab = mask_tokens(rows, S, 11, continuation=cont)
    n_words = n_sel_words = n_multi_sel = 0
    for r, l, c in zip(rows, lab, cont):
        sel = np.asarray(l) != -100
        p = 1
        while p < len(r) - 1:
            q = p + 1
            while q < len(r) - 1 and c[q]:
                q += 1
            assert sel[p:q].all() or not sel[p:q].any(), (p, q)
            n_words += 1
            n_sel_words += int(sel[p])
            n_multi_sel += int(sel[p] and q - p > 1)
            p = q
        assert not sel[0] and not sel[-1]
    assert n_multi_sel > 0
    assert abs(n_sel_words / n_words - 0.15) < 5 * np.sqrt(0.15 * 0.85 / n_words)
    # without the flags the same seed selects single positions of some multi-piece word
    _, lab1 = mask_tokens(rows, S, 11)
    split = False
    for l, c in zip(lab1, cont):
        sel = np.asarray(l) != -100
        for p in range(2, len(l) - 1):
            split |= bool(c[p]) and sel[p] != sel[p - 1]
    assert split


def test_mask_tokens_always_returns_a_label():
    """One 3-token row has a single eligible position: selected at every seed (with probability
    0.85 only by the smallest-draw rule)."""
    row = [[S.cls_id, 500, S.sep_id]]
    hit = 0
    for seed in range(40):
        out, lab = mask_tokens(row, S, seed)
        assert lab[0][0] == -100 and lab[0][2] == -100 and lab[0][1] == 500
        assert out[0][0] == S.cls_id and out[0][2] == S.sep_id
        hit += out[0][1] == S.mask_id
    assert hit > 20
    with pytest.raises(ValueError):
        mask_tokens([[S.cls_id, S.sep_id]], S, 0)
    with pytest.raises(ValueError):
        mask_tokens([[S.cls_id, S.pad_id, S.sep_id]], S, 0)


def test_pad_rows_label_pad():
    seqs = [[101, 5, 6, 102], [101, 7, 102], [101, 8, 9, 10, 11, 102]]
    labs = [[-100, 5, -100, -100], [-100, -100, -100], [101, 8, 9, 10, 11, 102]]
    ids, off, lab, klen = pad_rows(seqs, labs, label_pad=-100)
    assert lab.dtype == np.int32 and lab.reshape(3, 6).tolist() == [
        [-100, 5, -100, -100, -100, -100], [-100] * 6, [101, 8, 9, 10, 11, 102]]
    assert ids.reshape(3, 6)[1].tolist() == [101, 7, 102, 0, 0, 0] and klen.tolist() == [4, 3, 6]
    assert off.tolist() == [0, 6, 12, 18]
    # without the keyword: the zero-padded batch as it always was, byte for byte
    T, n = 6, 3
    want_ids, want_lab = np.zeros((n, T), np.int32), np.zeros((n, T), np.int32)
    for i, (x, y) in enumerate(zip(seqs, seqs)):
        want_ids[i, :len(x)] = x
        want_lab[i, :len(y)] = y
    got = pad_rows(seqs, seqs)
    want = (want_ids.ravel(), np.arange(0, n * T + 1, T, dtype=np.int32), want_lab.ravel(),
            np.array([4, 3, 6], np.int32))
    assert len(got) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    types = [[0, 0, 1, 1], [0, 1, 1], [0] * 6]
    got5 = pad_rows(seqs, seqs, types)
    assert len(got5) == 5 and got5[4].reshape(3, 6)[0].tolist() == [0, 0, 1, 1, 0, 0]
    assert pad_rows(seqs, seqs, types, label_pad=-100)[2].reshape(3, 6)[1].tolist() == [101, 7, 102, -100, -100, -100]


def test_labelled_rows_host_checks():
    """The label checks of ``MLMTrainer.step(ignore_index=...)``, reachable without a trainer."""
    rows, ids = labelled_rows([-100, 5, -100, 999, 0, -100], -100, 1000, 6)
    assert rows.dtype == np.int32 and ids.dtype == np.int32
    assert rows.tolist() == [1, 3, 4] and ids.tolist() == [5, 999, 0]
    with pytest.raises(ValueError, match="no labelled position"):
        labelled_rows([-100] * 6, -100, 1000, 6)
    with pytest.raises(ValueError, match="1000"):
        labelled_rows([-100, 1000, 3], -100, 1000, 3)
    with pytest.raises(ValueError, match="-1"):
        labelled_rows([-100, -1, 3], -100, 1000, 3)
    with pytest.raises(ValueError, match="one entry per token"):
        labelled_rows([1, 2, 3], -100, 1000, 4)
    # another ignore value: -100 is then an out-of-range label
    with pytest.raises(ValueError):
        labelled_rows([-1, -100, 3], -1, 1000, 3)
