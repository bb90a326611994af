"""GPU: the native trainers on sequences of more than 128 tokens (the tiled attention kernels of
k_train.hip), against torch autograd (oracle/train_ref.py) with the metric and the numbers of
tests/test_gpu_train.py: loss and scores within 1e-4 relative, every gradient tensor within 2e-4
of its norm, floored at 1e-4 of the global norm.  On the CPU, torch fp32 against torch fp64
autograd sits at 2.7e-5 by that metric on the RescoreBert batch below (worst tensor:
layer.1.attention.self.key.bias, whose true gradient is zero) and at 2.3e-6 on the MLM batch.
"""
import os

import numpy as np
import pytest
import torch

from asr_rescoring_amd import _lib
from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_TINY, make_weights

pytestmark = pytest.mark.gpu

NO_DROP = dict(hidden_dropout=0.0, attn_dropout=0.0)
LONG = [512, 385, 257, 129, 130, 64, 3, 200]


def _weights(seed=1):
    return make_weights(BERT_TINY, seed=seed, with_cls_linear=True, with_pooler=True)


def _rows(lengths, seed):
    """Ragged token rows of the given lengths (ids 1 .. vocab - 1: no [PAD]) with the per-hypothesis
    targets, AM scores and error rates of a RescoreBert batch."""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, BERT_TINY.vocab, t).tolist() for t in lengths]
    tokens = np.concatenate([np.asarray(s, np.int32) for s in seqs])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = len(lengths)
    target = rng.normal(-1.0, 1.0, n).astype(np.float32)
    am = rng.normal(-3.0, 1.0, n).astype(np.float32)
    cer = (rng.integers(0, 5, n) / 10.0).astype(np.float32)
    return seqs, tokens, off, target, am, cer


def _check_grads(tr, ref_grad):
    gnorm = np.sqrt(sum(float(np.sum(ref_grad(k).astype(np.float64) ** 2)) for k in tr.shapes))
    worst = (0.0, None)
    for k in tr.shapes:
        g, rg = tr.grad(k), ref_grad(k)
        rel = np.linalg.norm(g - rg) / max(np.linalg.norm(rg), 1e-4 * gnorm)
        worst = max(worst, (rel, k))
    print(f"TRAIN-LONG worst gradient: {worst[0]:.2e} {worst[1]}")
    assert worst[0] < 2e-4, worst


class _attn_mode:
    """RS_TRAIN_ATTN for the trainers created inside the block."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("RS_TRAIN_ATTN")
        os.environ["RS_TRAIN_ATTN"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("RS_TRAIN_ATTN", None)
        else:
            os.environ["RS_TRAIN_ATTN"] = self.old


def test_rescorebert_step_on_sequences_up_to_512_tokens():
    from asr_rescoring_amd.train import RescoreBertTrainer
    from oracle.train_ref import TorchTrainer
    w = _weights()
    seqs, tokens, off, target, am, cer = _rows(LONG, 3)
    utt = np.array([0, 4, 8], np.int32)
    tr = RescoreBertTrainer(w, BERT_TINY, method="MD_MWER", md_loss_weight=0.5, **NO_DROP)
    ref = TorchTrainer(w, BERT_TINY)
    try:
        loss, sc = tr.step(tokens, off, utt, target, am, cer, update=False)
        rloss, rsc = ref.step(seqs, target, am, cer, n_best=4, method="MD_MWER", md_loss_weight=0.5, update=False)
        assert abs(loss - rloss) <= 1e-4 * abs(rloss), (loss, rloss)
        assert np.abs(sc - rsc).max() <= 1e-4 * np.abs(rsc).max()
        _check_grads(tr, ref.grad)
    finally:
        tr.close()


def test_mlm_step_on_padded_rows_of_300_tokens():
    """Rows of 300, 140, 20, 257, 129 tokens padded to 300: key lengths below the row length on
    the tiled kernels (pads are queries, never keys)."""
    from asr_rescoring_amd.train import MLMTrainer, pad_rows
    from oracle.train_ref import TorchTrainer
    w = make_weights(BERT_TINY, seed=6)
    rng = np.random.default_rng(8)
    rows = [rng.integers(1, BERT_TINY.vocab, t).tolist() for t in [300, 140, 20, 257, 129]]
    labs = [rng.integers(1, BERT_TINY.vocab, len(r)).tolist() for r in rows]
    tr = MLMTrainer(w, BERT_TINY, lr=1e-3, **NO_DROP)
    ref = TorchTrainer(w, BERT_TINY, lr=1e-3, head="mlm")
    try:
        ids, poff, plab, klen = pad_rows(rows, labs)
        assert int(poff[1] - poff[0]) == 300 and klen.tolist() == [300, 140, 20, 257, 129]
        l = tr.step(ids, poff, plab, klen, update=False)
        rl = ref.step_mlm(rows, labs, update=False)
        assert abs(l - rl) <= 1e-4 * abs(rl), (l, rl)
        _check_grads(tr, lambda k: ref.model.w[k].grad.numpy())
    finally:
        tr.close()


def test_long_adamw_steps_are_deterministic_and_feed_the_scorer():
    from asr_rescoring_amd.scorer import RescoreBertScorer
    from asr_rescoring_amd.train import RescoreBertTrainer
    w = _weights(4)
    nb = D.synthetic_nbest(2, 3, vocab=BERT_TINY.vocab, len_lo=127, len_hi=510)
    lens = np.diff(nb.hyp_off)
    assert 128 < lens.max() <= 512
    rng = np.random.default_rng(21)
    target = rng.normal(-1.0, 1.0, nb.n_hyp).astype(np.float32)
    out = []
    for _ in range(2):
        tr = RescoreBertTrainer(w, BERT_TINY, method="MD", lr=5e-4, **NO_DROP)
        try:
            for _step in range(2):
                tr.step(nb.tokens, nb.hyp_off, nb.utt_off, target)
            _, sc = tr.step(nb.tokens, nb.hyp_off, nb.utt_off, target, update=False)
            out.append((tr.state_dict(), sc))
        finally:
            tr.close()
    (sd, sc), (sd2, sc2) = out
    assert all(np.array_equal(sd[k], sd2[k]) for k in sd) and np.array_equal(sc, sc2)
    scorer = RescoreBertScorer(sd, BERT_TINY, device=0, precision="fp16x3")
    try:
        got = scorer.score_nbest(nb.tokens, nb.hyp_off).cpu().numpy()
    finally:
        scorer.close()
    assert (np.abs(got - sc) <= 1e-4 * np.maximum(1.0, np.abs(sc))).all(), (got, sc)


def test_long_dropout_step_matches_oracle_fed_the_same_masks():
    """Attention and hidden dropout at p = 0.1 on a 300- and a 150-token sequence: the trainer's
    masks through padded_drop into the oracle; loss and gradients at the p = 0 tolerances."""
    from asr_rescoring_amd.train import RescoreBertTrainer, dropout_keep
    from oracle.train_ref import TorchTrainer, padded_drop
    S = BERT_TINY
    w = _weights(11)
    seqs, tokens, off, target, am, cer = _rows([300, 150], 9)
    utt = np.array([0, 2], np.int32)
    tr = RescoreBertTrainer(w, S, method="MD_MWER", md_loss_weight=0.5, lr=1e-3, dropout_seed=4321)
    ref = TorchTrainer(w, S, lr=1e-3)
    try:
        key = tr.dropout_step()
        loss, sc = tr.step(tokens, off, utt, target, am, cer, update=False)
        keep = lambda site, n: dropout_keep(4321, key, site, 0.1, n)
        drop = padded_drop(keep, [300, 150], S.hidden, S.heads, S.layers, 0.1, 0.1)
        rloss, rsc = ref.step(seqs, target, am, cer, n_best=2, method="MD_MWER", md_loss_weight=0.5, update=False,
                              drop=drop)
        assert abs(loss - rloss) <= 1e-4 * abs(rloss), (loss, rloss)
        assert np.abs(sc - rsc).max() <= 1e-4 * np.abs(rsc).max()
        _check_grads(tr, ref.grad)
    finally:
        tr.close()


def test_tiled_attention_on_a_short_batch():
    """RS_TRAIN_ATTN=tiled on the small batch of test_gradients_match_autograd (all T <= 22)."""
    from asr_rescoring_amd.train import RescoreBertTrainer
    from oracle.train_ref import TorchTrainer
    w = _weights()
    nb = D.synthetic_nbest(3, 4, seed=3, vocab=BERT_TINY.vocab, len_lo=1, len_hi=20)
    rng = np.random.default_rng(3)
    target = rng.normal(-1.0, 1.0, nb.n_hyp).astype(np.float32)
    cer = (rng.integers(0, 5, nb.n_hyp) / 10.0).astype(np.float32)
    am = nb.am.astype(np.float32)
    seqs = [nb.tokens[nb.hyp_off[h]:nb.hyp_off[h + 1]].tolist() for h in range(nb.n_hyp)]
    assert np.diff(nb.hyp_off).max() <= 22
    with _attn_mode("tiled"):
        tr = RescoreBertTrainer(w, BERT_TINY, method="MD_MWER", md_loss_weight=0.5, **NO_DROP)
    ref = TorchTrainer(w, BERT_TINY)
    try:
        loss, sc = tr.step(nb.tokens, nb.hyp_off, nb.utt_off, target, am, cer, update=False)
        rloss, rsc = ref.step(seqs, target, am, cer, n_best=4, method="MD_MWER", md_loss_weight=0.5, update=False)
        assert abs(loss - rloss) <= 1e-4 * abs(rloss)
        assert np.abs(sc - rsc).max() <= 1e-4 * np.abs(rsc).max()
        _check_grads(tr, ref.grad)
    finally:
        tr.close()


def test_legacy_attention_refuses_129_tokens():
    from asr_rescoring_amd.train import RescoreBertTrainer
    w = _weights()
    _, tokens, off, target, am, cer = _rows([129, 5], 2)
    with _attn_mode("legacy"):
        tr = RescoreBertTrainer(w, BERT_TINY, method="MD", **NO_DROP)
    try:
        with pytest.raises(_lib.RescoreError, match="error -5"):
            tr.step(tokens, off, np.array([0, 2], np.int32), target, am, cer, update=False)
        # the short rows still train
        tr.step(tokens[129:], np.array([0, 5], np.int32), np.array([0, 1], np.int32), target[1:], update=False)
    finally:
        tr.close()


def test_sequence_longer_than_max_pos_is_refused():
    from asr_rescoring_amd.train import RescoreBertTrainer
    w = _weights()
    _, tokens, off, target, am, cer = _rows([BERT_TINY.max_pos + 1, 4], 2)
    tr = RescoreBertTrainer(w, BERT_TINY, method="MD", **NO_DROP)
    try:
        with pytest.raises(_lib.RescoreError, match="error -5"):
            tr.step(tokens, off, np.array([0, 2], np.int32), target, am, cer, update=False)
    finally:
        tr.close()
