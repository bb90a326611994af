"""GPU: segment ids through the native trainers (``rs_trainer_set_token_types``): the forward reads a
per-row type, the backward sums the embedding gradient into the type table row by row.  Loss,
scores and every gradient against float64 autograd with per-token types (tests/seg_ref.py), at the
tolerances of test_gpu_train.py (loss and scores 1e-4 relative; every gradient within 2e-4 of its
norm, floored at 1e-4 of the global norm); both rows of ``token_type_embeddings.weight`` are also
held to that bound separately."""
import numpy as np
import pytest

from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_TINY, make_weights

import seg_ref

pytestmark = pytest.mark.gpu

NO_DROP = dict(hidden_dropout=0.0, attn_dropout=0.0)
TYPE_KEY = "bert.embeddings.token_type_embeddings.weight"


def _batch(seed, n_utt=3, n_best=4, len_hi=20, ctx_hi=12):
    """test_gpu_train.py's batch, turned into context pairs: contexts of 0..ctx_hi tokens, the first
    utterance's empty."""
    nb = D.synthetic_nbest(n_utt, n_best, seed=seed, vocab=BERT_TINY.vocab, len_lo=1, len_hi=len_hi)
    rng = np.random.default_rng(seed)
    target = rng.normal(-1.0, 1.0, nb.n_hyp).astype(np.float32)
    cer = (rng.integers(0, 5, nb.n_hyp) / 10.0).astype(np.float32)
    clen = rng.integers(1, ctx_hi + 1, n_utt)
    clen[0] = 0
    clen[-1] = ctx_hi
    ctx = rng.integers(D.FIRST_WORD_ID, BERT_TINY.vocab, int(clen.sum())).astype(np.int32)
    tokens, off, types, _, _ = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, np.concatenate([[0], np.cumsum(clen)]))
    assert types.any() and not types[:off[n_best]].any()
    return tokens, off, nb.utt_off, types.astype(np.int32), target, nb.am.astype(np.float32), cer


def _weights(seed=1):
    return make_weights(BERT_TINY, seed=seed, with_cls_linear=True, with_pooler=True)


def _check_grads(tr, ref_grads):
    gnorm = np.sqrt(sum(float(np.sum(ref_grads[k] ** 2)) for k in tr.shapes))
    worst = 0.0
    for k in tr.shapes:
        g, rg = tr.grad(k).astype(np.float64), ref_grads[k].reshape(tr.shapes[k])
        rel = np.linalg.norm(g - rg) / max(np.linalg.norm(rg), 1e-4 * gnorm)
        worst = max(worst, rel)
        assert rel < 2e-4, (k, rel, np.linalg.norm(rg))
    g, rg = tr.grad(TYPE_KEY).astype(np.float64), ref_grads[TYPE_KEY]
    for row in range(g.shape[0]):
        rel = np.linalg.norm(g[row] - rg[row]) / max(np.linalg.norm(rg[row]), 1e-4 * gnorm)
        print(f"token_type row {row}: rel {rel:.3e} (reference norm {np.linalg.norm(rg[row]):.3e})")
        assert np.linalg.norm(rg[row]) > 1e-3 * gnorm       # both rows carry a real gradient
        assert rel < 2e-4, (row, rel)
    print(f"worst gradient rel {worst:.3e}")


def _cls_against_autograd(method, batch, n_best):
    from asr_rescoring_amd.train import RescoreBertTrainer
    w = _weights()
    tokens, off, uoff, types, target, am, cer = batch
    tr = RescoreBertTrainer(w, BERT_TINY, method=method, md_loss_weight=0.5, **NO_DROP)
    try:
        loss, sc = tr.step(tokens, off, uoff, target, am, cer, update=False, token_types=types)
        rloss, rsc, rg = seg_ref.cls_step({k: w[k] for k in tr.shapes}, BERT_TINY, tokens, off, types, target, am, cer,
                                          n_best, method, 0.5, list(tr.shapes))
        print(f"{method}: loss {loss:.6f} vs {rloss:.6f}")
        assert abs(loss - rloss) <= 1e-4 * abs(rloss)
        assert np.abs(sc - rsc).max() <= 1e-4 * np.abs(rsc).max()
        _check_grads(tr, rg)
        # the types took effect: the untyped step is another step
        loss0, _ = tr.step(tokens, off, uoff, target, am, cer, update=False)
        assert abs(loss0 - loss) > 1e-3 * abs(loss)
    finally:
        tr.close()


@pytest.mark.parametrize("method", ["MD", "MD_MWER"])
def test_cls_step_with_types_matches_autograd(method):
    _cls_against_autograd(method, _batch(3), 4)


def test_cls_step_with_types_past_the_one_pass_column_sums():
    """More than 2048 token rows: the predicated type-row sums take tr_colsum's two-stage form."""
    batch = _batch(5, n_utt=12, n_best=16, len_hi=30)
    assert int(batch[1][-1]) > 2048
    _cls_against_autograd("MD_MWER", batch, 16)


def test_ragged_mlm_step_with_types_matches_autograd():
    from asr_rescoring_amd.train import MLMTrainer
    w = make_weights(BERT_TINY, seed=6)
    tokens, off, _, types, *_ = _batch(7)
    rng = np.random.default_rng(8)
    ids = tokens.copy()
    for h in range(len(off) - 1):                       # one [MASK] per row, anywhere but [CLS] and the last [SEP]
        ids[off[h] + int(rng.integers(1, off[h + 1] - off[h] - 1))] = D.MASK_ID
    tr = MLMTrainer(w, BERT_TINY, lr=1e-3, **NO_DROP)
    try:
        loss = tr.step(ids, off, tokens, update=False, token_types=types)
        rloss, rg = seg_ref.mlm_step({k: w[k] for k in tr.shapes}, BERT_TINY, ids, off, types, tokens, list(tr.shapes))
        print(f"MLM: loss {loss:.6f} vs {rloss:.6f}")
        assert abs(loss - rloss) <= 1e-4 * abs(rloss)
        _check_grads(tr, rg)
        with pytest.raises(ValueError):
            tr.step(ids, off, tokens, update=False, token_types=types[:-1])
        with pytest.raises(ValueError):
            tr.step(ids, off, tokens, update=False, token_types=types + 1)
    finally:
        tr.close()


def test_zero_types_are_the_untyped_step_and_typed_steps_repeat():
    from asr_rescoring_amd import _lib
    from asr_rescoring_amd.train import RescoreBertTrainer
    w = _weights(4)
    tokens, off, uoff, types, target, am, cer = _batch(9)
    tr = RescoreBertTrainer(w, BERT_TINY, method="MD_MWER", md_loss_weight=0.5, **NO_DROP)

    def step(tt=None):
        loss, sc = tr.step(tokens, off, uoff, target, am, cer, update=False, token_types=tt)
        return loss, sc, {k: tr.grad(k) for k in tr.shapes}

    def same(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    try:
        plain = step()
        assert not plain[2][TYPE_KEY][1].any() and plain[2][TYPE_KEY][0].any()
        zero = step(np.zeros_like(types))
        assert same(plain, zero) and not zero[2][TYPE_KEY][1].any()
        typed = step(types)
        assert not same(typed, plain) and typed[2][TYPE_KEY][1].any()
        assert same(step(), plain)                         # one-shot: the next step is untyped again
        assert same(step(types), typed)                    # bitwise reproducible
        # a count that does not match fails the step (RS_EARG) and is dropped with it
        d_type = tr._set_types(types, len(types))          # noqa: F841
        with pytest.raises(_lib.RescoreError, match=r"error -1: rs_trainer_set_token_types gave \d+ token types"):
            tr.step(tokens[:off[4]], off[:5], uoff[:2], target[:4], am[:4], cer[:4], update=False)
        assert same(step(), plain)
    finally:
        tr.close()
