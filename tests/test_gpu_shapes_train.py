"""GPU: the native trainers (train_api.hip, k_train.hip) at the encoder shapes of tests/shape_matrix.py
that the other trainer tests never run (they fix H = 256, HEADS = 4, F = 1024): h512 and h1024 (8 and 16
heads, the NV dispatch of k_train.hip, the sgemm picker at N, K of 512 .. 4096), f640, l1 (one layer) and
t1000 (intermediate 1000: % 4 only, the float4 pointwise kernels' and the sgemm edges' granularity).

References and tolerances are those of tests/test_gpu_train.py, unchanged: oracle.train_ref.TorchTrainer
(torch autograd + torch.optim.AdamW); loss and scores within 1e-4 relative, every tensor's gradient
within 2e-4 of its norm (floored at 1e-4 of the global norm); one AdamW update by the rule of
train_fixtures.check_updates: the update's L2 norm and its dot with a seeded probe within 2e-2 of the
reference update's norm, tensors of at most 1024 elements elementwise within 2e-2 of that norm,
attention.self.key.bias skipped (its gradient is exactly zero in exact arithmetic).

Batch: data.synthetic_nbest(3, 6, seed=3, vocab, len_lo=1, len_hi=40).  The MLM rows are its 18
hypotheses with one position masked each, plus one row of T = 72 and one of T = 3, padded like the
reference's collate.

Measured on MI355X (SHAPES lines): loss <= 2.2e-7 and scores <= 1.2e-6 relative; worst gradient 1.8e-6 ..
8.2e-6 of its norm (always an attention.self.key.bias, held at the floor); worst update 2.0e-4 .. 4.7e-3
(CLS) and 1.1e-4 .. 1.6e-2 (MLM; h512's last-layer value bias, elements with |g| near AdamW's eps).
"""
import numpy as np
import pytest

import shape_matrix as SM

pytestmark = pytest.mark.gpu

NO_DROP = dict(hidden_dropout=0.0, attn_dropout=0.0)
LR = 1e-3


def _check_grads(sid, what, tr, ref_grad):
    gnorm = np.sqrt(sum(float(np.sum(ref_grad(k).astype(np.float64) ** 2)) for k in tr.shapes))
    worst = ("", 0.0)
    for k in tr.shapes:
        g, rg = tr.grad(k), ref_grad(k)
        rel = np.linalg.norm(g - rg) / max(np.linalg.norm(rg), 1e-4 * gnorm)
        worst = max(worst, (k, rel), key=lambda t: t[1])
        assert rel < 2e-4, (k, rel, np.linalg.norm(rg))
    print(f"SHAPES {sid} train {what}: worst gradient {worst[1]:.3e} ({worst[0]}) global norm {gnorm:.3e}")


def _check_update(sid, what, before, after, ref_after, rel=2e-2):
    """train_fixtures.check_updates' rule with the reference update at hand instead of its sketch."""
    worst = ("", 0.0)
    for i, k in enumerate(sorted(before)):
        if k.endswith("attention.self.key.bias"):
            continue
        d = (after[k].astype(np.float64) - before[k].astype(np.float64)).ravel()
        rd = (ref_after[k].astype(np.float64) - before[k].astype(np.float64)).ravel()
        r = np.random.Generator(np.random.PCG64(1000 + i)).standard_normal(d.size)
        nrm = max(np.linalg.norm(rd), 1e-12)
        e = max(abs(np.linalg.norm(d) - np.linalg.norm(rd)), abs(float(d @ r) - float(rd @ r))) / nrm
        if d.size <= 1024:
            e = max(e, float(np.abs(d - rd).max()) / nrm)
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= rel, (k, e)
    print(f"SHAPES {sid} train {what}: worst update {worst[1]:.3e} ({worst[0]})")


@pytest.mark.parametrize("sid", SM.TRAINER_IDS)
def test_rescorebert_step_and_update(sid):
    """One MD_MWER step (update=False) against torch autograd with test_gradients_match_autograd's
    assertions, then one AdamW update on both sides."""
    from asr_rescoring_amd.train import RescoreBertTrainer
    from oracle.bert_ref import set_cpu_threads
    from oracle.train_ref import TorchTrainer
    set_cpu_threads()
    shape, w = SM.SHAPES[sid], SM.weights(sid)
    nb, seqs, target, am, cer = SM.train_inputs(sid)
    tr = RescoreBertTrainer(w, shape, method="MD_MWER", md_loss_weight=0.5, lr=LR, **NO_DROP)
    ref = TorchTrainer(w, shape, lr=LR)
    try:
        loss, sc = tr.step(nb.tokens, nb.hyp_off, nb.utt_off, target, am, cer, update=False)
        rloss, rsc = ref.step(seqs, target, am, cer, n_best=6, method="MD_MWER", md_loss_weight=0.5, update=False)
        print(f"SHAPES {sid} train cls: loss rel {abs(loss - rloss) / abs(rloss):.3e} "
              f"scores {np.abs(sc - rsc).max() / np.abs(rsc).max():.3e}")
        assert abs(loss - rloss) <= 1e-4 * abs(rloss)
        assert np.abs(sc - rsc).max() <= 1e-4 * np.abs(rsc).max()
        _check_grads(sid, "cls", tr, ref.grad)
        # the loss-only pass (the reference's dev loss) gives the same loss and scores
        l2, sc2 = tr.step(nb.tokens, nb.hyp_off, nb.utt_off, target, am, cer, update="loss")
        assert l2 == loss and np.array_equal(sc2, sc)
        before = {k: tr.tensor(k) for k in tr.shapes}
        assert all(np.array_equal(before[k], np.asarray(w[k], np.float32).reshape(tr.shapes[k])) for k in before)
        tr.step(nb.tokens, nb.hyp_off, nb.utt_off, target, am, cer, update=True)
        ref.step(seqs, target, am, cer, n_best=6, method="MD_MWER", md_loss_weight=0.5, update=True)
        _check_update(sid, "cls", before, {k: tr.tensor(k) for k in tr.shapes},
                      {k: ref.tensor(k).reshape(tr.shapes[k]) for k in tr.shapes})
    finally:
        tr.close()


def _mlm_rows(sid):
    """(rows, labels): every hypothesis of the batch with position 1 + h % L masked, then a row of
    T = 72 and one of T = 3 masked at their first word."""
    shape = SM.SHAPES[sid]
    _, seqs, *_ = SM.train_inputs(sid)
    rng = np.random.default_rng(7)
    for L in (70, 1):
        seqs = seqs + [[shape.cls_id] + rng.integers(106, shape.vocab, size=L).tolist() + [shape.sep_id]]
    rows, labs = [], []
    for h, s in enumerate(seqs):
        r = list(s)
        r[1 + h % (len(s) - 2)] = shape.mask_id
        rows.append(r)
        labs.append(list(s))
    assert len(rows[-2]) == 72 and len(rows[-1]) == 3
    return rows, labs


@pytest.mark.parametrize("sid", SM.TRAINER_IDS)
def test_mlm_step_and_update(sid):
    """MLMTrainer.step on a padded batch (pads are queries but not keys) against step_mlm: loss, every
    gradient, then one AdamW update."""
    from asr_rescoring_amd.train import MLMTrainer, pad_rows
    from oracle.bert_ref import set_cpu_threads
    from oracle.train_ref import TorchTrainer
    from asr_rescoring_amd.weights import make_weights
    set_cpu_threads()
    shape = SM.SHAPES[sid]
    assert shape.vocab % 4 == 0
    w = make_weights(shape, seed=5)
    rows, labs = _mlm_rows(sid)
    tr = MLMTrainer(w, shape, lr=LR, **NO_DROP)
    ref = TorchTrainer(w, shape, lr=LR, head="mlm")
    try:
        batch = pad_rows(rows, labs)
        l = tr.step(*batch, update=False)
        rl = ref.step_mlm(rows, labs, update=False)
        print(f"SHAPES {sid} train mlm: loss rel {abs(l - rl) / abs(rl):.3e}")
        assert abs(l - rl) <= 1e-4 * abs(rl), (l, rl)
        _check_grads(sid, "mlm", tr, ref.grad)
        before = {k: tr.tensor(k) for k in tr.shapes}
        tr.step(*batch, update=True)
        ref.step_mlm(rows, labs, update=True)
        _check_update(sid, "mlm", before, {k: tr.tensor(k) for k in tr.shapes},
                      {k: ref.tensor(k).reshape(tr.shapes[k]) for k in tr.shapes})
    finally:
        tr.close()
