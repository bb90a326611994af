"""GPU: labelled-row MLM training (``rs_train_step_mlm_labeled``, ``MLMTrainer.step(ignore_index=-100)``):
the head (transform + tied decoder + CE) over the labelled rows only, CE mean over them
(CrossEntropyLoss(ignore_index=-100), modeling_bert.py:972-975).

Reference: ``oracle.train_ref.TorchTrainer.step_mlm`` as it stands (its cross_entropy ignores -100),
fed label rows padded by the test to the batch's longest length with -100, so its own zero padding
never applies; the case with segment ids uses the typed float64 autograd model of tests/seg_ref.py
(the oracle's encoder takes no token types).  Tolerances: the trainer suite's own
(tests/test_gpu_train.py): loss within 1e-4 relative, each gradient within 2e-4 of
max(|ref grad|, 1e-4 |all grads|)."""
import ctypes

import numpy as np
import pytest
import torch

from asr_rescoring_amd.weights import BERT_TINY, make_weights

pytestmark = pytest.mark.gpu

S = BERT_TINY
NO_DROP = dict(hidden_dropout=0.0, attn_dropout=0.0)
IGN = -100
RS_EARG, RS_ESTATE = -1, -3          # include/rescore.h


def _rows(seed, lens):
    rng = np.random.default_rng(seed)
    return [[S.cls_id] + rng.integers(104, S.vocab, t - 2).tolist() + [S.sep_id] for t in lens]


def _padded_labels(rows, at):
    """Label rows of the batch's longest length: -100 everywhere but ``at`` = {(row, position): id}."""
    T = max(len(r) for r in rows)
    labs = [[IGN] * T for _ in rows]
    for (i, p), v in at.items():
        labs[i][p] = v
    return labs


def _check_grads(tr, ref_grad):
    gn = np.sqrt(sum(float(np.sum(np.asarray(ref_grad(k), np.float64) ** 2)) for k in tr.shapes))
    for k in tr.shapes:
        g, rg = tr.grad(k), np.asarray(ref_grad(k))
        rel = np.linalg.norm(g - rg) / max(np.linalg.norm(rg), 1e-4 * gn)
        assert rel < 2e-4, (k, rel, np.linalg.norm(rg))


def _parity(rows, labs, seed=6, steps=2):
    """Step 0: loss and every gradient vs autograd; then an AdamW update on both sides and the loss
    of the next step."""
    from asr_rescoring_amd.train import MLMTrainer, pad_rows
    from oracle.train_ref import TorchTrainer
    w = make_weights(S, seed=seed)
    tr = MLMTrainer(w, S, lr=1e-3, **NO_DROP)
    ref = TorchTrainer(w, S, lr=1e-3, head="mlm")
    try:
        batch = pad_rows(rows, labs, label_pad=IGN)
        l0 = tr.step(*batch, update=False, ignore_index=IGN)
        r0 = ref.step_mlm(rows, labs, update=False)
        print(f"step 0: loss {l0:.6f} vs {r0:.6f}")
        assert abs(l0 - r0) <= 1e-4 * abs(r0), (l0, r0)
        _check_grads(tr, lambda k: ref.model.w[k].grad.numpy())
        for step in range(steps):
            l, rl = tr.step(*batch, ignore_index=IGN), ref.step_mlm(rows, labs)
            print(f"update step {step}: loss {l:.6f} vs {rl:.6f}")
            assert abs(l - rl) <= 1e-4 * abs(rl), (step, l, rl)
        assert l != l0                                  # the update moved the parameters
    finally:
        tr.close()


RAGGED = [3, 14, 5, 9, 12, 7]


def _ragged_labels(rows, every_position_of=None):
    """7 labels (not a multiple of 4): a [CLS] position, one pad position, none in row 2."""
    at = {(0, 0): rows[0][0], (0, 1): rows[0][1], (1, 13): rows[1][13], (3, 4): 17, (3, 11): 5,
          (4, 6): rows[4][6], (5, 3): 999}
    assert len(rows[3]) == 9                            # (3, 11) is past row 3's end: a pad position
    if every_position_of is not None:
        i = every_position_of
        at.update({(i, p): rows[i][p] for p in range(len(rows[i]))})
    return _padded_labels(rows, at)


def test_labelled_step_matches_autograd_on_a_ragged_label_pattern():
    rows = _rows(31, RAGGED)
    labs = _ragged_labels(rows)
    assert sum(v != IGN for l in labs for v in l) == 7 and all(v == IGN for v in labs[2])
    _parity(rows, labs)


def test_labelled_step_with_a_row_labelled_at_every_real_position():
    rows = _rows(32, RAGGED)
    labs = _ragged_labels(rows, every_position_of=4)
    assert sum(v != IGN for v in labs[4]) == 12 and sum(v != IGN for l in labs for v in l) == 18
    _parity(rows, labs)


def test_one_label_in_a_batch_of_two_rows():
    rows = _rows(33, [6, 11])
    _parity(rows, _padded_labels(rows, {(1, 4): rows[1][4]}))


def _do_job_batch(seed, n=3, len_hi=12):
    from asr_rescoring_amd.train import do_job_rows, pad_rows
    rng = np.random.default_rng(seed)
    seqs = _rows(seed, rng.integers(4, len_hi + 1, n).tolist())
    ids, off, lab = do_job_rows(seqs)
    rows = [ids[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    labs = [lab[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    return rows, labs, pad_rows(rows, labs)


def test_all_rows_labelled_is_the_old_entry_bit_for_bit():
    from asr_rescoring_amd.train import MLMTrainer
    w = make_weights(S, seed=7)
    _, _, batch = _do_job_batch(41)
    assert (batch[2] != IGN).all() and len(batch[3]) > 8 and batch[3].min() < batch[3].max()
    out = []
    for kw in ({}, {"ignore_index": IGN}):
        tr = MLMTrainer(w, S, lr=1e-3, **NO_DROP)
        try:
            loss = tr.step(*batch, **kw)
            out.append((loss, {k: tr.grad(k) for k in tr.shapes}, {k: tr.tensor(k) for k in tr.shapes}))
        finally:
            tr.close()
    (l0, g0, p0), (l1, g1, p1) = out
    assert l0 == l1
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
        assert np.array_equal(p0[k], p1[k]), k
    assert any(not np.array_equal(p0[k], w[k].reshape(p0[k].shape)) for k in p0)


def test_labelled_steps_are_deterministic():
    from asr_rescoring_amd.train import MLMTrainer, mask_tokens, pad_rows
    w = make_weights(S, seed=9)
    rows = _rows(50, [9, 4, 14, 7, 11, 6, 13, 8])
    batches = []
    for step in range(8):
        m, l = mask_tokens(rows, S, (3, step), mlm_probability=0.3)
        batches.append(pad_rows(m, l, label_pad=IGN))
    assert len({int((b[2] != IGN).sum()) for b in batches}) > 2      # several head sizes
    runs = []
    for _ in range(2):
        tr = MLMTrainer(w, S, lr=1e-3, **NO_DROP)
        try:
            losses = [tr.step(*b, ignore_index=IGN) for b in batches]
            runs.append((losses, {k: tr.tensor(k) for k in tr.shapes}))
        finally:
            tr.close()
    assert runs[0][0] == runs[1][0]
    assert all(np.array_equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_labelled_step_with_token_types_and_key_len():
    """Segment ids, padded rows with key lengths and labelled rows in one step, against float64
    autograd with per-token types (tests/seg_ref.py) on the same padded batch."""
    import torch.nn.functional as Fn
    import seg_ref
    from asr_rescoring_amd.train import MLMTrainer, pad_rows
    w = make_weights(S, seed=6)
    rows = _rows(34, [10, 6, 13, 4])
    types = [[0] * (len(r) // 2) + [1] * (len(r) - len(r) // 2) for r in rows]
    labs = _padded_labels(rows, {(0, 3): rows[0][3], (0, 8): 55, (1, 0): rows[1][0], (2, 12): rows[2][12],
                                 (3, 9): 7})              # (3, 9): a pad position of the 4-token row
    tr = MLMTrainer(w, S, lr=1e-3, **NO_DROP)
    try:
        ids, off, lab, klen, tt = pad_rows(rows, labs, types, label_pad=IGN)
        loss = tr.step(ids, off, lab, klen, update=False, token_types=tt, ignore_index=IGN)
        m = seg_ref.SegBert({k: w[k] for k in tr.shapes}, S, grad=True)
        T = len(labs[0])
        x, am = torch.as_tensor(ids.reshape(-1, T).astype(np.int64)), torch.zeros(len(rows), T, dtype=torch.long)
        for i, r in enumerate(rows):
            am[i, :len(r)] = 1
        logits = m.mlm_logits(m.encoder(x, am, torch.as_tensor(tt.reshape(-1, T).astype(np.int64))))
        rloss = Fn.cross_entropy(logits.view(-1, S.vocab), torch.as_tensor(np.asarray(labs, np.int64)).view(-1),
                                 ignore_index=IGN)
        rloss.backward()
        rloss = float(rloss.detach())
        print(f"typed: loss {loss:.6f} vs {rloss:.6f}")
        assert abs(loss - rloss) <= 1e-4 * abs(rloss)
        _check_grads(tr, lambda k: (m.w[k].grad.detach() if m.w[k].grad is not None
                                    else torch.zeros_like(m.w[k]).detach()).numpy())
        # the types took effect
        untyped = tr.step(ids, off, lab, klen, update=False, ignore_index=IGN)
        assert abs(untyped - loss) > 1e-4 * abs(loss)
    finally:
        tr.close()


def test_labelled_step_on_a_160_token_row_takes_the_tiled_attention():
    from asr_rescoring_amd.train import MLMTrainer, pad_rows
    from oracle.train_ref import TorchTrainer
    w = make_weights(S, seed=6)
    rows = _rows(35, [160, 23])
    labs = _padded_labels(rows, {(0, 1): rows[0][1], (0, 77): rows[0][77], (0, 158): 300, (1, 5): rows[1][5],
                                 (1, 130): 4})            # (1, 130): a pad position
    tr = MLMTrainer(w, S, lr=1e-3, **NO_DROP)
    ref = TorchTrainer(w, S, lr=1e-3, head="mlm")
    try:
        l = tr.step(*pad_rows(rows, labs, label_pad=IGN), update=False, ignore_index=IGN)
        rl = ref.step_mlm(rows, labs, update=False)
        assert abs(l - rl) <= 1e-4 * abs(rl), (l, rl)
        keys = ["cls.predictions.transform.dense.weight", "bert.embeddings.word_embeddings.weight",
                "bert.encoder.layer.0.attention.self.query.weight", "bert.encoder.layer.0.attention.self.key.weight",
                "bert.encoder.layer.0.attention.self.value.weight"]
        gn = np.sqrt(sum(float(np.sum(ref.model.w[k].grad.numpy().astype(np.float64) ** 2)) for k in tr.shapes))
        for k in keys:
            g, rg = tr.grad(k), ref.model.w[k].grad.numpy()
            rel = np.linalg.norm(g - rg) / max(np.linalg.norm(rg), 1e-4 * gn)
            assert rel < 2e-4, (k, rel)
    finally:
        tr.close()


def test_labelled_step_with_dropout_matches_oracle_fed_the_same_masks():
    """p = 0.1: the masks of the step's dropout key, exported by ``dropout_keep`` and fed to the oracle
    through ``padded_drop`` (as test_mlm_dropout_matches_oracle_fed_the_same_masks does): the
    dropout sites and the step counter are those of the old entry."""
    from asr_rescoring_amd.train import MLMTrainer, dropout_keep, pad_rows
    from oracle.train_ref import TorchTrainer, padded_drop
    w = make_weights(S, seed=12)
    rows = _rows(36, [8, 12, 5, 10])
    labs = _padded_labels(rows, {(0, 2): rows[0][2], (1, 7): rows[1][7], (1, 8): 44, (2, 0): rows[2][0],
                                 (2, 10): 9, (3, 6): rows[3][6]})
    tr = MLMTrainer(w, S, lr=1e-3, dropout_seed=5)
    ref = TorchTrainer(w, S, lr=1e-3, head="mlm")
    try:
        key = tr.dropout_step()
        l = tr.step(*pad_rows(rows, labs, label_pad=IGN), update=False, ignore_index=IGN)
        assert tr.dropout_step() == key + 1
        T = len(labs[0])
        keep = lambda site, n: dropout_keep(5, key, site, 0.1, n)
        drop = padded_drop(keep, [T] * len(rows), S.hidden, S.heads, S.layers, 0.1, 0.1)
        rl = ref.step_mlm(rows, labs, update=False, drop=drop)
        assert abs(l - rl) <= 1e-4 * abs(rl), (l, rl)
        _check_grads(tr, lambda k: ref.model.w[k].grad.numpy())
        nl = ref.step_mlm(rows, labs, update="loss")     # without the masks: dropout really was applied
        assert abs(nl - l) > 1e-3 * abs(nl)
    finally:
        tr.close()


def test_dev_pass_returns_the_loss_and_changes_nothing():
    from asr_rescoring_amd.train import MLMTrainer, pad_rows
    w = make_weights(S, seed=8)
    rows = _rows(37, RAGGED)
    batch = pad_rows(rows, _ragged_labels(rows), label_pad=IGN)
    tr = MLMTrainer(w, S, lr=1e-3, **NO_DROP)
    try:
        before = {k: tr.tensor(k) for k in tr.shapes}
        dev = tr.step(*batch, update="loss", ignore_index=IGN)
        assert all(np.array_equal(before[k], tr.tensor(k)) for k in before)
    finally:
        tr.close()
    tr = MLMTrainer(w, S, lr=1e-3, **NO_DROP)
    try:
        assert tr.step(*batch, update=True, ignore_index=IGN) == dev
        assert any(not np.array_equal(before[k], tr.tensor(k)) for k in before)
    finally:
        tr.close()


def _raw_labelled_call(tr, ids, off, klen, lab_row, n_lab, lab_id):
    """rs_train_step_mlm_labeled through ctypes with a caller-made row list; returns the status."""
    from asr_rescoring_amd import _lib
    dev = tr.device
    d_ids = torch.as_tensor(np.ascontiguousarray(ids, np.int32)).to(dev)
    d_lab = torch.as_tensor(np.ascontiguousarray(lab_id, np.int32)).to(dev)
    rows = np.ascontiguousarray(lab_row, np.int32)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    tr.opts.update = 1
    return tr.lib.rs_train_step_mlm_labeled(tr.handle, _lib.ptr(d_ids), off.ctypes.data, len(off) - 1, klen.ctypes.data,
                                            rows.ctypes.data, n_lab, _lib.ptr(d_lab), ctypes.byref(tr.opts),
                                            _lib.ptr(loss), _lib.stream_ptr(dev))


def test_errors_leave_the_trainer_usable():
    from asr_rescoring_amd import _lib
    from asr_rescoring_amd.train import MLMTrainer, RescoreBertTrainer, pad_rows
    w = make_weights(S, seed=8, with_cls_linear=True, with_pooler=True)
    rows = _rows(38, [7, 5])
    labs = _padded_labels(rows, {(0, 2): rows[0][2], (1, 3): rows[1][3], (1, 6): 3})
    ids, off, lab, klen = pad_rows(rows, labs, label_pad=IGN)
    M = int(off[-1])
    tr = MLMTrainer(w, S, lr=1e-3, **NO_DROP)
    try:
        good = lambda: tr.step(ids, off, lab, klen, update=False, ignore_index=IGN)
        want = good()
        with pytest.raises(ValueError, match="no labelled position"):
            tr.step(ids, off, np.full(M, IGN, np.int32), klen, ignore_index=IGN)
        assert good() == want
        bad = lab.copy()
        bad[4] = 1000
        with pytest.raises(ValueError, match="1000"):
            tr.step(ids, off, bad, klen, ignore_index=IGN)
        assert good() == want
        for lab_row, n_lab, msg in (([2], 0, r"n_lab = 0"),
                                    ([2, 9, 8], 3, r"h_lab_row\[2\] = 8"),
                                    ([2, 9, 9], 3, r"h_lab_row\[2\] = 9"),
                                    ([2, M], 2, r"h_lab_row\[1\] = %d" % M),
                                    ([-1, 3], 2, r"h_lab_row\[0\] = -1")):
            rc = _raw_labelled_call(tr, ids, off, klen, lab_row, n_lab, [5] * len(lab_row))
            assert rc == RS_EARG, (lab_row, rc)
            with pytest.raises(_lib.RescoreError, match=msg):
                _lib.check(rc)
            assert good() == want
        before = {k: tr.tensor(k) for k in tr.shapes}
        assert good() == want and all(np.array_equal(before[k], tr.tensor(k)) for k in before)
    finally:
        tr.close()
    # with dropout on: a refused row list or label set leaves the dropout-step counter where it was,
    # so the next step draws the masks it would have drawn (the same loss as on a fresh trainer)
    losses = []
    for spoil in (False, True):
        tr = MLMTrainer(w, S, lr=1e-3, dropout_seed=5)
        try:
            key = tr.dropout_step()
            if spoil:
                for lab_row, n_lab in (([2], 0), ([2, 9, 8], 3), ([2, M], 2)):
                    assert _raw_labelled_call(tr, ids, off, klen, lab_row, n_lab, [5] * len(lab_row)) == RS_EARG
                with pytest.raises(ValueError):
                    tr.step(ids, off, np.full(M, IGN, np.int32), klen, ignore_index=IGN)
                assert tr.dropout_step() == key
            losses.append(tr.step(ids, off, lab, klen, update=False, ignore_index=IGN))
            assert tr.dropout_step() == key + 1
        finally:
            tr.close()
    assert losses[0] == losses[1]
    cls = RescoreBertTrainer(w, S, **NO_DROP)
    try:
        rc = _raw_labelled_call(cls, ids, off, klen, [2, 3], 2, [5, 6])
        assert rc == RS_ESTATE
        with pytest.raises(_lib.RescoreError, match="no MLM head"):
            _lib.check(rc)
    finally:
        cls.close()


# ---- end to end ---------------------------------------------------------------------------------

FT = dict(steps=10, batch_size=8, lr=1e-3, seed=3)


def finetune_corpus():
    """A small repeated corpus: 6 sentences of 5..10 words over 24 word ids, four copies each."""
    rng = np.random.default_rng(77)
    words = rng.choice(np.arange(200, S.vocab), 24, replace=False)
    sents = [rng.choice(words, int(rng.integers(5, 11))).tolist() for _ in range(6)]
    return sents * 4


def dev_masking(sents):
    """One fixed-seed masking of the corpus' distinct sentences: (rows, padded label rows)."""
    from asr_rescoring_amd.train import mask_tokens
    rows = [[S.cls_id] + s + [S.sep_id] for s in sents[:6]]
    m, l = mask_tokens(rows, S, 12345, mlm_probability=0.3)
    T = max(len(r) for r in m)
    return m, [x + [IGN] * (T - len(x)) for x in l]


def test_do_job_masked_finetune_labels_the_mask_only():
    """``masking="do_job_masked"``: the do_job rows of the default mode in the same seeded order,
    labelled at their [MASK] only — the first step's loss against the oracle on those rows."""
    from asr_rescoring_amd.train import finetune_mlm_on_texts
    from oracle.train_ref import TorchTrainer
    w = make_weights(S, seed=6)
    sents = finetune_corpus()[:6]
    _, losses = finetune_mlm_on_texts(w, sents, S, steps=2, batch_size=8, lr=1e-3, seed=3, masking="do_job_masked")
    rows, labs = [], []
    for s in sents:
        h = [S.cls_id] + s + [S.sep_id]
        for p in range(1, len(h) - 1):
            rows.append(h[:p] + [S.mask_id] + h[p + 1:])
            labs.append({p: h[p]})
    sel = np.random.Generator(np.random.PCG64(3)).permutation(len(rows))[:8]
    T = max(len(rows[i]) for i in sel)
    ref = TorchTrainer(w, S, lr=1e-3, head="mlm")
    rl = ref.step_mlm([rows[i] for i in sel], [[labs[i].get(p, IGN) for p in range(T)] for i in sel], update=False)
    assert abs(losses[0] - rl) <= 1e-4 * abs(rl), (losses[0], rl)
    assert len(losses) == 2 and losses[1] != losses[0]


def test_dynamic_finetune_feeds_the_pll_scorer_and_lowers_the_dev_loss():
    """``finetune_mlm_on_texts(masking="dynamic")`` on the repeated corpus: the state dict loads into
    PLLScorer and scores as oracle.bert_ref does (1e-3 relative, the existing finetune test's
    bound); the labelled loss of one fixed-seed dev masking is lower after training than before.

    Steps and lr were chosen with the same loop (the same seeds, batches and masks) on
    ``TorchTrainer`` on the CPU at lr 1e-3: its own loss on this dev masking (11 labels) is 7.6235
    before training and 3.5474 after 10 steps (2.5357 after 20, 1.3836 after 40, 0.8771 after 80);
    10, the smallest count tried, already more than halves it."""
    from asr_rescoring_amd import data as D
    from asr_rescoring_amd.scorer import PLLScorer
    from asr_rescoring_amd.train import MLMTrainer, finetune_mlm_on_texts, pad_rows
    from oracle.bert_ref import TorchBert, pll_reference_pattern
    w = make_weights(S, seed=6)
    sents = finetune_corpus()
    dev_rows, dev_labs = dev_masking(sents)
    dev_batch = pad_rows(dev_rows, dev_labs, label_pad=IGN)

    def dev_loss(weights):
        tr = MLMTrainer(weights, S, **NO_DROP)
        try:
            return tr.step(*dev_batch, update="loss", ignore_index=IGN)
        finally:
            tr.close()
    sd, losses = finetune_mlm_on_texts(w, sents, S, masking="dynamic", **FT)
    assert len(losses) == FT["steps"] and np.isfinite(losses).all()
    before, after = dev_loss(w), dev_loss(sd)
    print(f"dev loss {before:.4f} -> {after:.4f}; train {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert after < before
    nb = D.synthetic_nbest(2, 3, seed=40, vocab=S.vocab, len_lo=1, len_hi=12)
    sc = PLLScorer(sd, S, device=0, precision="fp16x3")
    try:
        got = sc.score(nb)
    finally:
        sc.close()
    _, want = pll_reference_pattern(TorchBert(sd, S), nb.tokens, nb.hyp_off, full_head=False)
    assert (np.abs(got - want) / np.abs(want)).max() < 1e-3
