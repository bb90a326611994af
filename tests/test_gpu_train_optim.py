"""Gradient accumulation, clipping, frozen tensors and the learning-rate hook of the native trainers
(rs_trainer_accumulate / _apply / _grad_norm / _set_trainable; train.py; cli.py), on the tiny BERT and
the batches of tests/train_fixtures.py.

Tolerances are the project's (tests/test_gpu_train.py): gradients within 2e-4 of the tensor's gradient
norm, floored at 1e-4 of the global norm; norms and losses within 1e-4 relative (fp32 on both sides,
different summation orders); parameter updates within 2e-2 of the update's norm per tensor, skipping
``attention.self.key.bias`` and exactly-zero gradients as ``check_updates`` does.  Everything that
include/rescore.h documents as bitwise is compared bitwise."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import yaml

from asr_rescoring_amd import _lib
from asr_rescoring_amd.weights import BERT_TINY
from train_fixtures import METHODS, mlm_fixture, rb_fixture

pytestmark = pytest.mark.gpu

NO_DROP = dict(hidden_dropout=0.0, attn_dropout=0.0)
RS_EARG, RS_ESTATE = -1, -3
FROZEN = ("bert.embeddings", "bert.encoder.layer.0")     # the tiny BERT has two layers
assert BERT_TINY.layers >= 2


def _rb(method="MD_MWER", **kw):
    from asr_rescoring_amd.train import RescoreBertTrainer
    w, trd, _, hp, _ = rb_fixture(method)
    kw = {"lr": 1e-3, "weight_decay": 0.01, **NO_DROP, **kw}
    return RescoreBertTrainer(w, BERT_TINY, method=method, md_loss_weight=hp["md_loss_weight"], **kw), w, trd, hp


def _rb_args(trd, hp, method, h0, h1):
    """Hypotheses [h0, h1) of the fixture's training split as one step's arguments."""
    from asr_rescoring_amd.train import reference_groups
    off = trd["hyp_off"].astype(np.int64)
    t0, t1 = int(off[h0]), int(off[h1])
    groups = np.array([0, h1 - h0], np.int32) if method == "MD" else reference_groups(h1 - h0, hp["n_best"])
    return (trd["tokens"][t0:t1], (off[h0:h1 + 1] - t0).astype(np.int32), groups, trd["pll"][h0:h1], trd["am"][h0:h1],
            trd["cer"][h0:h1])


@functools.lru_cache(maxsize=None)
def _mlm_rows():
    """The fixture's MLM rows with -100 labels: every third position keeps its label."""
    w, trd, _, hp, _ = mlm_fixture()
    labs = [[t if (p + i) % 3 == 0 else -100 for p, t in enumerate(l)] for i, l in enumerate(trd["labels"])]
    return w, trd["seqs"], labs, hp


def _mlm(**kw):
    from asr_rescoring_amd.train import MLMTrainer
    w, seqs, labs, hp = _mlm_rows()
    kw = {"lr": 1e-3, "weight_decay": 0.01, **NO_DROP, **kw}
    return MLMTrainer(w, BERT_TINY, **kw), w, seqs, labs


def _ragged(seqs, labs, r0, r1):
    """Rows [r0, r1) as ragged rows without key lengths: (ids, seq_off, labels, n labelled)."""
    ids = np.concatenate([np.asarray(s, np.int32) for s in seqs[r0:r1]])
    lab = np.concatenate([np.asarray(l, np.int32) for l in labs[r0:r1]])
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs[r0:r1]])]).astype(np.int32)
    return ids, off, lab, int(np.count_nonzero(lab != -100))


def _params(tr):
    return {k: tr.tensor(k) for k in tr.shapes}


def _same(a, b, keys=None):
    return [k for k in (a if keys is None else keys) if not np.array_equal(a[k].view(np.int32), b[k].view(np.int32))]


def _code(fn, *a, **kw):
    with pytest.raises(_lib.RescoreError) as e:
        fn(*a, **kw)
    return e.value.code


def _grads_close(got, want, keys):
    gn = np.sqrt(sum(float(np.sum(want[k].astype(np.float64) ** 2)) for k in keys))
    for k in keys:
        rel = np.linalg.norm(got[k].astype(np.float64) - want[k]) / max(np.linalg.norm(want[k]), 1e-4 * gn)
        assert rel < 2e-4, (k, rel)


def _updates_close(before, got, want, ref_grad, keys):
    for k in keys:
        if k.endswith("attention.self.key.bias") or not np.any(ref_grad(k)):
            continue
        d, rd = got[k] - before[k].reshape(got[k].shape), want[k] - before[k].reshape(got[k].shape)
        assert np.linalg.norm(d - rd) <= 2e-2 * max(np.linalg.norm(rd), 1e-12), k


# ---- 1. the bit contract of apply ----------------------------------------------------------------

@pytest.mark.parametrize("head", ["cls", "mlm"])
def test_apply_on_the_last_gradient_is_the_updating_step(head):
    """step(update=False) + apply(source="last") == step(update=True), and so is a second step after
    it (moments and step count)."""
    runs = []
    for split in (False, True):
        if head == "cls":
            tr, _, trd, hp = _rb("MD_MWED")
            batches = [_rb_args(trd, hp, "MD_MWED", 0, 6), _rb_args(trd, hp, "MD_MWED", 6, 12)]
        else:
            tr, _, seqs, labs = _mlm()
            batches = [_ragged(seqs, labs, 0, 5)[:3] + (None,), _ragged(seqs, labs, 5, 11)[:3] + (None,)]
        kw = {} if head == "cls" else {"ignore_index": -100}
        try:
            out = []
            for b in batches:
                if split:
                    tr.step(*b, update=False, **kw)
                    norm, applied = tr.apply(source="last")
                    assert applied and np.isfinite(norm) and norm > 0
                else:
                    tr.step(*b, update=True, **kw)
                out.append(_params(tr))
            runs.append(out)
        finally:
            tr.close()
    assert _same(runs[0][0], runs[1][0]) == [] and _same(runs[0][1], runs[1][1]) == []


# ---- 2. accumulation equals the big batch --------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
def test_rescorebert_accumulation_is_the_concatenated_batch(method):
    tr, _, trd, hp = _rb(method)
    try:
        tr.step(*_rb_args(trd, hp, method, 0, 12), update=False)
        big = {k: tr.grad(k) for k in tr.shapes}
        for h0, h1 in ((0, 6), (6, 12)):
            tr.step(*_rb_args(trd, hp, method, h0, h1), update=False)
            tr.accumulate(1.0)
        _grads_close({k: tr.accum(k) for k in tr.shapes}, big, list(tr.shapes))
        want = np.sqrt(sum(float(np.sum(tr.accum(k).astype(np.float64) ** 2)) for k in tr.shapes))
        assert abs(tr.grad_norm("accum") - want) <= 1e-9 * want
        tr.zero_accum()
        assert _code(tr.grad_norm, "accum") == RS_ESTATE
    finally:
        tr.close()


def test_mlm_accumulation_weighted_by_label_counts_is_the_concatenated_batch():
    tr, _, seqs, labs = _mlm()
    try:
        ids, off, lab, n_all = _ragged(seqs, labs, 0, 11)
        tr.step(ids, off, lab, update=False, ignore_index=-100)
        big = {k: tr.grad(k) for k in tr.shapes}
        tot = 0
        for r0, r1 in ((0, 5), (5, 11)):
            ids, off, lab, n = _ragged(seqs, labs, r0, r1)
            tr.step(ids, off, lab, update=False, ignore_index=-100)
            tr.accumulate(float(n))
            tot += n
        assert tot == n_all
        _grads_close({k: tr.accum(k).astype(np.float64) / tot for k in tr.shapes}, big, list(tr.shapes))
    finally:
        tr.close()


def test_micro_steps_advance_the_dropout_counter_by_one_each():
    tr, _, trd, hp = _rb("MD", hidden_dropout=0.1, attn_dropout=0.1, dropout_seed=3)
    try:
        key = tr.dropout_step()
        for h0, h1 in ((0, 6), (6, 12)):
            tr.step(*_rb_args(trd, hp, "MD", h0, h1), update=False)
            tr.accumulate(1.0)
        assert tr.dropout_step() == key + 2
        assert tr.apply(max_grad_norm=1.0)[1] and tr.dropout_step() == key + 2
    finally:
        tr.close()


# ---- 3. against torch: two backward passes, clip_grad_norm_, one AdamW step ----------------------

def _torch_rb_backward(ref, trd, hp, method, spans):
    from oracle.train_ref import rescorebert_loss
    ref.opt.zero_grad(set_to_none=False)
    for h0, h1 in spans:
        sc = ref.scores(trd["seqs"][h0:h1])
        rescorebert_loss(sc, trd["pll"][h0:h1], trd["am"][h0:h1], trd["cer"][h0:h1], hp["n_best"], method,
                         hp["md_loss_weight"]).backward()


def _torch_mlm_backward(ref, seqs, labs, spans):
    """The reference's padded batch (oracle/train_ref.py step_mlm), backward only, per span."""
    ref.opt.zero_grad(set_to_none=False)
    for r0, r1 in spans:
        rows, lb = seqs[r0:r1], labs[r0:r1]
        T = max(len(s) for s in rows)
        x, am, lab = (torch.zeros(len(rows), T, dtype=torch.long) for _ in range(3))
        for i, (sq, l) in enumerate(zip(rows, lb)):
            x[i, :len(sq)] = torch.as_tensor(np.asarray(sq, np.int64))
            am[i, :len(sq)] = 1
            lab[i, :len(l)] = torch.as_tensor(np.asarray(l, np.int64))
        logits = ref.model.mlm_logits(ref.model.encoder(x, am))
        torch.nn.functional.cross_entropy(logits.view(-1, logits.shape[-1]), lab.view(-1)).backward()


def _torch_clip_and_step(ref, factor):
    params = [p for p in ref.model.w.values() if p.grad is not None]
    norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params)))
    max_norm = factor * norm
    grads = {k: p.grad.detach().numpy().copy() for k, p in ref.model.w.items() if p.grad is not None}
    torch.nn.utils.clip_grad_norm_(params, max_norm)
    ref.opt.step()
    return norm, max_norm, grads


@pytest.mark.parametrize("factor", [0.5, 2.0])
@pytest.mark.parametrize("head", ["cls", "mlm"])
def test_accumulate_clip_step_matches_torch(head, factor, frozen=()):
    """factor 0.5: max_norm at half the torch norm, clipping active; 2.0: inactive."""
    from asr_rescoring_amd.train import pad_rows
    from oracle.train_ref import TorchTrainer
    spans = ((0, 6), (6, 12)) if head == "cls" else ((0, 5), (5, 11))
    if head == "cls":
        tr, w, trd, hp = _rb("MD_MWER")
        ref = TorchTrainer(w, BERT_TINY, lr=1e-3, weight_decay=0.01)
    else:
        tr, w, _, _ = _mlm()
        _, trd0, _, _, _ = mlm_fixture()
        seqs, labs = trd0["seqs"], trd0["labels"]
        ref = TorchTrainer(w, BERT_TINY, lr=1e-3, weight_decay=0.01, head="mlm")
    try:
        from asr_rescoring_amd.train import prefix_matches
        for k, p in ref.model.w.items():
            if any(prefix_matches(k, f) for f in frozen):
                p.requires_grad_(False)
        tr.freeze(*frozen)
        if head == "cls":
            _torch_rb_backward(ref, trd, hp, "MD_MWER", spans)
        else:
            _torch_mlm_backward(ref, seqs, labs, spans)
        rnorm, max_norm, rgrads = _torch_clip_and_step(ref, factor)
        before = _params(tr)
        for a, b in spans:
            if head == "cls":
                tr.step(*_rb_args(trd, hp, "MD_MWER", a, b), update=False)
            else:
                tr.step(*pad_rows(seqs[a:b], labs[a:b]), update=False)
            tr.accumulate(1.0)
        norm, applied = tr.apply(max_grad_norm=max_norm)
        print(f"CLIP {head} x{factor} frozen {len(frozen)}: norm {norm!r} torch {rnorm!r} max_norm {max_norm!r}")
        assert applied
        assert (norm > max_norm) == (factor < 1.0)            # precondition: clipping active / inactive
        assert abs(norm - rnorm) <= 1e-4 * rnorm
        after = _params(tr)
        trainable = [k for k in tr.shapes if tr.is_trainable(k)]
        assert sorted(trainable) == sorted(k for k in tr.shapes if k in rgrads)
        want = {k: ref.tensor(k).reshape(after[k].shape) for k in trainable}
        _updates_close(before, after, want, lambda k: rgrads[k], trainable)
        assert _same(before, after, [k for k in tr.shapes if k not in trainable]) == []
    finally:
        tr.close()


# ---- 4. frozen tensors ---------------------------------------------------------------------------

@pytest.mark.parametrize("head", ["cls", "mlm"])
def test_frozen_tensors_stay_and_the_rest_is_bitwise_the_all_trainable_step(head):
    def make():
        if head == "cls":
            tr, w, trd, hp = _rb("MD_MWED")
            return tr, lambda upd: tr.step(*_rb_args(trd, hp, "MD_MWED", 0, 12), update=upd)
        tr, w, seqs, labs = _mlm()
        return tr, lambda upd: tr.step(*_ragged(seqs, labs, 0, 11)[:3], update=upd, ignore_index=-100)
    tr, step = make()
    try:
        init = _params(tr)
        step(True)
        all_g, all_p = {k: tr.grad(k) for k in tr.shapes}, _params(tr)
    finally:
        tr.close()
    tr, step = make()
    try:
        tr.freeze(*FROZEN)
        frozen = [k for k in tr.shapes if not tr.is_trainable(k)]
        assert sorted(frozen) == sorted(k for k in tr.shapes if k.startswith(tuple(f + "." for f in FROZEN)))
        assert len(frozen) == 5 + 16
        live = [k for k in tr.shapes if k not in frozen]
        step(True)
        got_p = _params(tr)
        assert _same(init, got_p, frozen) == []                       # no update, no weight decay
        assert _same(all_p, got_p, live) == []
        assert all(tr.grad(k) is None for k in frozen)
        assert _same(all_g, {k: tr.grad(k) for k in live}, live) == []
        want = np.sqrt(sum(float(np.sum(all_g[k].astype(np.float64) ** 2)) for k in live))
        assert abs(tr.grad_norm("last") - want) <= 1e-9 * want
        assert _code(tr._get, tr.lib.rs_trainer_get_grad, frozen[0]) == RS_ESTATE
    finally:
        tr.close()
    # unfreeze: the all-trainable step again, bit for bit
    tr, step = make()
    try:
        tr.freeze(*FROZEN)
        tr.unfreeze("bert")
        assert all(tr.is_trainable(k) for k in tr.shapes)
        step(True)
        assert _same(all_p, _params(tr)) == [] and _same(all_g, {k: tr.grad(k) for k in tr.shapes}) == []
    finally:
        tr.close()


@pytest.mark.parametrize("head", ["cls", "mlm"])
def test_frozen_step_matches_torch_requires_grad_false(head):
    test_accumulate_clip_step_matches_torch(head, 0.5, frozen=FROZEN)


def test_one_of_the_fused_qkv_tensors_frozen():
    """The fused Q|K|V gradient launches run while any of the three is trainable: the other two keep
    their all-trainable gradients bitwise, the frozen one does not move."""
    tr, _, trd, hp = _rb("MD")
    try:
        init = _params(tr)
        tr.step(*_rb_args(trd, hp, "MD", 0, 12), update=True)
        all_p = _params(tr)
    finally:
        tr.close()
    tr, _, trd, hp = _rb("MD")
    try:
        tr.freeze("bert.encoder.layer.1.attention.self.key", "bert.encoder.layer.0.attention.self")
        tr.step(*_rb_args(trd, hp, "MD", 0, 12), update=True)
        got = _params(tr)
        frozen = [k for k in tr.shapes if not tr.is_trainable(k)]
        assert len(frozen) == 2 + 6
        assert _same(init, got, frozen) == [] and _same(all_p, got, [k for k in tr.shapes if k not in frozen]) == []
    finally:
        tr.close()


def test_mlm_freezing_cls_freezes_the_tied_word_embeddings():
    tr, _, seqs, labs = _mlm()
    try:
        word = "bert.embeddings.word_embeddings.weight"
        tr.freeze("cls")
        assert not tr.is_trainable(word) and not tr.is_trainable("cls.predictions.bias")
        assert tr.is_trainable("bert.embeddings.position_embeddings.weight")
        init = _params(tr)
        tr.step(*_ragged(seqs, labs, 0, 11)[:3], update=True, ignore_index=-100)
        got = _params(tr)
        head = [k for k in tr.shapes if k.startswith("cls.")] + [word]
        assert _same(init, got, head) == []
        assert "bert.encoder.layer.0.output.dense.weight" in _same(init, got)
        tr.unfreeze("cls.predictions.decoder")                       # the aliases alone
        assert tr.is_trainable(word) and tr.is_trainable("cls.predictions.bias")
        assert not tr.is_trainable("cls.predictions.transform.dense.weight")
    finally:
        tr.close()


def test_head_only_training_skips_the_encoder_backward_but_not_the_head():
    for make, batch, kw in ((lambda: _rb("MD"), None, {}), (_mlm, "mlm", {"ignore_index": -100})):
        made = make()
        tr = made[0]
        try:
            args = _rb_args(made[2], made[3], "MD", 0, 12) if batch is None else _ragged(made[2], made[3], 0, 11)[:3]
            tr.step(*args, update=False, **kw)
            head = [k for k in tr.shapes if not k.startswith("bert.")]
            all_g = {k: tr.grad(k) for k in head}
            tr.freeze("bert")
            init = _params(tr)
            tr.step(*args, update=True, **kw)
            live = [k for k in head if tr.is_trainable(k)]
            assert live and _same(all_g, {k: tr.grad(k) for k in live}, live) == []
            got = _params(tr)
            assert _same(init, got, [k for k in tr.shapes if k not in live]) == []
            assert sorted(_same(init, got)) == sorted(live)
        finally:
            tr.close()


# ---- 5. the skipped step of a non-finite gradient ------------------------------------------------

@pytest.mark.parametrize("source", ["accum", "last"])
def test_non_finite_gradient_skips_the_step(source):
    tr, _, trd, hp = _rb("MD")
    try:
        good = _rb_args(trd, hp, "MD", 0, 6)
        bad = list(_rb_args(trd, hp, "MD", 6, 12))
        bad[3] = bad[3].copy()
        bad[3][2] = np.inf                               # an MD target of inf: a value, not a fault
        init = _params(tr)
        tr.step(*bad, update=False)
        if source == "accum":
            tr.accumulate(1.0)
        norm, applied = tr.apply(max_grad_norm=1.0, source=source)
        assert not np.isfinite(norm) and applied is False
        assert _same(init, _params(tr)) == []
        if source == "accum":
            assert _code(tr.apply) == RS_ESTATE          # the accumulator was cleared with the skip
        tr.step(*good, update=True)
        seen = _params(tr)
    finally:
        tr.close()
    tr, _, trd, hp = _rb("MD")
    try:
        tr.step(*good, update=True)
        assert _same(_params(tr), seen) == []
    finally:
        tr.close()


# ---- 6. errors move nothing ----------------------------------------------------------------------

def test_errors_leave_parameters_and_the_dropout_counter_alone():
    tr, _, trd, hp = _rb("MD", hidden_dropout=0.1, attn_dropout=0.1)
    try:
        init, key = _params(tr), tr.dropout_step()
        args = _rb_args(trd, hp, "MD", 0, 6)
        assert _code(tr.accumulate) == RS_ESTATE                      # before any backward
        assert _code(tr.apply, source="last") == RS_ESTATE
        assert _code(tr.apply, source="accum") == RS_ESTATE           # empty accumulator
        assert _code(tr.grad_norm, "accum") == RS_ESTATE
        assert _code(tr.freeze, "bert.encoder.layer.7") == RS_EARG    # matches nothing
        assert _code(tr.freeze, "bert.encoder.lay") == RS_EARG
        assert _code(tr.is_trainable, "no.such.tensor") == RS_EARG
        tr.freeze("bert", "linear")
        assert _code(tr.step, *args, update=True) == RS_ESTATE        # everything frozen
        assert _code(tr.step, *args, update=False) == RS_ESTATE
        assert tr.dropout_step() == key and _same(init, _params(tr)) == []
        loss, _ = tr.step(*args, update="loss")                       # the loss-only pass needs no gradient
        assert np.isfinite(loss) and tr.dropout_step() == key
        tr.unfreeze("bert", "linear")
        tr.step(*args, update=False)
        tr.accumulate()
        assert tr.dropout_step() == key + 1
        assert _code(tr.freeze, "linear") == RS_ESTATE                # non-empty accumulator
        assert _code(tr.unfreeze, "linear") == RS_ESTATE
        assert tr.is_trainable("linear.weight")
        assert _same(init, _params(tr)) == [] and tr.dropout_step() == key + 1
        tr.zero_accum()
        tr.freeze("linear")
        assert _code(tr.accumulate) == RS_ESTATE                      # the old gradient went with the change
    finally:
        tr.close()


# ---- 7. epoch helpers and CLI --------------------------------------------------------------------

def test_rescorebert_epoch_defaults_and_accumulation():
    from asr_rescoring_amd.train import rescorebert_epoch
    method = "MD_MWER"
    tr, _, trd, hp = _rb(method)
    data = (trd["tokens"], trd["hyp_off"], trd["pll"], trd["am"], trd["cer"])
    try:
        rows = hp["batch_size"] * hp["n_best"]
        losses = [tr.step(*_rb_args(trd, hp, method, b, b + rows), update=True)[0] for b in range(0, 12, rows)]
        want_p, want_l = _params(tr), sum(losses) / len(losses)
    finally:
        tr.close()
    tr, _, _, _ = _rb(method)
    try:
        assert rescorebert_epoch(tr, *data, hp["batch_size"], hp["n_best"], update=True) == want_l
        assert _same(want_p, _params(tr)) == []
    finally:
        tr.close()
    tr, _, _, _ = _rb(method)
    try:
        seen, init = [], _params(tr)

        def lr_of(k):
            seen.append(k)
            return 0.0 if k == 0 else 1e-3
        # 4 batches of one utterance, groups of 3: 3 + 1 batches, ceil(4 / 3) optimizer steps
        loss = rescorebert_epoch(tr, *data, 1, hp["n_best"], update=True, accum_steps=3, max_grad_norm=5.0, lr_of_step=lr_of)
        assert seen == [0, 1] and np.isfinite(loss)
        assert _code(tr.apply) == RS_ESTATE                # nothing left in the accumulator
        assert _same(init, _params(tr)) != []
    finally:
        tr.close()
    # lr 0 and no decay: the first group's step moves nothing, so the lr of the recorder is the one used
    tr, _, _, _ = _rb(method, weight_decay=0.0)
    try:
        init = _params(tr)
        rescorebert_epoch(tr, *data, 2, hp["n_best"], update=True, accum_steps=2, lr_of_step=lambda k: 0.0)
        assert _same(init, _params(tr)) == []
    finally:
        tr.close()


def test_mlm_epoch_defaults_and_accumulation():
    from asr_rescoring_amd.train import mlm_epoch, pad_rows
    _, trd, _, hp, _ = mlm_fixture()
    seqs, labs, bs = trd["seqs"], trd["labels"], hp["batch_size"]
    tr = _mlm()[0]
    try:
        losses = [tr.step(*pad_rows(seqs[b:b + bs], labs[b:b + bs]), update=True) for b in range(0, len(seqs), bs)]
        want_p, want_l = _params(tr), sum(losses) / len(losses)
    finally:
        tr.close()
    tr = _mlm()[0]
    try:
        assert mlm_epoch(tr, seqs, labs, bs, update=True) == want_l
        assert _same(want_p, _params(tr)) == []
    finally:
        tr.close()
    tr = _mlm()[0]
    try:
        seen = []
        n_batches = -(-len(seqs) // bs)
        assert n_batches == 3
        mlm_epoch(tr, seqs, labs, bs, update=True, accum_steps=2, max_grad_norm=1.0,
                  lr_of_step=lambda k: seen.append(k) or 1e-3)
        assert seen == [0, 1]
        # labelled steps, one short group of all three batches
        w, rows, labs3, _ = _mlm_rows()
        mlm_epoch(tr, rows, labs3, bs, update=True, ignore_index=-100, accum_steps=4)
        assert _code(tr.apply) == RS_ESTATE
    finally:
        tr.close()


@pytest.fixture(scope="module")
def c1(golden_dir, tmp_path_factory):
    g = json.load(open(os.path.join(golden_dir, "c1_plumbing.json"), encoding="utf-8"))
    d = tmp_path_factory.mktemp("c1_optim")
    for name in ("hyps_text", "ref_text", "hyps_score"):
        json.dump(g[name], open(d / f"{name}.json", "w", encoding="utf-8"), ensure_ascii=False)
    special = {0: "[PAD]", 100: "[UNK]", 101: "[CLS]", 102: "[SEP]", 103: "[MASK]"}
    lines = [special.get(i, f"[unused{i}]") for i in range(106)] + list(g["charset"])
    (d / "vocab.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    return g, d


def _cfg(d, name, obj):
    p = d / name
    p.write_text(yaml.safe_dump(obj, allow_unicode=True), encoding="utf-8")
    return str(p)


OPTIM_KEYS = {"accum_steps": 2, "max_grad_norm": 1.0, "lr_schedule": "linear", "warmup_steps": 1,
              "freeze": ["bert.embeddings", "bert.encoder.layer.0", "bert.encoder.layer.1"]}


def _frozen_equal_initial(sd, kind):
    from asr_rescoring_amd.weights import BERT_BASE, make_weights
    w = make_weights(BERT_BASE, seed=1234, with_cls_linear=(kind == "cls"), with_pooler=(kind == "cls"))
    frozen = [k for k in sd if k.startswith(tuple(f + "." for f in OPTIM_KEYS["freeze"]))]
    assert len(frozen) == 5 + 32
    assert all(np.array_equal(sd[k].numpy().ravel(), np.asarray(w[k], np.float32).ravel()) for k in frozen)
    moved = "bert.encoder.layer.11.output.dense.weight"
    assert not np.array_equal(sd[moved].numpy().ravel(), np.asarray(w[moved], np.float32).ravel())


def test_cli_rescorebert_train_with_the_optimizer_options(c1):
    from asr_rescoring_amd import cli
    g, d = c1
    json.dump(g["lm"], open(d / "mlm_score.json", "w", encoding="utf-8"), ensure_ascii=False)
    json.dump(g["hyps_cer"], open(d / "hyps_cer.json", "w", encoding="utf-8"), ensure_ascii=False)
    feats = ["hyps_token_ids", "mlm_pll_score", "hyps_am_score", "hyps_cer"]
    fpaths = [str(d / f) for f in ("hyps_text.json", "mlm_score.json", "hyps_score.json", "hyps_cer.json")]
    out = d / "rb_out"
    res = cli.rescorebert_train(cli.ArgParser().parse(["--config", _cfg(d, "rb_train.yaml", {
        "task": "training", "method": "MD_MWER", "seed": 10, "md_loss_weight": 0.0001, "lr": 1e-4, "epoch": 1,
        "device": "cuda:0", "random_init_seed": 1234, "train_feature": feats, "train_feature_path": fpaths,
        "output_path": str(out), "batch_size": 1, "max_utt": 3, "n_best": 4,
        "model": {"bert": "bert-base-chinese", "vocab": str(d / "vocab.txt")}, **OPTIM_KEYS})]))
    assert len(res["train_loss"]) == 1 and np.isfinite(res["train_loss"][0])
    sd = torch.load(res["checkpoints"][-1], map_location="cpu", weights_only=True)
    _frozen_equal_initial(sd, "cls")
    files = cli.rescorebert(cli.ArgParser().parse(["--config", _cfg(d, "rb_score.yaml", {
        "device": "cuda:0", "checkpoint_path": res["checkpoints"][-1], "n_best": 4, "max_utt": 3,
        "model": {"bert": "bert-base-chinese", "vocab": str(d / "vocab.txt")},
        "dev_feature": ["hyps_token_ids"], "dev_feature_path": [str(d / "hyps_text.json")],
        "dev_output_format": str(d / "hyps_score.json"), "output_path": str(out)})]))
    lm = json.load(open(files["dev"], encoding="utf-8"))
    assert all(np.isfinite(v) for u in lm.values() for v in u.values())


def test_cli_mlm_finetune_with_the_optimizer_options(c1):
    from asr_rescoring_amd import cli
    from asr_rescoring_amd.frontend import NativeTokenizer
    from asr_rescoring_amd.scorer import PLLScorer
    from asr_rescoring_amd.train import do_job_rows
    from asr_rescoring_amd.weights import BERT_BASE
    g, d = c1
    tok = NativeTokenizer(str(d / "vocab.txt"))
    rows = []
    for u, t in g["ref_text"].items():
        ids, off, lab = do_job_rows([[101] + tok.encode(t) + [102]])
        for i in range(len(off) - 1):
            r = ids[off[i]:off[i + 1]].tolist()
            rows.append({"utt_id": u, "hyp_id": None, "input_ids": r, "attention_masks": [1] * len(r),
                         "mask_pos": i + 1, "labels": lab[off[i]:off[i + 1]].tolist()})
    assert len(rows) >= 24                                  # three batches of 8: two optimizer steps
    json.dump(rows, open(d / "train_rows.json", "w"))
    out = d / "mlm_out"
    res = cli.mlm_finetune(cli.ArgParser().parse(["--config", _cfg(d, "mlm_train.yaml", {
        "task": "training", "seed": 10, "lr": 1e-4, "epoch": 1, "device": "cuda:0", "random_init_seed": 1234,
        "train_data_path": str(d / "train_rows.json"), "output_path": str(out), "num_of_data": 24,
        "dataloader": {"shuffle": False, "batch_size": 8},
        "model": {"bert": "bert-base-chinese", "vocab": str(d / "vocab.txt")}, **OPTIM_KEYS})]))
    assert len(res["train_loss"]) == 1 and np.isfinite(res["train_loss"][0])
    sd = torch.load(res["checkpoints"][-1], map_location="cpu", weights_only=True)
    _frozen_equal_initial(sd, "mlm")
    assert torch.equal(sd["cls.predictions.decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])
    sc = PLLScorer({k: v.numpy() for k, v in sd.items()}, BERT_BASE, device=0, max_rows=4096)
    try:
        pll = sc.score_nbest(np.asarray([101, 200, 300, 102], np.int32), np.asarray([0, 4], np.int32))
        assert np.isfinite(pll.cpu().numpy()).all()
    finally:
        sc.close()
