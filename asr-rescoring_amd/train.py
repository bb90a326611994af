"""RescoreBert distillation training and MLM fine-tuning on the GPU (SURVEY §8f item 2;
RescoreBert/main.py:82-229, MLM_PLL/main.py:73-161).

``RescoreBertTrainer`` keeps the fp32 parameters, gradients and AdamW moments of a
``RescoreBert`` (BERT encoder + ``Linear(H, 1)`` on the CLS hidden state,
RescoreBert/model.py:4-21) resident on one GPU; ``step`` runs the native training step
(``rs_train_step_cls``): forward with saved activations, the distillation loss, the backward
through head, encoder and embeddings, and one ``torch.optim.AdamW`` update.

Losses exactly as RescoreBert/main.py:104-147 computes them (``csrc/train.h``), over groups of
consecutive hypotheses (the reference's ``reshape(-1, n_best)``; ``reference_groups``):
  MD       sum_i (s_i - t_i)^2                     (MSELoss(reduction="sum"); t = mlm_pll_score)
  MD_MWER  sum_g sum_i softmax(s + am)_i (cer_i - mean_g cer) + md_loss_weight * MD
  MD_MWED  sum_g KL(softmax(cer) || softmax((s + am) / T)) + md_loss_weight * MD,
           T = sum(s + am) / sum(cer) per group, differentiated through
Pinned against the reference's own training loop (tests/golden/make_golden_train.py, F6/F7:
losses, dev scores and parameter updates after two epochs, with dropout off as the fixtures
run it).  Dropout: the reference trains under ``model.train()`` with BertConfig's defaults
(hidden_dropout_prob = attention_probs_dropout_prob = 0.1), and so do these trainers by default
— hidden dropout after the embedding LayerNorm and on both residual branches, dropout on the
attention probabilities, inverted scaling, on every training step (not on the dev-loss pass).
The masks are counter-based draws (Philox4x32-10 keyed by ``dropout_seed`` and the trainer's
dropout-step counter, ``csrc/train.h``): bitwise reproducible, and exportable
(``dropout_keep``) so the tests feed the very same masks to the CPU oracle.  torch's RNG stream
itself cannot be matched, so a reference run with dropout is matched in distribution, not bits.

``MLMTrainer`` (BertForMaskedLM, decoder tied to the word embeddings) takes the reference's
padded batches (``pad_rows``: collate of MLM_PLL/main.py:28-54 — ids and labels padded with
0, pad positions are queries but not keys) and averages the CE over every position,
[PAD]-labelled pads included, as BertForMaskedLM's loss does there.  With ``ignore_index`` (-100,
the ``BertForMaskedLM(input_ids, labels)`` convention) the CE is the mean over the labelled positions
and the head runs on those rows only (``rs_train_step_mlm_labeled``); ``mask_tokens`` is the seeded
80/10/10 dynamic-masking collator that produces such labels.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .weights import BertShape, BERT_BASE


def param_shapes(shape: BertShape, head: str = "cls") -> Dict[str, Tuple[int, ...]]:
    """HF keys and shapes a trainer owns: RescoreBert without the unused pooler ("cls"), or
    BertForMaskedLM with its decoder tied to the word embeddings ("mlm")."""
    H, F = shape.hidden, shape.intermediate
    e = "bert.embeddings."
    out = {e + "word_embeddings.weight": (shape.vocab, H), e + "position_embeddings.weight": (shape.max_pos, H),
           e + "token_type_embeddings.weight": (shape.type_vocab, H), e + "LayerNorm.weight": (H,),
           e + "LayerNorm.bias": (H,)}
    for i in range(shape.layers):
        p = f"bert.encoder.layer.{i}."
        for n in ("query", "key", "value"):
            out[p + f"attention.self.{n}.weight"] = (H, H)
            out[p + f"attention.self.{n}.bias"] = (H,)
        out.update({p + "attention.output.dense.weight": (H, H), p + "attention.output.dense.bias": (H,),
                    p + "attention.output.LayerNorm.weight": (H,), p + "attention.output.LayerNorm.bias": (H,),
                    p + "intermediate.dense.weight": (F, H), p + "intermediate.dense.bias": (F,),
                    p + "output.dense.weight": (H, F), p + "output.dense.bias": (H,),
                    p + "output.LayerNorm.weight": (H,), p + "output.LayerNorm.bias": (H,)})
    if head == "mlm":
        c = "cls.predictions."
        out.update({c + "transform.dense.weight": (H, H), c + "transform.dense.bias": (H,),
                    c + "transform.LayerNorm.weight": (H,), c + "transform.LayerNorm.bias": (H,),
                    c + "bias": (shape.vocab,)})
    else:
        out["linear.weight"] = (1, H)
        out["linear.bias"] = (1,)
    return out


def prefix_matches(key: str, prefix: str) -> bool:
    """The rule ``freeze`` / ``unfreeze`` select tensors by (``rs_trainer_set_trainable``): whole dotted
    components, i.e. ``key`` equals ``prefix`` or starts with ``prefix + "."``; a trailing ``.`` of the
    prefix is ignored and an empty prefix matches nothing.  ``bert.encoder.layer.1`` selects layer 1 and
    not layer 10; the child names the reference's ``util/freezer.py`` takes (``bert``, ``linear``,
    ``cls``) work as they are."""
    prefix = prefix.rstrip(".")
    return bool(prefix) and (key == prefix or key.startswith(prefix + "."))


def lr_at(step: int, total_steps: int, warmup_steps: int, base_lr: float, schedule: str = "constant") -> float:
    """Learning rate of 0-based optimizer step ``step`` of a run of ``total_steps``: ``constant``, or
    ``linear``, the multiplier of transformers' ``get_linear_schedule_with_warmup`` (``step /
    max(1, warmup)`` below the warm-up, ``max(0, (total - step) / max(1, total - warmup))`` after)."""
    if schedule == "constant":
        return float(base_lr)
    if schedule != "linear":
        raise ValueError(f"unknown lr schedule {schedule!r} (constant, linear)")
    if step < warmup_steps:
        return float(base_lr) * (step / max(1, warmup_steps))
    return float(base_lr) * max(0.0, (total_steps - step) / max(1, total_steps - warmup_steps))


_SOURCES = {"last": 0, "accum": 1}


class _Trainer:
    HEAD = "cls"

    def __init__(self, weights: Dict[str, np.ndarray], shape: BertShape = BERT_BASE, device=0,
                 method: str = "MD", md_loss_weight: float = 1.0, lr: float = 1e-5, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.01, hidden_dropout: float = 0.1,
                 attn_dropout: float = 0.1, dropout_seed: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("librescore needs a HIP GPU (no CPU fallback)")
        self.lib = _lib.load()
        self.shape = shape
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index)
        torch.cuda.set_device(self.device)
        if method not in _lib.RS_LOSS:
            raise ValueError(f"unknown method {method!r} (MD, MD_MWER, MD_MWED)")
        self.method = method
        if not (0.0 <= hidden_dropout < 1.0 and 0.0 <= attn_dropout < 1.0):
            raise ValueError("dropout probabilities must be in [0, 1)")
        self.opts = _lib.RsTrainOpts(_lib.RS_LOSS[method], md_loss_weight, lr, betas[0], betas[1], eps,
                                     weight_decay, 1, hidden_dropout, attn_dropout, int(dropout_seed) & 0xFFFFFFFF)
        self.shapes = param_shapes(shape, self.HEAD)
        self.extra = {k: np.asarray(v) for k, v in weights.items()
                      if k.startswith("bert.pooler.") or (self.HEAD == "mlm" and k.startswith("cls.predictions.decoder."))}
        heads = _lib.RS_HEAD_CLS if self.HEAD == "cls" else _lib.RS_HEAD_MLM
        cfg = _lib.bert_cfg(shape, heads)
        h = ctypes.c_void_p()
        _lib.check(self.lib.rs_trainer_create(ctypes.byref(cfg), self.device.index, ctypes.byref(h)))
        self.handle = h
        try:
            # (only the trainer's own tensors: not e.g. an MLM head when initialising from BertForMaskedLM)
            _lib.upload_tensors(self.lib.rs_trainer_set_tensor, self.handle, weights, self.shapes)
            _lib.check(self.lib.rs_trainer_finalize(self.handle))
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rs_trainer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dropout_step(self) -> int:
        """Key (dropout-step counter) of the next training step that applies dropout."""
        return int(self.lib.rs_trainer_dropout_step(self.handle))

    def set_dropout_step(self, step: int) -> None:
        _lib.check(self.lib.rs_trainer_set_dropout_step(self.handle, int(step)))

    def reset_optimizer(self):
        """A fresh AdamW (moments and step count zeroed): the reference builds its optimizer
        inside every run_one_epoch (RescoreBert/main.py:83-86, MLM_PLL/main.py:74-77)."""
        _lib.check(self.lib.rs_trainer_reset_optimizer(self.handle))

    def _set_types(self, token_types, n_tok: int):
        """Segment ids of the NEXT step (``rs_trainer_set_token_types``): one per token row, values
        in ``[0, type_vocab)`` (``ValueError`` otherwise).  Returns the device tensor, which the
        caller keeps alive until the step has returned."""
        if token_types is None:
            return None
        tt = np.ascontiguousarray(np.asarray(token_types).reshape(-1), np.int32)
        if len(tt) != n_tok:
            raise ValueError(f"token_types needs one entry per token ({n_tok}), got {len(tt)}")
        tv = self.shape.type_vocab
        if len(tt) and (tt.min() < 0 or tt.max() >= tv):
            raise ValueError(f"token types must be in [0, {tv})")
        d_type = torch.as_tensor(tt).to(self.device)
        _lib.check(self.lib.rs_trainer_set_token_types(self.handle, _lib.ptr(d_type), len(tt)))
        return d_type

    @staticmethod
    def _update_flag(update) -> int:
        """True: backward + AdamW step; False: backward only; "loss": forward + loss only."""
        return -1 if update == "loss" else int(bool(update))

    def _get(self, fn, key: str) -> np.ndarray:
        shp = self.shapes[key]
        out = np.empty(shp, np.float32)
        _lib.check(fn(self.handle, key.encode(), out.ctypes.data, out.size))
        return out

    def tensor(self, key: str) -> np.ndarray:
        return self._get(self.lib.rs_trainer_get_tensor, key)

    def grad(self, key: str) -> Optional[np.ndarray]:
        """The last step's gradient of a tensor; ``None`` for a frozen one (torch's ``.grad``)."""
        if not self.is_trainable(key):
            return None
        return self._get(self.lib.rs_trainer_get_grad, key)

    def accum(self, key: str) -> Optional[np.ndarray]:
        """The accumulated (weighted sum of micro-batch) gradient of a tensor; ``None`` if frozen."""
        if not self.is_trainable(key):
            return None
        return self._get(self.lib.rs_trainer_get_accum, key)

    def _set_trainable(self, prefixes, flag: int) -> None:
        for p in prefixes:
            _lib.check(self.lib.rs_trainer_set_trainable(self.handle, str(p).encode(), flag))

    def freeze(self, *prefixes: str) -> None:
        """``requires_grad = False`` on every tensor a prefix selects (``prefix_matches``; the
        reference's ``util/freezer.py`` ``freeze_by_name``): no AdamW update or decay, no part in the
        gradient norm or the accumulation, and its gradient kernels are not launched.  On an MLM
        trainer ``cls`` holds the tied decoder, so it freezes the word embeddings too."""
        self._set_trainable(prefixes, 0)

    def unfreeze(self, *prefixes: str) -> None:
        self._set_trainable(prefixes, 1)

    def is_trainable(self, key: str) -> bool:
        rc = self.lib.rs_trainer_is_trainable(self.handle, key.encode())
        if rc < 0:
            _lib.check(rc)
        return bool(rc)

    def accumulate(self, weight: float = 1.0) -> None:
        """Adds ``weight`` times the last step's gradient (a ``step(update=False)``) to the accumulator."""
        _lib.check(self.lib.rs_trainer_accumulate(self.handle, float(weight), _lib.stream_ptr(self.device)))

    def zero_accum(self) -> None:
        _lib.check(self.lib.rs_trainer_zero_accum(self.handle))

    def grad_norm(self, source: str = "accum") -> float:
        """float64 L2 norm over the trainable tensors of the accumulator or the last gradient."""
        n = ctypes.c_double()
        _lib.check(self.lib.rs_trainer_grad_norm(self.handle, _SOURCES[source], ctypes.byref(n),
                                                 _lib.stream_ptr(self.device)))
        return n.value

    def apply(self, grad_scale: float = 1.0, max_grad_norm: Optional[float] = None, source: str = "accum",
              lr: Optional[float] = None) -> Tuple[float, bool]:
        """One AdamW step on ``grad_scale`` times the accumulator (or the last gradient), clipped to
        ``max_grad_norm`` like ``clip_grad_norm_``; ``lr`` overrides the trainer's for this step.
        Returns (the norm before clipping, whether the step was taken: a non-finite norm skips it)."""
        a = _lib.RsApplyOpts(_SOURCES[source], float(grad_scale), float(max_grad_norm or 0.0))
        o = _lib.RsTrainOpts.from_buffer_copy(self.opts)
        if lr is not None:
            o.lr = float(lr)
        n, ok = ctypes.c_double(), ctypes.c_int32()
        _lib.check(self.lib.rs_trainer_apply(self.handle, ctypes.byref(o), ctypes.byref(a), ctypes.byref(n),
                                             ctypes.byref(ok), _lib.stream_ptr(self.device)))
        return n.value, bool(ok.value)

    def state_dict(self) -> Dict[str, np.ndarray]:
        """HF-keyed weights (what the scorers load); the pooler passes through unchanged, the
        tied MLM decoder weight is the trained word-embedding matrix."""
        sd = {k: self.tensor(k) for k in self.shapes}
        sd.update(self.extra)
        if "cls.predictions.decoder.weight" in sd:
            sd["cls.predictions.decoder.weight"] = sd["bert.embeddings.word_embeddings.weight"]
        if "cls.predictions.decoder.bias" in sd:
            sd["cls.predictions.decoder.bias"] = sd["cls.predictions.bias"]
        return sd


class RescoreBertTrainer(_Trainer):
    HEAD = "cls"

    def step(self, tokens, hyp_off, utt_off, target, am=None, cer=None, update=True, token_types=None
             ) -> Tuple[float, np.ndarray]:
        """One step on a batch (RescoreBert/main.py:98-154): ``utt_off`` groups the hypotheses
        (``reference_groups``), ``target`` = mlm_pll_score, ``am`` = hyps_am_score, ``cer`` =
        hyps_cer.  ``update``: True (backward + AdamW), False (gradients only) or "loss"
        (forward only).  ``token_types``: one segment id per token (``data.with_context`` pairs).
        Returns (loss, CLS scores before the update)."""
        hoff = np.ascontiguousarray(hyp_off, np.int32)
        uoff = np.ascontiguousarray(utt_off, np.int32)
        n = len(hoff) - 1
        dev = self.device
        d_tok = torch.as_tensor(np.ascontiguousarray(tokens, np.int32)).to(dev)
        f32 = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float32)).to(dev)
        d_t, d_am, d_err = f32(target), f32(am), f32(cer)
        sc = torch.empty(n, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        self.opts.update = self._update_flag(update)
        d_type = self._set_types(token_types, int(hoff[-1]))      # noqa: F841
        _lib.check(self.lib.rs_train_step_cls(self.handle, _lib.ptr(d_tok), hoff.ctypes.data, n, uoff.ctypes.data,
                                              len(uoff) - 1, _lib.ptr(d_t), _lib.ptr(d_am), _lib.ptr(d_err),
                                              ctypes.byref(self.opts), _lib.ptr(sc), _lib.ptr(loss),
                                              _lib.stream_ptr(dev)))
        return float(loss.item()), sc.cpu().numpy()


def do_job_rows(hyps: Sequence[Sequence[int]], mask_id: int = 103):
    """MLM_PLL/preprocess.py:9-30 rows of [CLS] w.. [SEP] sequences: one [MASK] per word
    position; labels = the unmasked sequence.  Returns (ids, seq_off, labels) ragged int32."""
    ids, labels, off = [], [], [0]
    for h in hyps:
        h = list(h)
        for p in range(1, len(h) - 1):
            row = h.copy()
            row[p] = mask_id
            ids.extend(row)
            labels.extend(h)
            off.append(off[-1] + len(h))
    return np.asarray(ids, np.int32), np.asarray(off, np.int32), np.asarray(labels, np.int32)


def reference_groups(n_rows: int, n_best: int) -> np.ndarray:
    """Group offsets of a RescoreBert training batch: consecutive runs of ``n_best`` rows, as
    ``mix_score.reshape(-1, config.n_best)`` forms them (RescoreBert/main.py:116,132)."""
    if n_best <= 0 or n_rows % n_best:
        raise ValueError(f"batch of {n_rows} hypotheses does not reshape to (-1, {n_best})")
    return np.arange(0, n_rows + 1, n_best, dtype=np.int32)


def pad_rows(seqs: Sequence[Sequence[int]], labels: Sequence[Sequence[int]], types=None, label_pad: int = 0):
    """The reference's MLM batch (collate, MLM_PLL/main.py:28-54): every row padded to the
    batch's longest with id 0 and label 0 (pad_sequence); the attention mask's zeros become
    key lengths.  Returns (ids, row_off, labels, key_len) as int32, and with ``types`` (a segment-id
    row per sequence) a fifth item, the types padded with 0 like the ids.  ``label_pad``: the value
    that pads the labels (the ``ignore_index`` of a labelled step, so that pads carry no label)."""
    T = max(len(x) for x in seqs)
    n = len(seqs)
    ids = np.zeros((n, T), np.int32)
    lab = np.full((n, T), label_pad, np.int32)
    klen = np.empty(n, np.int32)
    for i, (x, y) in enumerate(zip(seqs, labels)):
        ids[i, :len(x)] = x
        lab[i, :len(y)] = y
        klen[i] = len(x)
    out = (ids.ravel(), np.arange(0, n * T + 1, T, dtype=np.int32), lab.ravel(), klen)
    if types is None:
        return out
    tt = np.zeros((n, T), np.int32)
    for i, t in enumerate(types):
        tt[i, :len(t)] = t
    return out + (tt.ravel(),)


def labelled_rows(labels, ignore_index: int, vocab: int, n_tok: int) -> Tuple[np.ndarray, np.ndarray]:
    """The labelled positions of a labels array with one entry per token row (``ignore_index``, the
    -100 of ``BertForMaskedLM(input_ids, labels)``, marks a position without a label): (row indices,
    ascending; label ids) as int32, the ``h_lab_row`` / ``d_lab_id`` of ``rs_train_step_mlm_labeled``.
    ``ValueError`` for a label count other than ``n_tok``, any other label outside ``[0, vocab)``, and
    no labelled position at all (HF's loss is NaN there)."""
    lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), np.int32)
    if len(lab) != n_tok:
        raise ValueError(f"labels needs one entry per token ({n_tok}), got {len(lab)}")
    rows = np.flatnonzero(lab != ignore_index).astype(np.int32)
    if len(rows) == 0:
        raise ValueError(f"no labelled position: every label is ignore_index ({ignore_index})")
    ids = np.ascontiguousarray(lab[rows])
    if ids.min() < 0 or ids.max() >= vocab:
        bad = int(rows[np.flatnonzero((ids < 0) | (ids >= vocab))[0]])
        raise ValueError(f"label {int(lab[bad])} at position {bad} is neither ignore_index ({ignore_index}) "
                         f"nor in [0, {vocab})")
    return rows, ids


class MLMTrainer(_Trainer):
    """MLM fine-tuning (MLM_PLL/main.py:73-161): BertForMaskedLM, CE over every position of the
    (padded) rows, mean; AdamW.  ``key_len`` marks each row's padding (``pad_rows``); without
    it the rows are ragged and every position is real.  With ``ignore_index`` (normally -100) the
    labels follow ``BertForMaskedLM(input_ids, labels)``: positions labelled ``ignore_index`` carry no
    loss, the CE is the mean over the others, and the head (transform + tied decoder) runs on those
    rows only (``rs_train_step_mlm_labeled``)."""
    HEAD = "mlm"

    def step(self, ids, seq_off, labels, key_len=None, update=True, token_types=None,
             ignore_index: Optional[int] = None) -> float:
        off = np.ascontiguousarray(seq_off, np.int32)
        kl = None if key_len is None else np.ascontiguousarray(key_len, np.int32)
        if kl is not None and len(kl) != len(off) - 1:
            raise ValueError("key_len needs one entry per row")
        dev = self.device
        rows = None
        if ignore_index is not None:
            rows, labels = labelled_rows(labels, int(ignore_index), self.shape.vocab, int(off[-1]))
        d_ids = torch.as_tensor(np.ascontiguousarray(ids, np.int32)).to(dev)
        d_lab = torch.as_tensor(np.ascontiguousarray(labels, np.int32)).to(dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        self.opts.update = self._update_flag(update)
        d_type = self._set_types(token_types, int(off[-1]))      # noqa: F841
        klp = None if kl is None else kl.ctypes.data
        if rows is None:
            _lib.check(self.lib.rs_train_step_mlm(self.handle, _lib.ptr(d_ids), off.ctypes.data, len(off) - 1, klp,
                                                  _lib.ptr(d_lab), ctypes.byref(self.opts), _lib.ptr(loss),
                                                  _lib.stream_ptr(dev)))
        else:
            _lib.check(self.lib.rs_train_step_mlm_labeled(self.handle, _lib.ptr(d_ids), off.ctypes.data, len(off) - 1,
                                                          klp, rows.ctypes.data, len(rows), _lib.ptr(d_lab),
                                                          ctypes.byref(self.opts), _lib.ptr(loss),
                                                          _lib.stream_ptr(dev)))
        return float(loss.item())


class _Grouped:
    """The optimizer side of an epoch helper.  With the defaults (``accum_steps`` 1, no clipping, no
    schedule) a batch is one ``tr.step(update=update)``, as it always was.  Otherwise (training
    passes only) every batch runs ``step(update=False)`` + ``accumulate(w)`` and each group of
    ``accum_steps`` consecutive batches (the last may be shorter) ends in one ``apply`` with
    ``grad_scale`` = 1 (``mean`` False: summed losses) or 1 / sum of the weights (``mean`` True), at
    the lr ``lr_of_step`` gives for the run's 0-based optimizer step."""

    def __init__(self, tr: _Trainer, update, accum_steps: int, max_grad_norm, lr_of_step, mean: bool):
        if accum_steps < 1:
            raise ValueError("accum_steps must be at least 1")
        self.tr, self.k, self.clip, self.lr_of, self.mean = tr, int(accum_steps), max_grad_norm, lr_of_step, mean
        self.plain = update is not True or (self.k == 1 and max_grad_norm is None and lr_of_step is None)
        self.update = update if self.plain else False
        self.n, self.wsum, self.opt_step = 0, 0.0, 0

    def after_step(self, weight: float, last: bool) -> None:
        if self.plain:
            return
        self.tr.accumulate(weight)
        self.n += 1
        self.wsum += weight
        if self.n == self.k or last:
            self.tr.apply(grad_scale=1.0 / self.wsum if self.mean else 1.0, max_grad_norm=self.clip,
                          lr=None if self.lr_of is None else self.lr_of(self.opt_step))
            self.n, self.wsum = 0, 0.0
            self.opt_step += 1


def rescorebert_epoch(tr: RescoreBertTrainer, tokens, hyp_off, target, am, cer, batch_size: int, n_best: int,
                      update=True, token_types=None, accum_steps: int = 1, max_grad_norm: Optional[float] = None,
                      lr_of_step=None) -> float:
    """One pass of RescoreBert/main.py:82-163 run_one_epoch(train=True) over the hypotheses in
    order: batches of ``batch_size * n_best`` rows (set_dataloader :71-79, shuffle False),
    groups of ``n_best`` (``reference_groups``) for MD_MWER / MD_MWED, which reshape the batch
    to (-1, n_best) (RescoreBert/main.py:116,132); MD is a plain MSELoss(sum) over the batch
    (:104-110) and takes any batch, ragged last batch and short N-best lists included;
    ``update`` True = grad_update (the caller resets AdamW first, as the reference builds it per
    call), "loss" = the dev pass.  ``token_types``: per-token segment ids, sliced with the tokens.
    ``accum_steps`` / ``max_grad_norm`` / ``lr_of_step`` (``_Grouped``): the losses are sums over
    utterances, so k accumulated micro-batches (weight 1, scale 1) are the one batch holding all of them.
    Returns the epoch loss (mean of the batch losses)."""
    hoff = np.asarray(hyp_off, np.int64)
    n = len(hoff) - 1
    rows = batch_size * n_best
    tot, nb = 0.0, 0
    grp = _Grouped(tr, update, accum_steps, max_grad_norm, lr_of_step, mean=False)
    update = grp.update
    for b0 in range(0, n, rows):
        b1 = min(n, b0 + rows)
        t0, t1 = int(hoff[b0]), int(hoff[b1])
        groups = np.array([0, b1 - b0], np.int32) if tr.method == "MD" else reference_groups(b1 - b0, n_best)
        loss, _ = tr.step(np.asarray(tokens[t0:t1]), (hoff[b0:b1 + 1] - t0).astype(np.int32),
                          groups, target[b0:b1], am[b0:b1], cer[b0:b1], update=update,
                          token_types=None if token_types is None else np.asarray(token_types[t0:t1]))
        grp.after_step(1.0, b1 == n)
        tot += loss
        nb += 1
    return tot / max(nb, 1)


def mlm_epoch(tr: MLMTrainer, seqs: Sequence[Sequence[int]], labels: Sequence[Sequence[int]], batch_size: int,
              update=True, order=None, token_types=None, ignore_index: Optional[int] = None, accum_steps: int = 1,
              max_grad_norm: Optional[float] = None, lr_of_step=None) -> float:
    """One pass of MLM_PLL/main.py:73-114 run_one_epoch (do_scoring False) over do_job rows:
    batches of ``batch_size`` rows (in ``order``, default as given), padded as the reference's
    collate pads them (``pad_rows``).  ``token_types``: a segment-id row per sequence, padded with
    the ids.  ``ignore_index``: labels equal to it carry no loss (``MLMTrainer.step``); the labels are
    then padded with it, so every batch needs a labelled position.  ``accum_steps`` / ``max_grad_norm``
    / ``lr_of_step`` (``_Grouped``): a batch is weighted by its number of loss positions and the group
    scaled by 1 / their sum, the CE mean over the group.  Returns the epoch loss (mean of the batch
    losses)."""
    idx = np.arange(len(seqs)) if order is None else np.asarray(order)
    tot, nb = 0.0, 0
    grp = _Grouped(tr, update, accum_steps, max_grad_norm, lr_of_step, mean=True)
    update = grp.update
    for b0 in range(0, len(idx), batch_size):
        sel = idx[b0:b0 + batch_size]
        tt = None if token_types is None else [token_types[i] for i in sel]
        ids, off, lab, klen, *typ = pad_rows([seqs[i] for i in sel], [labels[i] for i in sel], tt,
                                             label_pad=0 if ignore_index is None else ignore_index)
        tot += tr.step(ids, off, lab, klen, update=update, token_types=typ[0] if typ else None,
                       ignore_index=ignore_index)
        grp.after_step(float(len(lab) if ignore_index is None else np.count_nonzero(lab != ignore_index)),
                       b0 + batch_size >= len(idx))
        nb += 1
    return tot / max(nb, 1)


def mask_tokens(seqs: Sequence[Sequence[int]], shape: BertShape, seed, mlm_probability: float = 0.15,
                continuation: Optional[Sequence[Sequence[int]]] = None
                ) -> Tuple[List[List[int]], List[List[int]]]:
    """Dynamic MLM masking of ``[CLS] w.. [SEP]`` rows: the rule of transformers'
    ``DataCollatorForLanguageModeling.torch_mask_tokens`` on ragged rows, drawn from
    ``np.random.Generator(PCG64(seed))`` (``seed``: an int or a sequence of ints such as
    ``(seed, step)``; torch's Bernoulli stream is not reproduced, the rule is).  Position 0 and the
    last position of each row and any ``[PAD]`` are never selected; every other position is selected
    with ``mlm_probability``; of the selected, 80 % become ``shape.mask_id``, 10 % a uniform id in
    ``[0, vocab)`` and 10 % stay.  ``continuation`` (a 0/1 row per sequence, 1 = a ``##`` piece as
    ``rs_vocab_continuation`` marks it): the selection is drawn per word and covers all its pieces
    (whole-word masking); the 80/10/10 draw stays per position.  A call that selects nothing selects
    the eligible position (word) with the smallest draw, so every batch has a label; rows without
    any eligible position raise ``ValueError``.  Returns (masked rows, label rows): labels are the
    original id at the selected positions and -100 elsewhere."""
    if not 0.0 < mlm_probability <= 1.0:
        raise ValueError("mlm_probability must be in (0, 1]")
    rng = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray([len(s) for s in seqs], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = np.concatenate([np.asarray(s, np.int64).reshape(-1) for s in seqs]) if len(seqs) else np.zeros(0, np.int64)
    elig = flat != shape.pad_id
    nz = lens > 0
    elig[off[:-1][nz]] = False
    elig[off[1:][nz] - 1] = False
    if continuation is None:
        starts = np.ones(len(flat), bool)
    else:
        cont = np.concatenate([np.asarray(c, np.int64).reshape(-1) for c in continuation])
        if len(cont) != len(flat):
            raise ValueError("continuation needs one entry per token")
        starts = cont == 0
    # a unit (position, or word) begins at an eligible position that starts a word or follows an
    # ineligible one; rows are separated by their ineligible first and last positions
    prev = np.zeros(len(flat), bool)
    prev[1:] = elig[:-1]
    ustart = elig & (starts | ~prev)
    n_unit = int(ustart.sum())
    if n_unit == 0:
        raise ValueError("no eligible position (every row is [CLS] [SEP] or padding)")
    unit = np.maximum(np.cumsum(ustart) - 1, 0)
    u = rng.random(n_unit)
    pick = u < mlm_probability
    if not pick.any():
        pick[int(np.argmin(u))] = True
    sel = np.flatnonzero(elig & pick[unit])
    v = rng.random(len(sel))
    rid = rng.integers(0, shape.vocab, len(sel))
    out = flat.copy()
    out[sel] = np.where(v < 0.8, shape.mask_id, np.where(v < 0.9, rid, flat[sel]))
    lab = np.full(len(flat), -100, np.int64)
    lab[sel] = flat[sel]
    return ([out[off[i]:off[i + 1]].tolist() for i in range(len(seqs))],
            [lab[off[i]:off[i + 1]].tolist() for i in range(len(seqs))])


def mlm_epoch_dynamic(tr: MLMTrainer, sentences: Sequence[Sequence[int]], batch_size: int, seed: Sequence[int],
                      update=True, order=None, mlm_probability: float = 0.15, continuation=None, accum_steps: int = 1,
                      max_grad_norm: Optional[float] = None, lr_of_step=None) -> float:
    """One pass over ``[CLS] w.. [SEP]`` rows (one per sentence) with dynamic masking: batch b (of
    ``batch_size`` rows, in ``order``) is masked by ``mask_tokens`` seeded ``(*seed, b)``, so every
    batch has a labelled position and a pass is a function of ``seed`` alone; labelled steps
    (``ignore_index`` -100); ``accum_steps`` / ``max_grad_norm`` / ``lr_of_step`` as ``mlm_epoch``.
    Returns the epoch loss (mean of the batch losses)."""
    idx = np.arange(len(sentences)) if order is None else np.asarray(order)
    tot, nb = 0.0, 0
    grp = _Grouped(tr, update, accum_steps, max_grad_norm, lr_of_step, mean=True)
    update = grp.update
    for b0 in range(0, len(idx), batch_size):
        sel = idx[b0:b0 + batch_size]
        rows, labs = mask_tokens([sentences[i] for i in sel], tr.shape, tuple(seed) + (nb,), mlm_probability,
                                 None if continuation is None else [continuation[i] for i in sel])
        ids, off, lab, klen = pad_rows(rows, labs, label_pad=-100)
        tot += tr.step(ids, off, lab, klen, update=update, ignore_index=-100)
        grp.after_step(float(np.count_nonzero(lab != -100)), b0 + batch_size >= len(idx))
        nb += 1
    return tot / max(nb, 1)


def dropout_keep(seed: int, step: int, site: int, p: float, n: int, device=0) -> np.ndarray:
    """The keep bits (uint8 [n]) the trainer's kernels use for element e of dropout site
    ``site`` in dropout step ``step`` (``csrc/train.h``: 0 = embeddings; layer l: 1 + 3l
    attention probabilities in the saved-P layout, 2 + 3l self-output, 3 + 3l output, element
    = row * hidden + column), generated by the same device function."""
    lib = _lib.load()
    dev = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index)
    out = torch.empty(max(int(n), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.rs_dropout_keep(int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(site), float(p), int(n),
                                   _lib.ptr(out), _lib.stream_ptr(dev)))
    return out[:int(n)].cpu().numpy()


def finetune_mlm_on_texts(weights: Dict[str, np.ndarray], sentences: Sequence[Sequence[int]],
                          shape: BertShape = BERT_BASE, steps: int = 300, batch_size: int = 64,
                          lr: float = 1e-4, seed: int = 0, device=0, dropout: float = 0.0,
                          log_every: int = 0, masking: str = "do_job", mlm_probability: float = 0.15,
                          continuation=None) -> Tuple[Dict[str, np.ndarray], List[float]]:
    """MLM fine-tuning on in-domain text, then scoring with the result: the reference's
    pipeline (MLM_PLL/main.py:117-161 mlm_finetune_bert -> :184-186 scoring with that checkpoint ->
    rescore.py:25-45 fusion).  ``sentences`` are word-id lists (no [CLS]/[SEP]); their do_job rows
    (MLM_PLL/preprocess.py:9-30) are visited in a seeded permutation per epoch, ``batch_size``
    padded rows per step (collate, MLM_PLL/main.py:28-54), for ``steps`` AdamW steps.
    Deterministic (native trainer, bitwise reproducible; dropout off by default).  Returns the
    HF-keyed state dict (loadable by the scorers) and the per-step losses.
    ``masking``: "do_job" (default) is the reference's batch, a label at every position, pads
    included; "do_job_masked" the same rows labelled at their [MASK] only (-100 elsewhere, the head
    over ``batch_size`` rows); "dynamic" one row per sentence, re-masked every step by
    ``mask_tokens`` seeded with ``(seed, step)`` (``mlm_probability``; ``continuation``: a 0/1 list
    per sentence, without [CLS]/[SEP], for whole-word masking)."""
    if masking not in ("do_job", "do_job_masked", "dynamic"):
        raise ValueError(f"unknown masking {masking!r} (do_job, do_job_masked, dynamic)")
    seqs, labels = [], []
    for s in sentences:
        h = [shape.cls_id] + [int(x) for x in s] + [shape.sep_id]
        if masking == "dynamic":
            seqs.append(h)
            continue
        for p in range(1, len(h) - 1):
            row = list(h)
            row[p] = shape.mask_id
            seqs.append(row)
            labels.append(h if masking == "do_job" else [-100] * p + [h[p]] + [-100] * (len(h) - p - 1))
    cont = None if continuation is None or masking != "dynamic" else [[0] + [int(x) for x in c] + [0]
                                                                      for c in continuation]
    tr = MLMTrainer(weights, shape, device=device, lr=lr, hidden_dropout=dropout, attn_dropout=dropout,
                    dropout_seed=seed)
    try:
        rng = np.random.Generator(np.random.PCG64(seed))
        order = np.empty(0, np.int64)
        losses: List[float] = []
        for it in range(steps):
            if len(order) < batch_size:
                order = np.concatenate([order, rng.permutation(len(seqs))])
            sel, order = order[:batch_size], order[batch_size:]
            if masking == "do_job":
                ids, off, lab, klen = pad_rows([seqs[i] for i in sel], [labels[i] for i in sel])
                losses.append(tr.step(ids, off, lab, klen))
            else:
                rows, labs = [seqs[i] for i in sel], [labels[i] for i in sel] if labels else None
                if masking == "dynamic":
                    rows, labs = mask_tokens(rows, shape, (seed, it), mlm_probability,
                                             None if cont is None else [cont[i] for i in sel])
                ids, off, lab, klen = pad_rows(rows, labs, label_pad=-100)
                losses.append(tr.step(ids, off, lab, klen, ignore_index=-100))
            if log_every and (it + 1) % log_every == 0:
                print(f"finetune step {it + 1}/{steps} loss {losses[-1]:.4f}", flush=True)
        return tr.state_dict(), losses
    finally:
        tr.close()
