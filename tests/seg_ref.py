"""CPU reference with segment ids (test infrastructure only): a self-contained torch float64 BERT
with per-token ``token_type_ids``.  The expressions are those of ``oracle/bert_ref.py`` (which
restates transformers' ``modeling_bert.py``: BertEmbeddings, eager attention, BertSelfOutput,
BertIntermediate with erf GELU, BertOutput, BertPredictionHeadTransform, the tied decoder) with the
type lookup ``token_type_embeddings.weight[token_type_ids]`` in place of row 0.
``tests/test_seg_ref.py`` pins it against that oracle at all-zero types and against transformers
under random types.

Provides the MLM log-softmax rows of span-masked copies, the RescoreBert CLS score, the last hidden
states, and the MD / MD_MWER / MLM training losses with autograd.
"""
from typing import Dict, List, Sequence

import numpy as np
import torch
import torch.nn.functional as Fn


class SegBert:
    """float64 BERT from an HF-keyed weight dict; ``grad``: every parameter a leaf with a gradient."""

    def __init__(self, weights: Dict[str, np.ndarray], shape, grad: bool = False):
        self.s = shape
        self.w = {k: torch.from_numpy(np.array(v, np.float64, copy=True)) for k, v in weights.items()
                  if not k.startswith("cls.predictions.decoder.")}
        if grad:
            for t in self.w.values():
                t.requires_grad_(True)

    def _lin(self, x, key):
        return Fn.linear(x, self.w[key + ".weight"], self.w[key + ".bias"])

    def _ln(self, x, key):
        return Fn.layer_norm(x, (self.s.hidden,), self.w[key + ".weight"], self.w[key + ".bias"], eps=self.s.ln_eps)

    def encoder(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids: torch.Tensor):
        """int64 [B, T] ids, mask and types -> last hidden [B, T, H]."""
        s = self.s
        B, T = input_ids.shape
        e = "bert.embeddings."
        x = (Fn.embedding(input_ids, self.w[e + "word_embeddings.weight"], padding_idx=s.pad_id)
             + Fn.embedding(token_type_ids, self.w[e + "token_type_embeddings.weight"])
             + self.w[e + "position_embeddings.weight"][torch.arange(T)][None])
        x = self._ln(x, e + "LayerNorm")
        add = (1.0 - attention_mask[:, None, None, :].to(x.dtype)) * torch.finfo(x.dtype).min
        nh, hd = s.heads, s.head_dim
        for i in range(s.layers):
            p = f"bert.encoder.layer.{i}."
            q = self._lin(x, p + "attention.self.query").view(B, T, nh, hd).transpose(1, 2)
            k = self._lin(x, p + "attention.self.key").view(B, T, nh, hd).transpose(1, 2)
            v = self._lin(x, p + "attention.self.value").view(B, T, nh, hd).transpose(1, 2)
            pr = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * (hd ** -0.5) + add, dim=-1)
            ctx = torch.matmul(pr, v).transpose(1, 2).reshape(B, T, s.hidden)
            x = self._ln(self._lin(ctx, p + "attention.output.dense") + x, p + "attention.output.LayerNorm")
            it = Fn.gelu(self._lin(x, p + "intermediate.dense"))
            x = self._ln(self._lin(it, p + "output.dense") + x, p + "output.LayerNorm")
        return x

    def mlm_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        c = "cls.predictions."
        t = self._ln(Fn.gelu(self._lin(hidden, c + "transform.dense")), c + "transform.LayerNorm")
        return Fn.linear(t, self.w["bert.embeddings.word_embeddings.weight"], self.w[c + "bias"])

    def cls_score(self, hidden: torch.Tensor) -> torch.Tensor:
        return Fn.linear(hidden[:, 0, :], self.w["linear.weight"], self.w["linear.bias"]).squeeze(-1)


def pad(rows: Sequence[Sequence[int]]) -> torch.Tensor:
    T = max(len(r) for r in rows)
    out = torch.zeros(len(rows), T, dtype=torch.long)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.as_tensor(np.asarray(r, np.int64))
    return out


def _split(a, off) -> List[np.ndarray]:
    return [np.asarray(a[off[h]:off[h + 1]]) for h in range(len(off) - 1)]


def _batch(seqs, types):
    return pad(seqs), pad([[1] * len(s) for s in seqs]), pad(types)


def span_rows(model: SegBert, tokens, hyp_off, types, row_off, lo, hi, query, batch: int = 64) -> np.ndarray:
    """log_softmax rows float64 [R, vocab] of the span-masked copies (``rs_pll_score_spans`` rows):
    row r of hypothesis h has positions [lo[r], hi[r]) set to [MASK] — the types stay those of the
    positions — and is read at query[r]."""
    seqs, tys = _split(tokens, hyp_off), _split(types, hyp_off)
    hyp = np.repeat(np.arange(len(seqs)), np.diff(row_off))
    out = []
    with torch.no_grad():
        for b0 in range(0, len(lo), batch):
            rs = range(b0, min(len(lo), b0 + batch))
            ids = []
            for r in rs:
                x = seqs[hyp[r]].copy()
                x[lo[r]:hi[r]] = model.s.mask_id
                ids.append(x)
            x, am, tt = _batch(ids, [tys[hyp[r]] for r in rs])
            hid = model.encoder(x, am, tt)
            q = [int(query[r]) for r in rs]
            out.append(model.mlm_logits(hid[list(range(len(q))), q, :]).log_softmax(dim=-1))
    return torch.cat(out).numpy() if out else np.zeros((0, model.s.vocab))


def row_logprobs(lsm: np.ndarray, tokens, hyp_off, row_off, query) -> np.ndarray:
    """The label log-prob of every row of ``span_rows`` (label = the token at the query position)."""
    hyp = np.repeat(np.arange(len(hyp_off) - 1), np.diff(row_off))
    lab = np.asarray(tokens)[np.asarray(hyp_off)[hyp] + np.asarray(query)]
    return lsm[np.arange(len(lab)), lab]


def sum_rows(rows, row_off) -> np.ndarray:
    return np.asarray([float(np.sum(rows[row_off[h]:row_off[h + 1]])) for h in range(len(row_off) - 1)])


def hidden_states(model: SegBert, tokens, hyp_off, types, batch: int = 64) -> List[np.ndarray]:
    """Last hidden state [T_h, H] of every hypothesis."""
    seqs, tys = _split(tokens, hyp_off), _split(types, hyp_off)
    out = []
    with torch.no_grad():
        for b0 in range(0, len(seqs), batch):
            hid = model.encoder(*_batch(seqs[b0:b0 + batch], tys[b0:b0 + batch]))
            out += [hid[i, :len(s)].numpy() for i, s in enumerate(seqs[b0:b0 + batch])]
    return out


def cls_scores(model: SegBert, tokens, hyp_off, types) -> np.ndarray:
    seqs, tys = _split(tokens, hyp_off), _split(types, hyp_off)
    with torch.no_grad():
        return model.cls_score(model.encoder(*_batch(seqs, tys))).numpy()


def rescorebert_loss(sc: torch.Tensor, target, am, cer, n_best: int, method: str, md_loss_weight: float):
    """RescoreBert/main.py:104-147 (MD, MD_MWER) in float64."""
    md = torch.sum((sc - torch.as_tensor(np.asarray(target, np.float64))) ** 2)
    if method == "MD":
        return md
    if method != "MD_MWER":
        raise ValueError(method)
    c = torch.as_tensor(np.asarray(cer, np.float64)).reshape(-1, n_best)
    p = torch.softmax((sc + torch.as_tensor(np.asarray(am, np.float64))).reshape(-1, n_best), dim=-1)
    avg = (torch.sum(c, dim=-1) / n_best).unsqueeze(dim=-1)
    return torch.sum(p * (c - avg)) + md_loss_weight * md


def _grads(model: SegBert, keys) -> Dict[str, np.ndarray]:
    return {k: (model.w[k].grad if model.w[k].grad is not None else torch.zeros_like(model.w[k])).numpy()
            for k in keys}


def cls_step(weights, shape, tokens, hyp_off, types, target, am, cer, n_best, method, md_loss_weight, keys):
    """(loss, scores, {key: gradient}) of one RescoreBert training batch, autograd in float64."""
    m = SegBert(weights, shape, grad=True)
    sc = m.cls_score(m.encoder(*_batch(_split(tokens, hyp_off), _split(types, hyp_off))))
    loss = rescorebert_loss(sc, target, am, cer, n_best, method, md_loss_weight)
    loss.backward()
    return float(loss.detach()), sc.detach().numpy(), _grads(m, keys)


def mlm_step(weights, shape, ids, seq_off, types, labels, keys):
    """(loss, {key: gradient}) of one ragged MLM batch: cross entropy, mean over every position."""
    m = SegBert(weights, shape, grad=True)
    seqs = _split(ids, seq_off)
    x, am, tt = _batch(seqs, _split(types, seq_off))
    logits = m.mlm_logits(m.encoder(x, am, tt))
    keep = am.bool()
    loss = Fn.cross_entropy(logits[keep], pad(_split(labels, seq_off))[keep])
    loss.backward()
    return float(loss.detach()), _grads(m, keys)
