"""Drop-in scorers backed by librescore (HIP, gfx950).

* ``PLLScorer`` — MLM_PLL.  ``score_nbest`` replaces the per-hypothesis accumulation of
  ``run_one_epoch(do_scoring=True)`` (MLM_PLL/main.py:73-114) over the rows of
  ``do_job`` (MLM_PLL/preprocess.py:9-30); ``masked_logprob`` replaces the row-level
  ``token_score`` (MLM_PLL/main.py:89-105) for any padded batch; ``run_one_epoch``
  mirrors the reference function's signature and ``output_score`` update.
* ``RescoreBertHIP`` — ``torch.nn.Module`` with the forward signature of
  ``RescoreBert`` (RescoreBert/model.py:13-21).

Tensors cross the C ABI as device pointers on ``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from .data import NBest, PLL_VARIANTS, pll_spans, pll_strided
from .weights import BertShape, BERT_BASE


def _prefix_lengths(attention_mask: torch.Tensor) -> np.ndarray:
    """Row lengths of a right-padded 0/1 attention mask (``pad_sequence`` output).

    A left-padded, holed or non-binary mask would make the ragged scorers score other
    tokens than the reference's additive-mask forward, so it is rejected."""
    am = attention_mask.detach().to("cpu", torch.int64)
    if am.dim() != 2:
        raise ValueError("attention_mask must be [B, T]")
    if not bool(((am == 0) | (am == 1)).all()):
        raise ValueError("attention_mask must hold only 0 and 1")
    lens = am.sum(-1)
    pos = torch.arange(am.shape[1])[None, :]
    if not bool((am.bool() == (pos < lens[:, None])).all()):
        raise ValueError("attention_mask must be prefix ones (right padding)")
    return lens.numpy().astype(np.int32)


class BertEngine:
    """One ``rs_model`` handle: packed weights + workspace on one GPU."""

    def __init__(self, weights: Dict[str, np.ndarray], shape: BertShape = BERT_BASE,
                 heads: int = _lib.RS_HEAD_MLM, device: int | str | torch.device = 0,
                 max_rows: int = 65536, precision: str = "fp16x3"):
        if not torch.cuda.is_available():
            raise RuntimeError("librescore needs a HIP GPU (no CPU fallback)")
        self.lib = _lib.load()
        self.shape = shape
        self.device = torch.device("cuda", torch.device(device).index if not isinstance(device, int)
                                   else device)
        torch.cuda.set_device(self.device)
        cfg = _lib.bert_cfg(shape, heads, precision)
        self.precision = precision
        h = ctypes.c_void_p()
        _lib.check(self.lib.rs_model_create(ctypes.byref(cfg), self.device.index, ctypes.byref(h)))
        self.handle = h
        try:
            _lib.upload_tensors(self.lib.rs_model_set_tensor, self.handle, weights)
            _lib.check(self.lib.rs_model_finalize(self.handle))
            _lib.check(self.lib.rs_model_reserve(self.handle, int(max_rows)))
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rs_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- deferred range / timeout check (rs_model_set_sync_check, rs_check) -------------
    def set_sync_check(self, on: bool = True):
        """False: scoring calls stay asynchronous on the current stream and their non-finite /
        statistics-timeout flags accumulate until ``check()``; True (default): every call
        synchronises and raises on its own flags."""
        _lib.check(self.lib.rs_model_set_sync_check(self.handle, int(on)))

    def check(self):
        """Synchronise the current stream and raise if any deferred call flagged an error."""
        _lib.check(self.lib.rs_check(self.handle, _lib.stream_ptr(self.device)))

    # ---- profiling (HIP events per kernel kind) ----------------------------------------
    def profile(self, on: bool = True):
        _lib.check(self.lib.rs_profile_enable(self.handle, int(on)))

    def profile_read(self) -> Dict[str, Tuple[float, int, float]]:
        out = {}
        for i, name in enumerate(_lib.KINDS):
            ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
            _lib.check(self.lib.rs_profile_read(self.handle, i, ctypes.byref(ms), ctypes.byref(n),
                                                ctypes.byref(fl)))
            out[name] = (ms.value, n.value, fl.value)
        return out

    def _dev_tokens(self, tokens) -> torch.Tensor:
        if isinstance(tokens, torch.Tensor):
            return tokens.to(self.device, torch.int32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(tokens, np.int32)).to(self.device)

    def _hyps(self, tokens, hyp_off):
        """A ragged hypothesis list as the C ABI takes it: (device tokens, int32 offsets, count)."""
        off = np.ascontiguousarray(hyp_off, np.int32)
        return self._dev_tokens(tokens), off, len(off) - 1

    # ---- segment ids (rs_model_set_token_types) ----------------------------------------
    def _set_types(self, token_types):
        """Hands ``token_types`` (one segment id per token of the NEXT scoring call, array or tensor;
        None: nothing set, every token type 0) to the handle.  Values outside ``[0, type_vocab)``
        raise ``ValueError`` here (the device would clamp them); a length that differs from the
        call's token count makes that call fail (RS_EARG).  Returns the device tensor, which the
        caller keeps alive until its call has returned."""
        if token_types is None:
            return None
        d_type = self._dev_tokens(token_types).reshape(-1)
        if d_type.numel():
            lo, hi = int(d_type.min()), int(d_type.max())
            if lo < 0 or hi >= self.shape.type_vocab:
                raise ValueError(f"token types must be in [0, {self.shape.type_vocab}), got {lo if lo < 0 else hi}")
        _lib.check(self.lib.rs_model_set_token_types(self.handle, _lib.ptr(d_type), d_type.numel()))
        return d_type

    def clear_token_types(self):
        """Drops a pending segment-id setting (``rs_model_set_token_types(NULL)``)."""
        _lib.check(self.lib.rs_model_set_token_types(self.handle, None, 0))


def _ragged(input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids, device):
    """Ragged copy of a right-padded [B, T] batch, the unpadded prefix of each row (device gather,
    no host round trip): (ids int32 [sum len], row offsets int32 [B + 1], types like ids or None)."""
    lens = _prefix_lengths(attention_mask)
    ids = input_ids.to(device)
    keep = torch.arange(ids.shape[1], device=device)[None, :] < torch.from_numpy(lens).to(device)[:, None]
    off = np.zeros(len(lens) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    types = None
    if token_type_ids is not None:
        types = token_type_ids.to(device)
        if types.shape != keep.shape:
            raise ValueError("token_type_ids must have the shape of input_ids")
        types = types[keep].to(torch.int32).contiguous()
    return ids[keep].to(torch.int32).contiguous(), off, types


def _word_rows(off: np.ndarray) -> int:
    """Masked rows of ``rs_pll_score`` / ``rs_pll_topk``: one per word position ([CLS] w.. [SEP])."""
    return int((np.diff(off) - 2).sum()) if len(off) > 1 else 0


class PLLScorer(BertEngine):
    """MLM_PLL scorer (BertForMaskedLM head)."""

    def __init__(self, weights, shape: BertShape = BERT_BASE, device=0, max_rows: int = 65536,
                 precision: str = "fp16x3"):
        # fp16x3 (default): fp32-accurate split-fp16 operands, like the reference's fp32
        # BertForMaskedLM; "fp16" is an opt-in reduced-precision fast mode
        super().__init__(weights, shape, _lib.RS_HEAD_MLM, device, max_rows, precision)

    def score_nbest(self, tokens, hyp_off, return_rows: bool = False, variant: str = "original", word_start=None,
                    token_types=None, score_from=None, stride: int = 0):
        """tokens int32 [sum T] ([CLS] w.. [SEP] per hypothesis), hyp_off int [H+1].

        ``variant``: "original" (``rs_pll_score``), or "word_l2r" / "whole_word" (``data.pll_spans``
        over ``word_start``, uint8 per token, through ``score_spans``), or "strided" (``data.pll_strided``
        with ``stride`` >= 1 through ``score_sets``: every ``stride``-th token masked in one copy and all
        of them scored from it, ``min(stride, L)`` forwards per hypothesis; an approximation of PLL
        whose rows come back in ``pll_strided``'s order).

        ``token_types``: one segment id per token (``data.with_context``: 0 over ``[CLS] context
        [SEP]``, 1 over the hypothesis).  ``score_from`` int [H]: hypothesis h is scored only at
        positions ``p >= score_from[h]`` (the hypothesis half of a pair); every variant then goes
        through ``score_spans``.

        Returns float64 [H] device tensor of PLL (and float32 per-row log-probs)."""
        if variant == "strided":
            return self.score_sets(tokens, hyp_off, *pll_strided(hyp_off, stride, score_from=score_from),
                                   return_rows=return_rows, token_types=token_types)
        if variant not in PLL_VARIANTS:
            raise ValueError(f"unknown PLL variant {variant!r} {PLL_VARIANTS + ('strided',)}")
        if variant != "original" or score_from is not None:
            if variant != "original" and word_start is None:
                raise ValueError(f"variant {variant!r} needs word_start")
            return self.score_spans(tokens, hyp_off, *pll_spans(hyp_off, word_start, variant, score_from=score_from),
                                    return_rows=return_rows, token_types=token_types)
        d_tok, off, n_hyp = self._hyps(tokens, hyp_off)
        pll = torch.empty(n_hyp, dtype=torch.float64, device=self.device)
        rows = torch.empty(_word_rows(off), dtype=torch.float32, device=self.device) if return_rows else None
        d_type = self._set_types(token_types)      # noqa: F841  (alive until the call has returned)
        _lib.check(self.lib.rs_pll_score(self.handle, _lib.ptr(d_tok), off.ctypes.data, n_hyp,
                                         _lib.ptr(pll), _lib.ptr(rows), _lib.stream_ptr(self.device)))
        return (pll, rows) if return_rows else pll

    def score_spans(self, tokens, hyp_off, row_off, lo, hi, query, return_rows: bool = False, token_types=None):
        """Span-masked PLL (``rs_pll_score_spans``): row r of hypothesis h (``row_off[h] <= r <
        row_off[h + 1]``) is the hypothesis with positions ``[lo[r], hi[r])`` replaced by [MASK],
        scored at ``query[r]`` (positions relative to the hypothesis, ``1 <= lo <= query < hi <=
        T - 1``).  Rows may come in any order, repeat and skip positions.  ``token_types``: one
        segment id per token (``score_nbest``).

        Returns float64 [H] device tensor (sum of each hypothesis' rows in row order; no rows: 0)
        and, with ``return_rows``, the float32 per-row log-probs."""
        d_tok, off, n_hyp = self._hyps(tokens, hyp_off)
        roff = np.ascontiguousarray(row_off, np.int32)
        if len(roff) != n_hyp + 1:
            raise ValueError("row_off must have one entry per hypothesis plus one")
        n_rows = max(int(roff[-1]), 0) if n_hyp else 0
        cols = [None if c is None else np.ascontiguousarray(c, np.int32) for c in (lo, hi, query)]
        if any(c is not None and len(c) != n_rows for c in cols):
            raise ValueError("lo, hi and query must have row_off[-1] entries")
        pll = torch.empty(n_hyp, dtype=torch.float64, device=self.device)
        rows = torch.empty(n_rows, dtype=torch.float32, device=self.device) if return_rows else None
        d_type = self._set_types(token_types)      # noqa: F841
        _lib.check(self.lib.rs_pll_score_spans(self.handle, _lib.ptr(d_tok), off.ctypes.data, n_hyp, roff.ctypes.data,
                                               *[_lib.ptr(c) for c in cols], _lib.ptr(pll), _lib.ptr(rows),
                                               _lib.stream_ptr(self.device)))
        return (pll, rows) if return_rows else pll

    def score_sets(self, tokens, hyp_off, row_off, pos_off, pos, return_rows: bool = False, token_types=None):
        """Multi-mask PLL rows (``rs_pll_score_sets``): row r of hypothesis h (``row_off[h] <= r <
        row_off[h + 1]``) is the hypothesis with every position of ``pos[pos_off[r]:pos_off[r + 1]]``
        replaced by [MASK], and every one of them is scored from that one forward (positions relative
        to the hypothesis, strictly ascending within a row, ``1 <= p <= T - 2``, at least one per row).

        Returns float64 [H] device tensor (sum of each hypothesis' entries in list order; no rows: 0)
        and, with ``return_rows``, the float32 log-prob of every entry of ``pos``."""
        d_tok, off, n_hyp = self._hyps(tokens, hyp_off)
        roff = np.ascontiguousarray(row_off, np.int32)
        if len(roff) != n_hyp + 1:
            raise ValueError("row_off must have one entry per hypothesis plus one")
        n_rows = max(int(roff[-1]), 0) if n_hyp else 0
        poff = np.ascontiguousarray(pos_off, np.int32)
        ps = np.ascontiguousarray(pos, np.int32)
        if len(poff) != n_rows + 1:
            raise ValueError("pos_off must have row_off[-1] + 1 entries")
        n_pos = max(int(poff[-1]), 0)
        if len(ps) != n_pos:
            raise ValueError("pos must have pos_off[-1] entries")
        pll = torch.empty(n_hyp, dtype=torch.float64, device=self.device)
        rows = torch.empty(n_pos, dtype=torch.float32, device=self.device) if return_rows else None
        d_type = self._set_types(token_types)      # noqa: F841
        _lib.check(self.lib.rs_pll_score_sets(self.handle, _lib.ptr(d_tok), off.ctypes.data, n_hyp, roff.ctypes.data,
                                              poff.ctypes.data, ps.ctypes.data, _lib.ptr(pll), _lib.ptr(rows),
                                              _lib.stream_ptr(self.device)))
        return (pll, rows) if return_rows else pll

    def score(self, nb: NBest) -> np.ndarray:
        return self.score_nbest(nb.tokens, nb.hyp_off, token_types=nb.token_type,
                                score_from=nb.score_from).cpu().numpy()

    def masked_logprob_multi(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, labels: torch.Tensor,
                             token_type_ids=None) -> torch.Tensor:
        """``BertForMaskedLM(input_ids, labels)`` per-position log-probs for a padded batch [B, T] whose
        rows are already masked: every position with ``labels != -100`` (any number >= 1 per row, inside
        the row's attended prefix) is scored against its label from the row's one forward
        (``rs_masked_logprob_multi``).  Returns float32 [B, T] on the device,
        ``log_softmax(logits[b, t])[labels[b, t]]`` at the scored positions and ``nan`` elsewhere
        (their mean, negated, is the model's loss)."""
        d_ids, off, types = _ragged(input_ids, attention_mask, token_type_ids, self.device)
        B, T = input_ids.shape
        lab = labels.to(self.device)
        if lab.shape != input_ids.shape:
            raise ValueError("labels must have the shape of input_ids")
        lens = torch.from_numpy(np.diff(off).astype(np.int64)).to(self.device)
        scored = lab != -100
        if bool((scored & (torch.arange(T, device=self.device)[None, :] >= lens[:, None])).any()):
            raise ValueError("a label outside its row's attended prefix")
        b_idx, t_idx = torch.nonzero(scored, as_tuple=True)          # row-major: ascending within a row
        q_off = np.zeros(B + 1, np.int32)
        q_off[1:] = np.cumsum(scored.sum(1).cpu().numpy())
        qpos = t_idx.to(torch.int32).cpu().numpy()
        d_lab = lab[b_idx, t_idx].to(torch.int32).contiguous()
        out = torch.empty(len(qpos), dtype=torch.float32, device=self.device)
        d_type = self._set_types(types)      # noqa: F841
        _lib.check(self.lib.rs_masked_logprob_multi(self.handle, _lib.ptr(d_ids), off.ctypes.data, B, q_off.ctypes.data,
                                                    _lib.ptr(qpos), _lib.ptr(d_lab), _lib.ptr(out),
                                                    _lib.stream_ptr(self.device)))
        full = torch.full((B, T), float("nan"), dtype=torch.float32, device=self.device)
        full[b_idx, t_idx] = out
        return full

    def score_cands(self, ids, seq_off, q_off, qpos, c_off, cand, token_types=None) -> torch.Tensor:
        """Candidate log-probs on ragged rows (``rs_masked_logprob_cands``): row s is tokens
        ``ids[seq_off[s]:seq_off[s + 1]]`` (already masked), scored at positions
        ``qpos[q_off[s]:q_off[s + 1]]`` (strictly ascending, at least one per row); query q's candidates
        are the vocabulary ids ``cand[c_off[q]:c_off[q + 1]]`` (any order, duplicates allowed, the list
        may be empty).  Returns float32 [n_c] on the device, ``log_softmax(logits[qpos_q])[cand[c]]`` in
        the order of ``cand``: bitwise what ``rs_masked_logprob_multi`` gives with that id as the label."""
        d_ids, off, n_seq = self._hyps(ids, seq_off)
        qo, qp, co, cd = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in (q_off, qpos, c_off, cand))
        if len(qo) != n_seq + 1:
            raise ValueError("q_off must have one entry per row plus one")
        n_q = max(int(qo[-1]), 0) if n_seq else 0
        if len(qp) != n_q or len(co) != n_q + 1:
            raise ValueError("qpos must have q_off[-1] entries and c_off one more")
        n_c = max(int(co[-1]), 0)
        if len(cd) != n_c:
            raise ValueError("cand must have c_off[-1] entries")
        out = torch.empty(n_c, dtype=torch.float32, device=self.device)
        d_type = self._set_types(token_types)      # noqa: F841
        _lib.check(self.lib.rs_masked_logprob_cands(self.handle, _lib.ptr(d_ids), off.ctypes.data, n_seq, qo.ctypes.data,
                                                    qp.ctypes.data, co.ctypes.data, cd.ctypes.data, _lib.ptr(out),
                                                    _lib.stream_ptr(self.device)))
        return out

    def masked_logprob_cands(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, mask_pos, candidates,
                             token_type_ids=None):
        """``log_softmax(logits[b, mask_pos[b]])[candidates[b]]`` for a padded batch [B, T] (the form
        ``masked_logprob`` takes), ``candidates`` a list of id lists, one per row.  Returns a list of
        float32 device tensors, one per row, in the order of that row's list."""
        d_ids, off, types = _ragged(input_ids, attention_mask, token_type_ids, self.device)
        B = input_ids.shape[0]
        if len(candidates) != B:
            raise ValueError("candidates must hold one list per row")
        mp = np.asarray([int(x) for x in mask_pos], np.int32)
        c_off = np.zeros(B + 1, np.int32)
        c_off[1:] = np.cumsum([len(c) for c in candidates])
        cand = np.asarray([int(x) for c in candidates for x in c], np.int32)
        out = self.score_cands(d_ids, off, np.arange(B + 1, dtype=np.int32), mp, c_off, cand, token_types=types)
        return [out[c_off[b]:c_off[b + 1]] for b in range(B)]

    def masked_logprob(self, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                       labels: torch.Tensor, mask_pos, token_type_ids=None) -> torch.Tensor:
        """``token_score`` of MLM_PLL/main.py:101-105 for a padded batch [B, T].

        ``attention_mask`` rows must be a prefix of ones (``pad_sequence`` output);
        ``token_type_ids``: padded [B, T] segment ids as transformers takes them."""
        d_ids, off, types = _ragged(input_ids, attention_mask, token_type_ids, self.device)
        B = input_ids.shape[0]
        mp = np.asarray([int(x) for x in mask_pos], np.int32)
        lab = labels.to(self.device)[torch.arange(B, device=self.device),
                                     torch.from_numpy(mp.astype(np.int64)).to(self.device)]
        return self._masked_logprob(d_ids, off, mp, lab.to(torch.int32).contiguous(), types)

    def _masked_logprob(self, d_ids, off, mp, lab, token_types=None) -> torch.Tensor:
        """``rs_masked_logprob`` on ragged rows (device ids and labels, int32 offsets and query
        positions): float32 [R] device tensor."""
        out = torch.empty(len(off) - 1, dtype=torch.float32, device=self.device)
        d_type = self._set_types(token_types)      # noqa: F841
        _lib.check(self.lib.rs_masked_logprob(self.handle, _lib.ptr(d_ids), off.ctypes.data, mp.ctypes.data,
                                              _lib.ptr(lab), len(off) - 1, _lib.ptr(out),
                                              _lib.stream_ptr(self.device)))
        return out

    def masked_topk(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, mask_pos, k: int = 5,
                    token_type_ids=None):
        """The model's ``k`` preferred tokens at ``mask_pos`` of every row of a padded batch [B, T]
        (the form ``masked_logprob`` takes): ``torch.topk(log_softmax(logits[range(B), mask_pos]), k)``
        of MLM_PLL/main.py:101-105 without the [B, vocab] rows.  Returns device tensors
        (ids int32 [B, k], logprob float32 [B, k]), best first, equal logits by the lower id.
        ``token_type_ids``: padded [B, T] segment ids."""
        d_ids, off, types = _ragged(input_ids, attention_mask, token_type_ids, self.device)
        B = input_ids.shape[0]
        mp = np.asarray([int(x) for x in mask_pos], np.int32)
        top_id = torch.empty((B, max(int(k), 0)), dtype=torch.int32, device=self.device)
        top_lp = torch.empty((B, max(int(k), 0)), dtype=torch.float32, device=self.device)
        d_type = self._set_types(types)      # noqa: F841
        _lib.check(self.lib.rs_masked_topk(self.handle, _lib.ptr(d_ids), off.ctypes.data, mp.ctypes.data, B, int(k),
                                           _lib.ptr(top_id), _lib.ptr(top_lp), _lib.stream_ptr(self.device)))
        return top_id, top_lp

    def topk_nbest(self, tokens, hyp_off, k: int = 5, return_pll: bool = False, token_types=None):
        """``score_nbest`` plus the ``k`` preferred tokens of every masked row (rows ordered as
        ``score_nbest(..., return_rows=True)``'s: hypothesis by hypothesis, position by position).

        Returns (ids int32 [R, k], logprob float32 [R, k]) device tensors, followed by
        (pll float64 [H], rows float32 [R]) — bitwise ``score_nbest``'s — when ``return_pll``."""
        d_tok, off, n_hyp = self._hyps(tokens, hyp_off)
        n_rows = _word_rows(off)
        pll = torch.empty(n_hyp, dtype=torch.float64, device=self.device) if return_pll else None
        rows = torch.empty(n_rows, dtype=torch.float32, device=self.device) if return_pll else None
        top_id = torch.empty((n_rows, max(int(k), 0)), dtype=torch.int32, device=self.device)
        top_lp = torch.empty((n_rows, max(int(k), 0)), dtype=torch.float32, device=self.device)
        d_type = self._set_types(token_types)      # noqa: F841
        _lib.check(self.lib.rs_pll_topk(self.handle, _lib.ptr(d_tok), off.ctypes.data, n_hyp, int(k), _lib.ptr(pll),
                                        _lib.ptr(rows), _lib.ptr(top_id), _lib.ptr(top_lp),
                                        _lib.stream_ptr(self.device)))
        return (top_id, top_lp, pll, rows) if return_pll else (top_id, top_lp)

    def row_logprobs(self, rows) -> torch.Tensor:
        """``token_score`` (MLM_PLL/main.py:101-105) of every do_job row, float32 [R] (device),
        all rows in one ragged launch sequence."""
        seqs = [r["input_ids"] for r in rows]
        off = np.zeros(len(rows) + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in seqs])
        d_ids = torch.from_numpy(np.concatenate([np.asarray(s, np.int32) for s in seqs])).to(self.device)
        mp = np.asarray([r["mask_pos"] for r in rows], np.int32)
        lab = torch.from_numpy(np.asarray([r["labels"][r["mask_pos"]] for r in rows], np.int32)).to(self.device)
        return self._masked_logprob(d_ids, off, mp, lab)

    def run_one_epoch(self, rows, output_score: dict) -> dict:
        """Mirror of ``run_one_epoch(..., train_mode=False, do_scoring=True)``
        (MLM_PLL/main.py:73-114) over ``do_job`` rows (dicts with utt_id, hyp_id,
        input_ids, labels, mask_pos): scores all rows in one ragged launch sequence and
        adds them to ``output_score[utt][hyp]`` in row order (float64, like ``+=``)."""
        if not rows:
            return output_score
        for r, s in zip(rows, self.row_logprobs(rows).cpu().tolist()):
            output_score[r["utt_id"]][r["hyp_id"]] += s
        return output_score


class RescoreBertScorer(BertEngine):
    """RescoreBert scorer on ragged hypotheses (CLS head)."""

    def __init__(self, weights, shape: BertShape = BERT_BASE, device=0, max_rows: int = 65536,
                 precision: str = "fp16x3"):
        super().__init__(weights, shape, _lib.RS_HEAD_CLS, device, max_rows, precision)

    def score_nbest(self, tokens, hyp_off, token_types=None) -> torch.Tensor:
        d_tok, off, n = self._hyps(tokens, hyp_off)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        d_type = self._set_types(token_types)      # noqa: F841
        _lib.check(self.lib.rs_cls_score(self.handle, _lib.ptr(d_tok), off.ctypes.data, n,
                                         _lib.ptr(out), _lib.stream_ptr(self.device)))
        return out

    def score(self, nb: NBest) -> np.ndarray:
        return self.score_nbest(nb.tokens, nb.hyp_off, token_types=nb.token_type).cpu().numpy()


class RescoreBertHIP(torch.nn.Module):
    """Same construction/forward contract as ``RescoreBert`` (RescoreBert/model.py:4-21).

    ``weights`` is the HF-keyed state dict (``bert.*`` + ``linear.weight/bias``) instead of
    a model name, since nothing can be fetched offline."""

    def __init__(self, weights: Dict[str, np.ndarray], shape: BertShape = BERT_BASE, device=0,
                 max_rows: int = 65536, precision: str = "fp16x3"):
        super().__init__()
        self.engine = RescoreBertScorer(weights, shape, device, max_rows, precision)

    def forward(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, token_type_ids=None) -> torch.Tensor:
        d_ids, off, types = _ragged(input_ids, attention_mask, token_type_ids, self.engine.device)
        if (np.diff(off) == 0).any():
            raise ValueError("every row needs at least one attended token")
        return self.engine.score_nbest(d_ids, off, token_types=types)


def pll_of(weights, nb: NBest, shape: BertShape = BERT_BASE, device=0) -> np.ndarray:
    """Convenience: PLL float64 [H] of an ``NBest`` (one scorer, one call)."""
    sc = PLLScorer(weights, shape, device)
    try:
        return sc.score(nb)
    finally:
        sc.close()

