"""AM/LM fusion, argmax, corpus CER and RMBR (CER utility) on the GPU.

Host mirrors of the reference functions (same names, argument meaning, tie rules):

* ``find_best_weight`` — rescore.py:25-45 (101-weight grid, strict ``<`` keeps the first
  best weight); the whole grid is one ``rs_fuse_rerank`` launch and the corpus CER of every
  weight is one ``rs_corpus_edits`` launch over a per-hypothesis ``ed(ref, hyp)`` table
  (``rs_ref_edit``), exactly Σ edits / Σ ref chars as ``jiwer.cer`` computes it.
* ``fuse_rerank`` — ``rescore`` + ``get_highest_score_hyp`` (rescore.py:47-58).
* ``mbr_decode`` / ``find_best_length`` — RMBR/mbr.py:5-28, RMBR/main.py:15-35 with
  ``CerScoreFunction``; the pairwise edit matrix is computed once and reused for every k.
* ``consensus_decode`` / ``find_best_weight_consensus`` — no reference counterpart: the per-slot vote
  over the N-best confusion network (``cnet``), every hypothesis weighted by the softmax of the fused
  score, scored by the same CER kernels; a third decoding rule beside argmax and MBR.
* ``consensus_decode_lm`` / ``find_best_weight_consensus_lm`` — no reference counterpart: that vote with
  the masked LM's log-probs of each contested slot's competing tokens mixed in (``cnet.slot_lm_vote``).

Inputs are ``NBest`` (token/char ids); "characters" are symbols, as jiwer's CER splits text
into characters (CJK: one token per character).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .data import NBest

# Edit-distance kernels (csrc/k_rerank.hip): exact for strings of up to RS_MAX_EDIT symbols
MAX_EDIT_LEN = 16384


def _dev(a, dtype, device):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(device)


def weight_grid(mode: str = "norm") -> np.ndarray:
    """rescore.py:37 (np.arange(0.0, 1.01, 0.01)); the legacy log used arange(0, 1.0, 0.01)."""
    return np.arange(0.0, 1.0, 0.01) if mode == "legacy" else np.arange(0.0, 1.01, 0.01)


def _strings(nb: NBest):
    """Hypothesis words only ([CLS]/[SEP] stripped), flat int32 + offsets (vectorised)."""
    off = np.asarray(nb.hyp_off, np.int64)
    keep = np.ones(len(nb.tokens), bool)
    if nb.n_hyp:
        keep[off[:-1]] = False           # [CLS]
        keep[off[1:] - 1] = False        # [SEP]
    flat = np.ascontiguousarray(nb.tokens[keep], np.int32)
    soff = np.zeros(nb.n_hyp + 1, np.int32)
    soff[1:] = np.cumsum(np.diff(off) - 2)
    return flat, soff


def ref_edits(nb: NBest, device=0) -> torch.Tensor:
    """int32 [H] = Levenshtein(ref_u, hyp_h) for every hypothesis (device)."""
    lib = _lib.load()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    flat, soff = _strings(nb)
    if any(len(r) == 0 for r in nb.refs):
        raise ValueError("one or more references are empty strings")   # jiwer behaviour
    rflat = np.concatenate(nb.refs).astype(np.int32)
    roff = np.zeros(nb.n_utt + 1, np.int32)
    roff[1:] = np.cumsum([len(r) for r in nb.refs])
    if max(int(np.diff(soff).max(initial=0)), int(np.diff(roff).max(initial=0))) > MAX_EDIT_LEN:
        raise ValueError(f"strings longer than {MAX_EDIT_LEN} symbols are not supported")
    d_c, d_so, d_uo = _dev(flat, torch.int32, dev), _dev(soff, torch.int32, dev), _dev(nb.utt_off, torch.int32, dev)
    d_rc, d_ro = _dev(rflat, torch.int32, dev), _dev(roff, torch.int32, dev)
    out = torch.empty(nb.n_hyp, dtype=torch.int32, device=dev)
    _lib.check(lib.rs_ref_edit(_lib.ptr(d_c), _lib.ptr(d_so), _lib.ptr(d_uo), _lib.ptr(d_rc), _lib.ptr(d_ro),
                               nb.n_utt, _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


def fuse_rerank(am, lm, hyp_len, utt_off, weights, mode: str = "norm", n_best: int = 1 << 30,
                device=0) -> torch.Tensor:
    """argmax int32 [W, U] of the fused scores for every weight (device)."""
    lib = _lib.load()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    am_d = am if isinstance(am, torch.Tensor) else _dev(am, torch.float64, dev)
    lm_d = lm if isinstance(lm, torch.Tensor) else _dev(lm, torch.float64, dev)
    am_d, lm_d = am_d.to(dev, torch.float64).contiguous(), lm_d.to(dev, torch.float64).contiguous()
    ln = _dev(hyp_len, torch.int32, dev)
    uo = _dev(utt_off, torch.int32, dev)
    w = _dev(np.asarray(weights, np.float64), torch.float64, dev)
    n_utt = len(utt_off) - 1
    out = torch.empty(len(weights), n_utt, dtype=torch.int32, device=dev)
    _lib.check(lib.rs_fuse_rerank(_lib.ptr(am_d), _lib.ptr(lm_d), _lib.ptr(ln), _lib.ptr(uo), n_utt,
                                  min(int(n_best), 2**31 - 1), _lib.ptr(w), len(weights), _lib.RS_FUSE[mode],
                                  _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


def corpus_edits(ed_ref: torch.Tensor, utt_off, argmax: torch.Tensor, device=0) -> torch.Tensor:
    lib = _lib.load()
    dev = argmax.device
    uo = _dev(utt_off, torch.int32, dev)
    W, U = argmax.shape
    out = torch.empty(W, dtype=torch.int64, device=dev)
    _lib.check(lib.rs_corpus_edits(_lib.ptr(ed_ref), _lib.ptr(uo), _lib.ptr(argmax.contiguous()), U, W,
                                   _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


def find_best_weight(nb: NBest, lm, n_best: int = 10, mode: str = "norm", device=0
                     ) -> Tuple[float, float, np.ndarray, np.ndarray]:
    """rescore.py:25-45: returns (best_weight, best_cer, argmax [W, U], cer [W])."""
    grid = weight_grid(mode)
    lens = nb.hyp_len()
    arg = fuse_rerank(nb.am, lm, lens, nb.utt_off, grid, mode, n_best, device)
    ed = ref_edits(nb, device)
    edits = corpus_edits(ed, nb.utt_off, arg, device).cpu().numpy()
    total = sum(len(r) for r in nb.refs)
    cers = edits / total
    best_i, best = 0, float("inf")
    for i, c in enumerate(cers):            # strict '<' keeps the first best (rescore.py:41)
        if c < best:
            best, best_i = c, i
    return float(grid[best_i]), float(best), arg.cpu().numpy(), cers


def pairwise_edit(nb: NBest, device=0) -> Tuple[torch.Tensor, np.ndarray]:
    """Concatenated n_u x n_u int32 matrices and their int64 offsets."""
    lib = _lib.load()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    flat, soff = _strings(nb)
    n_u = np.diff(nb.utt_off).astype(np.int64)
    moff = np.zeros(nb.n_utt + 1, np.int64)
    moff[1:] = np.cumsum(n_u * n_u)
    if len(soff) > 1 and int(np.diff(soff).max()) > MAX_EDIT_LEN:
        raise ValueError(f"strings longer than {MAX_EDIT_LEN} symbols are not supported")
    d_c, d_so = _dev(flat, torch.int32, dev), _dev(soff, torch.int32, dev)
    d_uo, d_mo = _dev(nb.utt_off, torch.int32, dev), _dev(moff, torch.int64, dev)
    ed = torch.empty(int(moff[-1]), dtype=torch.int32, device=dev)
    _lib.check(lib.rs_pairwise_edit(_lib.ptr(d_c), _lib.ptr(d_so), _lib.ptr(d_uo), _lib.ptr(d_mo), nb.n_utt,
                                    int(n_u.max(initial=0)), _lib.ptr(ed), _lib.stream_ptr(dev)))
    return ed, moff


def mbr_scores(nb: NBest, k: int, ed: torch.Tensor, moff: np.ndarray, device=0
               ) -> Tuple[np.ndarray, np.ndarray]:
    """RMBR/mbr.py:5-28 for top-k: (argmax int [U], scores float32 [U, k])."""
    lib = _lib.load()
    dev = ed.device
    if int(np.diff(nb.utt_off).min(initial=k)) < k:
        raise ValueError("every utterance needs at least k hypotheses")
    lens = nb.hyp_len()
    if (lens == 0).any():
        raise ValueError("one or more references are empty strings")   # jiwer on an empty hyp_j
    d_mo, d_uo = _dev(moff, torch.int64, dev), _dev(nb.utt_off, torch.int32, dev)
    d_len = _dev(lens, torch.int32, dev)
    sc = torch.empty(nb.n_utt, k, dtype=torch.float32, device=dev)
    am = torch.empty(nb.n_utt, dtype=torch.int32, device=dev)
    _lib.check(lib.rs_mbr_scores(_lib.ptr(ed), _lib.ptr(d_mo), _lib.ptr(d_uo), _lib.ptr(d_len), nb.n_utt, k,
                                 _lib.ptr(sc), _lib.ptr(am), _lib.stream_ptr(dev)))
    return am.cpu().numpy(), sc.cpu().numpy()


def mbr_decode(nb: NBest, k: int, device=0) -> Tuple[np.ndarray, np.ndarray]:
    ed, moff = pairwise_edit(nb, device)
    return mbr_scores(nb, k, ed, moff, device)


def find_best_length(nb: NBest, n_best: int, device=0) -> Tuple[float, int, np.ndarray]:
    """RMBR/main.py:15-35: (best_cer, best_length, best scores [U, k])."""
    ed, moff = pairwise_edit(nb, device)
    ed_ref = ref_edits(nb, device)
    total = sum(len(r) for r in nb.refs)
    best_cer, best_len, best_sc = float("inf"), 2, None
    for k in range(2, n_best + 1):
        am, sc = mbr_scores(nb, k, ed, moff, device)
        arg = torch.from_numpy(am.astype(np.int32)).to(ed.device)[None, :]
        err = float(corpus_edits(ed_ref, nb.utt_off, arg).cpu()[0]) / total
        if err < best_cer:
            best_cer, best_len, best_sc = err, k, sc
    return best_cer, best_len, best_sc


class _Consensus:
    """A slot table of the first ``n_best`` hypotheses per utterance plus what scoring its decodes needs."""

    def __init__(self, nb: NBest, n_best: int, mode: str, device):
        from . import cnet
        if any(len(r) == 0 for r in nb.refs):
            raise ValueError("one or more references are empty strings")   # jiwer behaviour
        self.nb, self.cnet = nb, cnet
        keep = [np.arange(a, min(b, a + n_best)) for a, b in zip(nb.utt_off[:-1], nb.utt_off[1:])]
        self.idx = np.concatenate(keep) if keep else np.zeros(0, np.int64)
        self.table = cnet.merge_nbest([[nb.hyp_words(int(h)).tolist() for h in hs] for hs in keep], mode, device)
        dev = self.dev = self.table.device
        self.inv = _dev(np.asarray(list(self.table._vocab) + [0], np.int32), torch.int32, dev)
        roff = np.zeros(nb.n_utt + 1, np.int32)
        roff[1:] = np.cumsum([len(r) for r in nb.refs])
        self.d_rc, self.d_ro = _dev(np.concatenate(nb.refs), torch.int32, dev), _dev(roff, torch.int32, dev)
        self.total = int(roff[-1])
        self.one_off = np.arange(nb.n_utt + 1, dtype=np.int32)          # one decode per utterance
        self.d_one = _dev(self.one_off, torch.int32, dev)
        so = torch.from_numpy(self.table.slot_off.astype(np.int64)).to(dev)
        n_slot = int(self.table.slot_off[-1])
        utt = torch.repeat_interleave(torch.arange(nb.n_utt, device=dev), so[1:] - so[:-1])
        self.slot_pos, self.slot_utt = torch.arange(n_slot, device=dev) - so[utt], utt

    def weights(self, lm, weight: float, scale: float) -> np.ndarray:
        nb, t = self.nb, self.table
        lm = lm.cpu().numpy() if isinstance(lm, torch.Tensor) else np.asarray(lm)
        return self.cnet.consensus_weights(np.asarray(nb.am)[self.idx], lm[self.idx], nb.hyp_len()[self.idx],
                                           t.utt_off, weight, scale)

    def decode(self, w: np.ndarray):
        """(corpus edits, decoded id lists) of the vote under weights ``w``."""
        lib, nb, dev = _lib.load(), self.nb, self.dev
        _, _, _, dec, dlen = self.table.vote_device(torch.from_numpy(np.ascontiguousarray(w, np.float64)))
        dlen = dlen[:nb.n_utt].to(torch.int64)
        n_slot = self.slot_pos.numel()
        flat = self.inv[dec[:n_slot][self.slot_pos < dlen[self.slot_utt]].to(torch.int64)]
        soff = torch.zeros(nb.n_utt + 1, dtype=torch.int32, device=dev)
        soff[1:] = torch.cumsum(dlen, 0)
        chars = torch.cat([flat, torch.zeros(1, dtype=torch.int32, device=dev)]).contiguous()
        ed = torch.empty(max(nb.n_utt, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.rs_ref_edit(_lib.ptr(chars), _lib.ptr(soff), _lib.ptr(self.d_one), _lib.ptr(self.d_rc),
                                   _lib.ptr(self.d_ro), nb.n_utt, _lib.ptr(ed), _lib.stream_ptr(dev)))
        first = torch.zeros(1, nb.n_utt, dtype=torch.int32, device=dev)
        edits = int(corpus_edits(ed, self.one_off, first).cpu()[0])
        so, fl = soff.cpu().numpy(), flat.cpu().numpy()
        return edits, [fl[a:b] for a, b in zip(so[:-1], so[1:])]


def consensus_decode(nb: NBest, lm, weight: float, scale: float = 1.0, n_best: int = 1 << 30, mode: str = "exact",
                     device=0) -> Tuple[float, List[np.ndarray]]:
    """Confusion-network consensus decode: every hypothesis votes per slot with its softmax-normalised
    fused score (cnet.consensus_weights); returns (corpus CER, decoded ids per utterance), the CER as
    ``find_best_weight`` forms it (rs_ref_edit, rs_corpus_edits; sum of edits / sum of reference symbols)."""
    c = _Consensus(nb, n_best, mode, device)
    edits, dec = c.decode(c.weights(lm, weight, scale))
    return edits / c.total, dec


def find_best_weight_consensus(nb: NBest, lm, n_best: int = 10, scale: float = 1.0, mode: str = "exact", device=0
                               ) -> Tuple[float, float, np.ndarray]:
    """The 101-weight grid of ``find_best_weight`` for the consensus decode: (best_weight, best_cer,
    cer [W]); strict ``<`` keeps the first best weight.  The table is merged once and voted per weight."""
    c = _Consensus(nb, n_best, mode, device)
    grid = weight_grid("norm")
    cers = np.asarray([c.decode(c.weights(lm, float(w), scale))[0] / c.total for w in grid])
    best_i, best = 0, float("inf")
    for i, v in enumerate(cers):
        if v < best:
            best, best_i = v, i
    return float(grid[best_i]), float(best), cers


LAM_GRID = (0.0, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0)


class _ConsensusLM(_Consensus):
    """``_Consensus`` (exact table) plus the masked-LM log-probs of every contested top-1 position's
    candidates: one row ``[CLS] top-1 [SEP]`` per position, that position replaced by [MASK] on the
    device, all rows in one ``score_cands`` call.  Computed once per table, reused for every ``lam``."""

    def __init__(self, nb: NBest, scorer, n_best: int, device):
        if nb.token_type is not None:
            raise ValueError("consensus_decode_lm takes plain hypothesis lists (no context pairs)")
        super().__init__(nb, n_best, "exact", device)
        self.scorer = scorer
        self._lp = self._pcs = None

    def rows(self):
        """(contested positions, device ids, seq_off, qpos): one row per ``position_candidates`` entry, the
        utterance's ``[CLS] top-1 [SEP]`` with position g + 1 replaced by [MASK] on the device."""
        nb, dev = self.nb, self.scorer.device
        if self._pcs is None:
            self._pcs = self.table.position_candidates()
        pcs = self._pcs
        ho = np.asarray(nb.hyp_off, np.int64)
        top = np.asarray(nb.utt_off, np.int64)[[u for u, *_ in pcs]]            # the top-1 hypothesis of each row
        a, T = ho[top], ho[top + 1] - ho[top]
        seq_off = np.zeros(len(pcs) + 1, np.int64)
        seq_off[1:] = np.cumsum(T)
        src = np.repeat(a - seq_off[:-1], T) + np.arange(seq_off[-1])           # row r, position t <- token a[r] + t
        qpos = np.asarray([g + 1 for _, _, g, _, _ in pcs], np.int64)           # past [CLS]
        d_rows = self.scorer._dev_tokens(nb.tokens)[torch.from_numpy(src).to(dev)]
        d_rows[torch.from_numpy(seq_off[:-1] + qpos).to(dev)] = self.scorer.shape.mask_id
        return pcs, d_rows, seq_off.astype(np.int32), qpos.astype(np.int32)

    def slot_lp(self):
        """({(utterance, slot): float32 log-probs in ``position_candidates`` order}, forwards)."""
        if self._lp is not None:
            return self._lp
        pcs, d_rows, seq_off, qpos = self.rows()
        if not pcs:
            self._lp = ({}, 0)
            return self._lp
        c_off = np.zeros(len(pcs) + 1, np.int32)
        c_off[1:] = np.cumsum([len(t) for _, _, _, t, _ in pcs])
        cand = np.asarray([t for _, _, _, toks, _ in pcs for t in toks], np.int32)
        lp = self.scorer.score_cands(d_rows, seq_off, np.arange(len(pcs) + 1, dtype=np.int32), qpos, c_off,
                                     cand).cpu().numpy()
        self._lp = ({(u, s): lp[c_off[i]:c_off[i + 1]] for i, (u, s, *_) in enumerate(pcs)}, len(pcs))
        return self._lp

    def edits_of(self, decoded) -> int:
        """Corpus edits of one decode per utterance (id lists), as ``decode`` scores the vote's."""
        lib, nb, dev = _lib.load(), self.nb, self.dev
        soff = np.zeros(nb.n_utt + 1, np.int32)
        soff[1:] = np.cumsum([len(d) for d in decoded])
        flat = np.asarray([t for d in decoded for t in d] + [0], np.int32)
        chars, d_so = _dev(flat, torch.int32, dev), _dev(soff, torch.int32, dev)
        ed = torch.empty(max(nb.n_utt, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.rs_ref_edit(_lib.ptr(chars), _lib.ptr(d_so), _lib.ptr(self.d_one), _lib.ptr(self.d_rc),
                                   _lib.ptr(self.d_ro), nb.n_utt, _lib.ptr(ed), _lib.stream_ptr(dev)))
        first = torch.zeros(1, nb.n_utt, dtype=torch.int32, device=dev)
        return int(corpus_edits(ed, self.one_off, first).cpu()[0])

    def decode_lm(self, w: np.ndarray, lam: float):
        """(corpus edits, decoded id lists) of ``cnet.slot_lm_vote`` under weights ``w``."""
        if lam == 0:
            return self.decode(w)
        dec, _, _ = self.cnet.slot_lm_vote(self.table, w, self.slot_lp()[0], lam)
        dec = [np.asarray(d, np.int32) for d in dec]
        return self.edits_of(dec), dec


def consensus_decode_lm(nb: NBest, lm, scorer, weight: float, lam: float, scale: float = 1.0, n_best: int = 1 << 30,
                        device=0, return_info: bool = False):
    """``consensus_decode`` (exact table) with the masked LM's opinion on every contested top-1 position:
    ``scorer`` (a ``PLLScorer`` whose vocabulary ids are ``nb``'s symbols) scores each such slot's
    competing tokens from one masked forward of the top-1 (``PLLScorer.score_cands``), and
    ``cnet.slot_lm_vote`` mixes them into the slot's vote with weight ``lam`` in [0, 1].  ``lam == 0`` is
    ``consensus_decode`` itself and runs no forward.  Returns (corpus CER, decoded ids per utterance) and,
    with ``return_info``, a dict: ``n_forwards``, ``n_contested`` and ``slot_lp`` (the log-probs used)."""
    c = _ConsensusLM(nb, scorer, n_best, device)
    edits, dec = c.decode_lm(c.weights(lm, weight, scale), float(lam))
    if not return_info:
        return edits / c.total, dec
    slot_lp, n_fwd = c.slot_lp() if lam != 0 else ({}, 0)
    return edits / c.total, dec, {"n_forwards": n_fwd, "n_contested": len(c.rows()[0]), "slot_lp": slot_lp}


def find_best_weight_consensus_lm(nb: NBest, lm, scorer, weight: float, lam_grid: Sequence[float] = LAM_GRID,
                                  scale: float = 1.0, n_best: int = 10, device=0) -> Tuple[float, float, np.ndarray]:
    """Sweeps ``lam`` over ``lam_grid`` at a fixed fusion ``weight``: (best_lam, best_cer, cer per lam);
    strict ``<`` keeps the first best.  The table is merged and the LM scores computed once."""
    c = _ConsensusLM(nb, scorer, n_best, device)
    w = c.weights(lm, weight, scale)
    cers = np.asarray([c.decode_lm(w, float(lam))[0] / c.total for lam in lam_grid])
    best_i, best = 0, float("inf")
    for i, v in enumerate(cers):
        if v < best:
            best, best_i = v, i
    return float(lam_grid[best_i]), float(best), cers


def argmax_words(nb: NBest, idx: Sequence[int]) -> List[np.ndarray]:
    return [nb.hyp_words(nb.utt_off[u] + int(i)) for u, i in enumerate(idx)]
