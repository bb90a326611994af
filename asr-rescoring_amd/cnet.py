"""N-best confusion network on the GPU: merge, oracle path, consensus vote
(Nbest_Align/preprocess.py:67-159 and CorrectBart/get_feature.py: hypotheses 2..N aligned to the top-1,
the alignments folded into one slot table, the table searched for the path closest to the transcript).

``merge_nbest`` aligns every (top-1, hypothesis n) pair of every utterance in one ``rs_align`` launch and
folds them with ``rs_cn_merge`` (csrc/k_cnet.hip) into a ``SlotTable``; ``SlotTable.oracle`` is the
reference's exhaustive search as a DP (``rs_cn_oracle``), ``SlotTable.vote`` a ROVER-style weighted vote
per slot (``rs_cn_vote``).  Two modes: ``"reference"`` is the reference's table bit for bit, including the
entries its fold copies into gap slots; ``"exact"`` (default) leaves those gaps, so every hypothesis token
appears exactly once.  Tokens may be any hashable values except the gap ``"*"``.  No CPU fallback.
"""
from __future__ import annotations

import math
from typing import Hashable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, align

GAP = align.GAP
MODES = {"reference": 0, "exact": 1}      # RS_CN_REFERENCE / RS_CN_EXACT
MAX_LEN, MAX_N = 4096, 1024


def _off(lens, dtype=np.int32):
    out = np.zeros(len(lens) + 1, dtype)
    out[1:] = np.cumsum(np.asarray(lens, np.int64))
    return out


class SlotTable:
    """The merged table of a batch of utterances.

    ``src`` int32: utterance u's table at ``cell_off[u]``, ``[slots][N]`` row-major, the index of a token
    inside hypothesis n or -1 for a gap; ``slot_off`` int32 [U + 1]; ``hyps`` the token lists it indexes.
    """

    def __init__(self, hyps, ids, vocab, mode, dev, d):
        self.hyps, self.mode, self.device = hyps, mode, dev
        self._ids, self._vocab, self._d = ids, vocab, d
        self.utt_off = d["utt_off_h"]
        self.slot_off = d["slot_off"].cpu().numpy()
        self.cell_off = d["cell_off"].cpu().numpy()
        self.src = d["src"].cpu().numpy()[:int(self.cell_off[-1])]
        self.n_utt = len(hyps)
        self.max_n = max((len(h) for h in hyps), default=0)

    def n_slots(self, u: int) -> int:
        return int(self.slot_off[u + 1] - self.slot_off[u])

    def src_of(self, u: int) -> np.ndarray:
        """int32 [slots, N] of utterance u."""
        return self.src[self.cell_off[u]:self.cell_off[u + 1]].reshape(self.n_slots(u), len(self.hyps[u]))

    def tokens(self) -> List[List[list]]:
        """Per utterance the reference's merged_alignment: a list of slots, each N tokens with "*" gaps."""
        return [[[h[n][i] if i >= 0 else GAP for n, i in enumerate(row)] for row in self.src_of(u)]
                for u, h in enumerate(self.hyps)]

    def _table_ptrs(self):
        d = self._d
        return [_lib.ptr(d[k]) for k in ("src", "slot_off", "cell_off", "utt_off", "tok", "hyp_off")]

    def _split(self, a: np.ndarray) -> List[np.ndarray]:
        return [a[self.slot_off[u]:self.slot_off[u + 1]] for u in range(self.n_utt)]

    def oracle(self, refs: Sequence[Sequence[Hashable]]):
        """(dist int32 [U], labels: per utterance int32 [slots]) against one transcript per utterance."""
        if len(refs) != self.n_utt:
            raise ValueError("one transcript per utterance")
        lib, dev = _lib.load(), self.device
        vocab = dict(self._vocab)          # transcript-only tokens get ids no hypothesis has
        rid = [[vocab.setdefault(t, len(vocab)) for t in r] for r in refs]
        rlen = np.asarray([len(r) for r in rid], np.int64)
        S = np.diff(self.slot_off).astype(np.int64)
        e_off = _off((S + 1) * (rlen + 1), np.int64)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
        d_ref = T(np.asarray([t for r in rid for t in r] + [0], np.int32))
        d_roff, d_eoff = T(_off(rlen)), T(e_off)
        d_E = torch.empty(max(int(e_off[-1]), 1), dtype=torch.int32, device=dev)
        d_dist = torch.empty(max(self.n_utt, 1), dtype=torch.int32, device=dev)
        d_lab = torch.full((max(int(self.slot_off[-1]), 1),), -1, dtype=torch.int32, device=dev)
        _lib.check(lib.rs_cn_oracle(*self._table_ptrs(), self.n_utt, self.max_n, _lib.ptr(d_ref), _lib.ptr(d_roff),
                                    int(rlen.max(initial=0)), _lib.ptr(d_eoff), _lib.ptr(d_E), _lib.ptr(d_dist),
                                    _lib.ptr(d_lab), _lib.stream_ptr(dev)))
        return d_dist.cpu().numpy()[:self.n_utt], self._split(d_lab.cpu().numpy())

    def vote_device(self, w: torch.Tensor):
        """Raw vote on a float64 device tensor of one weight per hypothesis: device tensors
        (win_tok, win_col, share, dec, dec_len); utterance u's decode is dec[slot_off[u] .. + dec_len[u])."""
        lib, dev = _lib.load(), self.device
        n = max(int(self.slot_off[-1]), 1)
        if w.dtype != torch.float64 or w.numel() != int(self.utt_off[-1]):
            raise ValueError("weights: one float64 per hypothesis")
        w = w.to(dev).contiguous()
        win = torch.full((n,), -1, dtype=torch.int32, device=dev)
        col = torch.full((n,), -1, dtype=torch.int32, device=dev)
        share = torch.zeros(n, dtype=torch.float64, device=dev)
        dec = torch.full((n,), -1, dtype=torch.int32, device=dev)
        dlen = torch.zeros(max(self.n_utt, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.rs_cn_vote(*self._table_ptrs(), self.n_utt, self.max_n, _lib.ptr(w), _lib.ptr(win),
                                  _lib.ptr(col), _lib.ptr(share), _lib.ptr(dec), _lib.ptr(dlen),
                                  _lib.stream_ptr(dev)))
        return win, col, share, dec, dlen

    def vote(self, weights: Optional[Sequence] = None):
        """(decoded, winner_col, share) per utterance: the winning tokens without gaps, and per slot the
        winner's first column and its share of the weight.  ``weights``: one per hypothesis (flat, or a
        list per utterance); None = uniform, plain majority voting."""
        n_hyp = int(self.utt_off[-1])
        if weights is None:
            w = np.ones(n_hyp, np.float64)
        else:
            w = np.asarray(weights, np.float64) if np.ndim(weights[0] if len(weights) else 0) == 0 \
                else np.concatenate([np.asarray(x, np.float64) for x in weights])
        win, col, share, _, _ = self.vote_device(torch.from_numpy(np.ascontiguousarray(w)))
        inv = list(self._vocab)
        decoded = [[inv[t] for t in ws if t >= 0] for ws in self._split(win.cpu().numpy())]
        return decoded, self._split(col.cpu().numpy()), self._split(share.cpu().numpy())

    def position_candidates(self, min_distinct: int = 2):
        """The contested top-1 positions of an ``exact`` table: every slot whose column 0 is a top-1 token
        (not a gap) and that holds at least ``min_distinct`` distinct non-gap entries.  Per such slot
        ``(utterance, slot, g, tokens, cols)``: g the token's position in the top-1, the distinct non-gap
        tokens in order of their first column, and those first columns.  A slot whose hypotheses agree
        needs no language-model forward."""
        if self.mode != "exact":
            raise ValueError("position_candidates needs the exact table (every token appears once)")
        out = []
        for u, h in enumerate(self.hyps):
            src = self.src_of(u)
            if src.size == 0:
                continue
            # the slots worth a Python loop: a top-1 token and at least min_distinct distinct ids
            width = max(max(len(t) for t in self._ids[u]), 1)
            idm = np.full((len(h), width), -1, np.int64)
            for n, t in enumerate(self._ids[u]):
                idm[n, :len(t)] = t
            tid = np.where(src >= 0, idm[np.arange(len(h))[None, :], np.maximum(src, 0)], -1)
            srt = np.sort(tid, axis=1)
            distinct = (srt[:, 0] >= 0).astype(np.int64) + ((srt[:, 1:] != srt[:, :-1]) & (srt[:, 1:] >= 0)).sum(1)
            for s in np.nonzero((src[:, 0] >= 0) & (distinct >= min_distinct))[0].tolist():
                row = src[s]
                toks, cols = [], []
                for n, i in enumerate(row):
                    if i >= 0 and h[n][i] not in toks:
                        toks.append(h[n][i])
                        cols.append(n)
                if len(toks) >= min_distinct:
                    out.append((u, s, int(row[0]), toks, cols))
        return out


def _flat_weights(table: SlotTable, weights) -> np.ndarray:
    n_hyp = int(table.utt_off[-1])
    if weights is None:
        return np.ones(n_hyp, np.float64)
    if np.ndim(weights[0] if len(weights) else 0) == 0:
        return np.asarray(weights, np.float64)
    return np.concatenate([np.asarray(x, np.float64) for x in weights])


def _lse(xs) -> float:
    mx = max(xs)
    return mx + math.log(sum(math.exp(x - mx) for x in xs))


def slot_lm_vote(table: SlotTable, weights, slot_lp, lam: float):
    """``SlotTable.vote`` with a masked-LM opinion on the slots of ``slot_lp``: ``{(utterance, slot): one
    log-prob per distinct non-gap token of the slot, in ``position_candidates`` order}``.  Host, float64.

    Per slot with scores, masses as ``rs_cn_vote`` forms them (float64 sum of ``w`` over a candidate's
    columns, ascending): T = its non-gap candidates with mass > 0, M their total,
    ``s_c = (1 - lam) ln m_c + lam (lp_c - logsumexp_T lp)`` (``lam == 1``: the second term alone) and
    ``m''_c = M exp(s_c - logsumexp_T s)``: the LM redistributes the tokens' mass inside the slot.  The gap
    keeps its mass and its verdict: it wins exactly when it wins the plain vote (the LM has no score
    for "no token here"); otherwise the winner is the largest ``m''_c``, equal ones by the lowest first
    column.  Slots without scores, and slots whose token mass is 0, keep the plain vote.  ``lam == 0``
    is ``table.vote(weights)`` itself.  Returns what ``vote`` returns."""
    if not 0.0 <= lam <= 1.0:
        raise ValueError("lam must be in [0, 1]")
    decoded, cols, shares = table.vote(weights)
    if lam == 0 or not slot_lp:
        return decoded, cols, shares
    w = _flat_weights(table, weights)
    cols = [c.copy() for c in cols]
    shares = [x.copy() for x in shares]
    changed = set()
    for (u, s), lps in slot_lp.items():
        h = table.hyps[u]
        row = table.src_of(u)[s]
        wu = w[table.utt_off[u]:table.utt_off[u + 1]]
        first, mass = {}, {}
        for n, i in enumerate(row):                     # ascending column order, like the kernel
            t = h[n][i] if i >= 0 else GAP
            if t not in first:
                first[t] = n
                mass[t] = 0.0
            mass[t] += float(wu[n])
        toks = [t for t in first if t != GAP]
        if len(lps) != len(toks):
            raise ValueError(f"slot ({u}, {s}): {len(lps)} log-probs for {len(toks)} distinct tokens")
        plain_win = None
        for t in first:
            if plain_win is None or mass[t] > mass[plain_win]:
                plain_win = t
        T = [(t, float(lp)) for t, lp in zip(toks, lps) if mass[t] > 0.0]
        if plain_win == GAP or not T:
            continue
        M = 0.0
        for t, _ in T:
            M += mass[t]
        L = _lse([lp for _, lp in T])
        sc = [lp - L if lam == 1 else (1.0 - lam) * math.log(mass[t]) + lam * (lp - L) for t, lp in T]
        Ls = _lse(sc)
        best = None
        for (t, _), x in zip(T, sc):
            m2 = M * math.exp(x - Ls)
            if best is None or m2 > best[0]:
                best = (m2, t)
        total = 0.0
        for x in wu:
            total += float(x)
        cols[u][s] = first[best[1]]
        shares[u][s] = best[0] / total
        changed.add(u)
    for u in changed:
        h = table.hyps[u]
        src = table.src_of(u)
        decoded[u] = [h[c][src[s][c]] for s, c in enumerate(cols[u]) if src[s][c] >= 0]
    return decoded, cols, shares


def merge_nbest(hyps_per_utt: Sequence[Sequence[Sequence[Hashable]]], mode: str = "exact", device=0, *,
                slack: int = 0, sentinel: int = -1) -> SlotTable:
    """The slot tables of a batch: ``hyps_per_utt[u]`` = [top-1, hypothesis 2, ..., hypothesis N] as token
    lists (N >= 1).  One ``rs_align`` launch over all pairs, then the two ``rs_cn_merge`` launches.
    ``slack`` / ``sentinel``: extra elements allocated behind the K and table buffers and the value both
    are filled with before the launches (the tests look for writes outside the table)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}")
    if any(len(h) == 0 for h in hyps_per_utt):
        raise ValueError("every utterance needs at least one hypothesis")
    if not torch.cuda.is_available():
        raise RuntimeError("librescore needs a HIP GPU (no CPU fallback)")
    lib = _lib.load()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    hyps = [[list(t) for t in h] for h in hyps_per_utt]
    vocab: dict = {}
    ids = [[[vocab.setdefault(t, len(vocab)) for t in hyp] for hyp in h] for h in hyps]
    if GAP in vocab:
        raise ValueError('the gap token "*" cannot be a hypothesis token')
    U = len(ids)
    utt_off = _off([len(h) for h in ids])
    hyp_len = np.asarray([len(t) for h in ids for t in h], np.int32)
    max_len = int(hyp_len.max(initial=0))
    if max_len > MAX_LEN:
        raise ValueError(f"token lists longer than {MAX_LEN} are not supported")
    _, ri, hi, out_off, n_al = align.align_ids([h[0] for h in ids for _ in h[1:]], [t for h in ids for t in h[1:]],
                                              dev.index or 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    d = {"utt_off_h": utt_off, "utt_off": T(utt_off), "hyp_off": T(_off(hyp_len)),
         "tok": T(np.asarray([t for h in ids for hyp in h for t in hyp] + [0], np.int32))}
    d_ri, d_hi, d_oo, d_n = T(ri), T(hi), T(out_off), T(np.append(n_al, 0).astype(np.int32))
    d_len = T(np.append(hyp_len, 0).astype(np.int32))
    top_len = hyp_len[utt_off[:-1]].astype(np.int64) if U else np.zeros(0, np.int64)
    gap_off = _off(top_len + 1, np.int64)
    d_goff = T(gap_off)
    d_K = d["K"] = torch.full((max(int(gap_off[-1]), 1) + slack,), sentinel, dtype=torch.int32, device=dev)
    d_ns = torch.zeros(max(U, 1), dtype=torch.int32, device=dev)
    args = [_lib.ptr(d_ri), _lib.ptr(d_hi), _lib.ptr(d_oo), _lib.ptr(d_n), _lib.ptr(d["utt_off"]), _lib.ptr(d_len),
            U, max_len, _lib.ptr(d_goff), _lib.ptr(d_K)]
    _lib.check(lib.rs_cn_merge(*args, _lib.ptr(d_ns), None, None, None, 0, MODES[mode], _lib.stream_ptr(dev)))
    n_slots = d_ns.cpu().numpy()[:U].astype(np.int64)
    slot_off = _off(n_slots)
    cell_off = _off(n_slots * np.diff(utt_off), np.int64)
    cap = int(cell_off[-1])
    d["slot_off"], d["cell_off"] = T(slot_off), T(cell_off)
    d["src"] = torch.full((max(cap, 1) + slack,), sentinel, dtype=torch.int32, device=dev)
    _lib.check(lib.rs_cn_merge(*args, None, _lib.ptr(d["slot_off"]), _lib.ptr(d["cell_off"]), _lib.ptr(d["src"]),
                               d["src"].numel(), MODES[mode], _lib.stream_ptr(dev)))
    return SlotTable(hyps, ids, vocab, mode, dev, d)


def consensus_weights(am, lm, hyp_len, utt_off, weight: float, scale: float = 1.0) -> np.ndarray:
    """float64 [n_hyp]: per utterance softmax of scale * ((1 - w) * am / len + w * lm / len), the
    length-normalised fusion of rescore.py:13-58."""
    am, lm = np.asarray(am, np.float64), np.asarray(lm, np.float64)
    ln = np.maximum(np.asarray(hyp_len, np.float64), 1.0)
    fused = scale * ((1.0 - weight) * am / ln + weight * lm / ln)
    out = np.empty_like(fused)
    for a, b in zip(utt_off[:-1], utt_off[1:]):
        if b > a:
            e = np.exp(fused[a:b] - fused[a:b].max())
            out[a:b] = e / e.sum()
    return out


def align_features(table: SlotTable, labels: Sequence[Sequence[int]], tokenizer, gap_token: str = GAP,
                   utt_ids: Optional[Sequence[str]] = None) -> List[dict]:
    """The Nbest_Align/preprocess.py:142-157 row per utterance: slot 0 as [CLS] + its entries, every later
    slot as [SEP] + its entries (no closing [SEP]), token types alternating 0 / 1 per slot, prediction_pos
    the index of each slot's leading [CLS] / [SEP].  Assembled on the host."""
    rows = []
    for u, slots in enumerate(table.tokens()):
        toks, types, pos = [], [], []
        for s, slot in enumerate(slots):
            pos.append(len(toks))
            toks += ["[CLS]" if s == 0 else "[SEP]"] + [gap_token if t == GAP else t for t in slot]
            types += [s % 2] * (len(slot) + 1)
        ids = [int(i) for i in tokenizer.convert_tokens_to_ids(toks)]
        row = {"utt_id": utt_ids[u]} if utt_ids is not None else {}
        row.update({"input_ids": ids, "attention_masks": [1] * len(ids), "token_type_ids": types,
                    "prediction_pos": pos, "labels": [int(x) for x in labels[u]]})
        rows.append(row)
    return rows
