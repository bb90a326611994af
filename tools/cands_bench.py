"""Candidate-set scores and the LM-weighted consensus decode on the C3 shape (N = 50, L ~ 35), bert-base.

(a) ``PLLScorer.score_cands`` against ``rs_masked_logprob_multi`` on the same rows (one [MASK] row per
    contested top-1 position of the set) at 1, 8 and 50 candidates per query: the ratio of the call times.
(b) ``rerank.consensus_decode_lm`` end to end (merge, the forwards, the host vote, the CER kernels) beside
    ``rerank.consensus_decode``, 256 utterances x N = 50.
(c) On bench.py's own set (``synthetic_nbest(utts, 50, seed=1, hard=True)``, the LM fine-tuned 300 steps on
    the set's references: in-sample), the corpus CER of the fused argmax, the consensus decode and the
    consensus decode with the LM over the lam grid.
GPU calls are warmed up twice, then timed as the median of CALLS calls by the host clock, each ending in
a device synchronise.  Appends one JSON line to the output file.
Usage: python tools/cands_bench.py [--utts 256] [--nbest 50] [--calls 7] [--cer-utts 200] [--finetune-steps 300]
                                   [--out profiles/cands_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__  # noqa: E402

__graft_entry__._import_pkg()
from asr_rescoring_amd import _lib, cnet, data as D, rerank  # noqa: E402
from asr_rescoring_amd.scorer import PLLScorer  # noqa: E402
from asr_rescoring_amd.weights import BERT_BASE, make_weights  # noqa: E402


def timed(fn, calls, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--nbest", type=int, default=50)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--cer-utts", type=int, default=200)
    ap.add_argument("--finetune-steps", type=int, default=300)
    ap.add_argument("--max-rows", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cands_bench.jsonl"))
    a = ap.parse_args()
    weights = make_weights(BERT_BASE, seed=1234)
    scorer = PLLScorer(weights, BERT_BASE, device=0, max_rows=a.max_rows)
    res = {"utts": a.utts, "nbest": a.nbest, "calls": a.calls, "device": torch.cuda.get_device_name(0),
           "precision": "fp16x3"}

    # ---- (a) score_cands / rs_masked_logprob_multi on the decode's own rows
    nb = D.synthetic_nbest(a.utts, a.nbest, seed=1, len_lo=25, len_hi=45, max_edits=5)
    rng = np.random.default_rng(0)
    lm = rng.normal(-40, 8, nb.n_hyp)
    c0 = rerank._ConsensusLM(nb, scorer, 1 << 30, 0)          # the rows consensus_decode_lm scores
    pcs, d_rows, seq_off, qpos = c0.rows()
    n_slots = int(c0.table.slot_off[-1])
    n_q = len(pcs)
    q_off = np.arange(n_q + 1, dtype=np.int32)
    res.update({"slots": n_slots, "contested": n_q, "token_rows": int(seq_off[-1]),
                "mean_candidates": float(np.mean([len(t) for *_, t, _ in pcs]))})
    d_lab = torch.from_numpy(np.asarray([t[0] for *_, t, _ in pcs], np.int32)).to(scorer.device)
    out1 = torch.empty(n_q, dtype=torch.float32, device=scorer.device)

    def multi():
        _lib.check(scorer.lib.rs_masked_logprob_multi(scorer.handle, _lib.ptr(d_rows), seq_off.ctypes.data, n_q,
                                                      q_off.ctypes.data, qpos.ctypes.data, _lib.ptr(d_lab), _lib.ptr(out1),
                                                      _lib.stream_ptr(scorer.device)))
    res["masked_logprob_multi"] = timed(multi, a.calls)
    res["score_cands"] = {}
    for k in (1, 8, 50):
        cand = rng.integers(0, BERT_BASE.vocab, size=(n_q, k)).astype(np.int32)
        cand[:, 0] = d_lab.cpu().numpy()
        c_off = (np.arange(n_q + 1) * k).astype(np.int32)
        t = timed(lambda: scorer.score_cands(d_rows, seq_off, q_off, qpos, c_off, cand.reshape(-1)), a.calls)
        got = scorer.score_cands(d_rows, seq_off, q_off, qpos, c_off, cand.reshape(-1)).view(n_q, k)[:, 0]
        multi()
        assert torch.equal(got.view(torch.int32), out1.view(torch.int32)), "score_cands != rs_masked_logprob_multi"
        t["ratio_to_multi"] = t["median_ms"] / res["masked_logprob_multi"]["median_ms"]
        res["score_cands"][str(k)] = t
    res["masked_logprob_multi_after"] = timed(multi, a.calls)

    # ---- (b) the decode end to end beside the plain consensus decode
    res["consensus_decode"] = timed(lambda: rerank.consensus_decode(nb, lm, 0.5), a.calls)
    res["consensus_decode_lm"] = timed(lambda: rerank.consensus_decode_lm(nb, lm, scorer, 0.5, 0.5), a.calls)
    c = rerank._ConsensusLM(nb, scorer, 1 << 30, 0)
    w = c.weights(lm, 0.5, 1.0)
    t0 = time.perf_counter()
    pc = c.table.position_candidates()
    t1 = time.perf_counter()
    slot_lp, _ = c.slot_lp()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    cnet.slot_lm_vote(c.table, w, slot_lp, 0.5)
    t3 = time.perf_counter()
    res["decode_lm_parts_ms"] = {"position_candidates": (t1 - t0) * 1e3, "rows_and_forwards": (t2 - t1) * 1e3,
                                 "slot_lm_vote_host": (t3 - t2) * 1e3, "contested": len(pc)}
    scorer.close()

    # ---- (c) CER on bench.py's own fine-tuned set (in-sample: the LM saw the references)
    if a.cer_utts > 0:
        from asr_rescoring_amd.train import finetune_mlm_on_texts
        nb2 = D.synthetic_nbest(a.cer_utts, a.nbest, seed=1, hard=True)
        w_ft, losses = finetune_mlm_on_texts(weights, nb2.refs, BERT_BASE, steps=a.finetune_steps, lr=1e-4, seed=0,
                                             device=0)
        torch.cuda.synchronize()
        s2 = PLLScorer(w_ft, BERT_BASE, device=0, max_rows=a.max_rows)
        lm2 = s2.score_nbest(nb2.tokens, nb2.hyp_off).cpu().numpy()
        bw, bcer, _, cers = rerank.find_best_weight(nb2, lm2, n_best=a.nbest, device=0)
        cw, ccer, _ = rerank.find_best_weight_consensus(nb2, lm2, a.nbest, 1.0, "exact", 0)
        blam, lcer, lcers = rerank.find_best_weight_consensus_lm(nb2, lm2, s2, cw, rerank.LAM_GRID, 1.0, a.nbest, 0)
        _, _, info = rerank.consensus_decode_lm(nb2, lm2, s2, cw, 1.0, 1.0, a.nbest, 0, return_info=True)
        s2.close()
        res["cer"] = {"utts": a.cer_utts, "finetune_steps": a.finetune_steps,
                      "finetune_loss_first_final": [losses[0], losses[-1]], "set": "in-sample (bench.py's synthetic set)",
                      "am_only": float(cers[0]), "argmax": bcer, "argmax_weight": bw, "consensus": ccer,
                      "consensus_weight": cw, "consensus_lm": dict(zip(map(str, rerank.LAM_GRID), map(float, lcers))),
                      "best_lam": blam, "best_consensus_lm": lcer, "contested": info["n_contested"],
                      "forwards": info["n_forwards"], "pll_forwards": int(nb2.n_forwards())}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
