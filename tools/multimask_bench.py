"""Cost and rerank effect of the strided PLL approximation (rs_pll_score_sets through
``PLLScorer.score_nbest(variant="strided")``) against exact PLL (rs_pll_score) on the synthetic set of
tools/span_bench.py (40 utterances x N = 50, BERT-base, fp16x3, the bench's weights and chunk size).

Timing: every variant is warmed up, then timed as the median of CALLS calls, each closed by a device
synchronise; rs_pll_score is timed first and again last (the noise reference); score_sets runs at
strides 1, 2, 4, 8 and ">= L" (one position per row: rs_pll_score's own rows, without the layer-0
dedup).  Every line carries its forwards per call and its ratio to rs_pll_score.

Rerank effect: the LM is fine-tuned the way bench.py fine-tunes its own (train.finetune_mlm_on_texts on
the set's reference sentences), then rerank.find_best_weight runs with exact PLL and with each stride:
best weight, corpus CER, and the share of utterances whose pick (at the variant's best weight) equals
the exact-PLL pick (at its best weight).  The set is synthetic and the LM has seen its references:
the CER figures are in-sample and say how far the approximation moves the fused pick, not how good
the LM is.

Appends one JSON line per measurement to profiles/multimask_bench.jsonl.
Usage: python tools/multimask_bench.py [--calls 20] [--utts 40] [--nbest 50] [--finetune-steps 300]"""
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
from asr_rescoring_amd import data as D, rerank  # noqa: E402
from asr_rescoring_amd.scorer import PLLScorer  # noqa: E402
from asr_rescoring_amd.weights import BERT_BASE, make_weights  # noqa: E402

STRIDES = [1, 2, 4, 8]


def timed(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--utts", type=int, default=40)
    ap.add_argument("--nbest", type=int, default=50)
    ap.add_argument("--max-rows", type=int, default=262144)
    ap.add_argument("--finetune-steps", type=int, default=300)
    ap.add_argument("--finetune-lr", type=float, default=1e-4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multimask_bench.jsonl"))
    args = ap.parse_args()
    calls = max(args.calls, 20)
    nb = D.synthetic_nbest(args.utts, args.nbest, seed=1, hard=True)
    L = np.diff(nb.hyp_off) - 2
    big = int(L.max())                                   # stride >= L: singleton rows
    common = {"utts": args.utts, "n_best": args.nbest, "hypotheses": int(nb.n_hyp), "positions": int(L.sum()),
              "mean_L": float(L.mean()), "max_rows": args.max_rows, "precision": "fp16x3",
              "device": torch.cuda.get_device_name(0)}
    weights0 = make_weights(BERT_BASE, seed=1234)
    recs = []

    # ---- timing ------------------------------------------------------------------------------
    s = PLLScorer(weights0, BERT_BASE, device=0, max_rows=args.max_rows, precision="fp16x3")
    tok = s._dev_tokens(nb.tokens)
    base = timed(lambda: s.score_nbest(tok, nb.hyp_off), calls)

    def timing(variant, t, forwards):
        return {"kind": "timing", "variant": variant, "median_ms": t[0], "min_ms": t[1], "max_ms": t[2],
                "ratio": t[0] / base[0], "forwards": int(forwards), "calls": calls}

    recs.append(timing("rs_pll_score", base, L.sum()))
    for k in STRIDES + [big]:
        plan = D.pll_strided(nb.hyp_off, k)
        t = timed(lambda: s.score_sets(tok, nb.hyp_off, *plan), calls)
        recs.append(timing(f"score_sets stride {k}" if k != big else f"score_sets stride >= L ({big})", t, plan[0][-1]))
    again = timed(lambda: s.score_nbest(tok, nb.hyp_off), calls)     # the noise reference
    recs.append(timing("rs_pll_score (after)", again, L.sum()))
    s.close()

    # ---- rerank effect -----------------------------------------------------------------------
    if args.finetune_steps > 0:
        from asr_rescoring_amd.train import finetune_mlm_on_texts
        w_ft, losses = finetune_mlm_on_texts(weights0, nb.refs, BERT_BASE, steps=args.finetune_steps,
                                             lr=args.finetune_lr, seed=0, device=0)
        torch.cuda.synchronize()
        s = PLLScorer(w_ft, BERT_BASE, device=0, max_rows=args.max_rows, precision="fp16x3")
        grid = rerank.weight_grid("norm")
        picks = {}
        for k in [0] + STRIDES:                           # 0: exact PLL
            lm = (s.score_nbest(tok, nb.hyp_off) if k == 0 else
                  s.score_nbest(tok, nb.hyp_off, variant="strided", stride=k)).cpu().numpy()
            bw, bcer, arg, _ = rerank.find_best_weight(nb, lm, n_best=args.nbest, device=0)
            picks[k] = arg[int(np.argmin(np.abs(np.asarray(grid) - bw)))]
            recs.append({"kind": "rerank", "variant": "exact PLL" if k == 0 else f"stride {k}", "best_weight": bw,
                         "cer_synthetic_in_sample": bcer,
                         "same_pick_as_exact": float((picks[k] == picks[0]).mean()),
                         "finetune_steps": args.finetune_steps, "finetune_lr": args.finetune_lr,
                         "finetune_first_loss": float(losses[0]), "finetune_final_loss": float(losses[-1])})
        s.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in recs:
            r.update(common)
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
