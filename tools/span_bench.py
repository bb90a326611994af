"""Cost of span-masked PLL: rs_pll_score_spans with rs_pll_score's own rows (the degenerate spans), with
the PLL-word-l2r rows and with the PLL-whole-word rows, against rs_pll_score on the same synthetic set
(40 utterances x N = 50, BERT-base, fp16x3, the bench's weights and chunk size; seeded word lengths
1..4).  Every variant is warmed up, then timed as the median of CALLS calls, each closed by a device
synchronise; rs_pll_score is timed first and again last (the noise reference).
Appends one JSON line per variant to profiles/span_bench.jsonl.
Usage: python tools/span_bench.py [--calls 20] [--utts 40] [--nbest 50] [--out profiles/span_bench.jsonl]"""
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
from asr_rescoring_amd import data as D  # noqa: E402
from asr_rescoring_amd.scorer import PLLScorer  # noqa: E402
from asr_rescoring_amd.weights import BERT_BASE, make_weights  # noqa: E402


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


def word_starts(hyp_off, seed, max_word=4):
    """uint8 per token: seeded word lengths 1..max_word inside every hypothesis."""
    rng = np.random.default_rng(seed)
    ws = np.zeros(int(hyp_off[-1]), np.uint8)
    for h in range(len(hyp_off) - 1):
        a, b = int(hyp_off[h]), int(hyp_off[h + 1])
        ws[a] = ws[b - 1] = 1
        p = a + 1
        while p < b - 1:
            ws[p] = 1
            p += int(rng.integers(1, max_word + 1))
    return ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--utts", type=int, default=40)
    ap.add_argument("--nbest", type=int, default=50)
    ap.add_argument("--max-rows", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "span_bench.jsonl"))
    args = ap.parse_args()
    calls = max(args.calls, 20)
    nb = D.synthetic_nbest(args.utts, args.nbest, seed=1, hard=True)
    ws = word_starts(nb.hyp_off, seed=2)
    s = PLLScorer(make_weights(BERT_BASE, seed=1234), BERT_BASE, device=0, max_rows=args.max_rows, precision="fp16x3")
    tok = s._dev_tokens(nb.tokens)
    rows = int((nb.hyp_off[1:] - nb.hyp_off[:-1] - 2).sum())
    base = timed(lambda: s.score_nbest(tok, nb.hyp_off), calls)
    recs = [{"variant": "rs_pll_score", "median_ms": base[0], "min_ms": base[1], "max_ms": base[2], "ratio": 1.0,
             "mean_span": 1.0}]
    for variant in D.PLL_VARIANTS:
        spans = D.pll_spans(nb.hyp_off, ws, variant)
        t = timed(lambda: s.score_spans(tok, nb.hyp_off, *spans), calls)
        recs.append({"variant": f"rs_pll_score_spans {variant}", "median_ms": t[0], "min_ms": t[1], "max_ms": t[2],
                     "ratio": t[0] / base[0], "mean_span": float((spans[2] - spans[1]).mean())})
    again = timed(lambda: s.score_nbest(tok, nb.hyp_off), calls)     # the noise reference
    recs.append({"variant": "rs_pll_score (after)", "median_ms": again[0], "min_ms": again[1], "max_ms": again[2],
                 "ratio": again[0] / base[0], "mean_span": 1.0})
    s.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in recs:
            r.update({"utts": args.utts, "n_best": args.nbest, "hypotheses": int(nb.n_hyp), "masked_rows": rows,
                      "calls": calls, "max_rows": args.max_rows, "precision": "fp16x3",
                      "device": torch.cuda.get_device_name(0)})
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
