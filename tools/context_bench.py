"""Cost of context-conditioned scoring: ``score_nbest(token_types, score_from)`` on the pairs
``[CLS] context [SEP] hypothesis [SEP]`` (``data.with_context``, one seeded context of CTX tokens per
utterance) against the plain ``rs_pll_score`` call on the same hypotheses (40 utterances x N = 50,
BERT-base, fp16x3, the bench's weights and chunk size).  Both are warmed up, then timed as the
median of CALLS calls, each closed by a device synchronise; the plain call is timed first and again
last (the noise reference).  One more pair call each with RS_DEDUP=1 and RS_DEDUP=0 under the
profiler gives the layer-0 Q/K/V flops: equal figures mean the pairs' chunks ran without the dedup
(fp16x3: a chunk with a sequence over 64 tokens).
Appends JSON lines to profiles/context_bench.jsonl.
Usage: python tools/context_bench.py [--calls 20] [--utts 40] [--nbest 50] [--ctx 32] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--utts", type=int, default=40)
    ap.add_argument("--nbest", type=int, default=50)
    ap.add_argument("--ctx", type=int, default=32)
    ap.add_argument("--max-rows", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "context_bench.jsonl"))
    args = ap.parse_args()
    nb = D.synthetic_nbest(args.utts, args.nbest, seed=1, hard=True)
    rng = np.random.default_rng(3)
    ctx = rng.integers(D.FIRST_WORD_ID, BERT_BASE.vocab, args.utts * args.ctx).astype(np.int32)
    tokens, off, types, score_from, _ = D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx,
                                                       np.arange(args.utts + 1) * args.ctx)
    s = PLLScorer(make_weights(BERT_BASE, seed=1234), BERT_BASE, device=0, max_rows=args.max_rows, precision="fp16x3")
    tok, ptok, ptype = s._dev_tokens(nb.tokens), s._dev_tokens(tokens), s._dev_tokens(types)
    rows = int((np.diff(nb.hyp_off) - 2).sum())

    def pair_call():
        return s.score_nbest(ptok, off, token_types=ptype, score_from=score_from)
    base = timed(lambda: s.score_nbest(tok, nb.hyp_off), args.calls)
    pair = timed(pair_call, args.calls)
    again = timed(lambda: s.score_nbest(tok, nb.hyp_off), args.calls)
    flops = {}
    for dd in ("1", "0"):
        os.environ["RS_DEDUP"] = dd
        s.profile(True)
        pair_call()
        flops[dd] = s.profile_read()["qkv"][2]
        s.profile(False)
    os.environ.pop("RS_DEDUP")
    s.close()
    common = {"utts": args.utts, "n_best": args.nbest, "hypotheses": int(nb.n_hyp), "masked_rows": rows,
              "calls": args.calls, "max_rows": args.max_rows, "precision": "fp16x3", "context_tokens": args.ctx,
              "device": torch.cuda.get_device_name(0)}
    recs = [{"variant": "rs_pll_score (plain)", "median_ms": base[0], "min_ms": base[1], "max_ms": base[2], "ratio": 1.0,
             "token_rows": int((np.diff(nb.hyp_off) * (np.diff(nb.hyp_off) - 2)).sum())},
            {"variant": "context pairs, types + score_from", "median_ms": pair[0], "min_ms": pair[1], "max_ms": pair[2],
             "ratio": pair[0] / base[0], "token_rows": int((np.diff(off) * (np.diff(off) - score_from - 1)).sum()),
             "max_pair_len": int(np.diff(off).max()), "qkv_flops_dedup_on": flops["1"], "qkv_flops_dedup_off": flops["0"],
             "chunks_deduplicated": bool(flops["1"] < flops["0"])},
            {"variant": "rs_pll_score (plain, after)", "median_ms": again[0], "min_ms": again[1], "max_ms": again[2],
             "ratio": again[0] / base[0]}]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in recs:
            r.update(common)
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
