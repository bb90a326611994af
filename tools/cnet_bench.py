"""Confusion-network steps on the C3 shape (N = 50, L ~ 35): cnet.merge_nbest (which contains the
rs_align launch), SlotTable.oracle and SlotTable.vote on the GPU against the plain-Python restatement
(tests/cnet_ref.py) on the same lists.  GPU calls are warmed up, then timed as the median of CALLS calls by
the host clock, each ending in a device synchronise; ``align_ids`` is timed alone on the same pairs to
show its part of a merge call.  The restatement runs once over the first REF_UTTS utterances (it is
minutes over all of them) and is reported per utterance.  Appends one JSON line to the output file.
Usage: python tools/cnet_bench.py [--utts 256] [--nbest 50] [--calls 7] [--ref-utts 16]
                                  [--out profiles/cnet_bench.jsonl]"""
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import __graft_entry__  # noqa: E402

__graft_entry__._import_pkg()
import cnet_ref as C  # noqa: E402
from asr_rescoring_amd import align, cnet, data as D  # noqa: E402


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
    ap.add_argument("--ref-utts", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cnet_bench.jsonl"))
    a = ap.parse_args()
    nb = D.synthetic_nbest(a.utts, a.nbest, seed=1, vocab=3000, len_lo=25, len_hi=45, max_edits=5)
    lists = [[nb.hyp_words(h).tolist() for h in range(nb.utt_off[u], nb.utt_off[u + 1])] for u in range(nb.n_utt)]
    refs = [[int(x) for x in r] for r in nb.refs]
    rng = np.random.default_rng(0)
    w = torch.from_numpy(cnet.consensus_weights(nb.am, rng.normal(-40, 8, nb.n_hyp), nb.hyp_len(), nb.utt_off, 0.5))
    pairs_r = [h[0] for h in lists for _ in h[1:]]
    pairs_h = [t for h in lists for t in h[1:]]
    res = {"utts": a.utts, "nbest": a.nbest, "mean_len": float(np.mean([len(t) for h in lists for t in h])),
           "calls": a.calls, "device": torch.cuda.get_device_name(0)}
    res["merge"] = timed(lambda: cnet.merge_nbest(lists, "exact"), a.calls)
    res["align_ids_alone"] = timed(lambda: align.align_ids(pairs_r, pairs_h), a.calls)
    table = cnet.merge_nbest(lists, "exact")
    res["slots"] = int(table.slot_off[-1])
    res["oracle"] = timed(lambda: table.oracle(refs), a.calls)
    res["vote"] = timed(lambda: table.vote_device(w), a.calls)
    total = sum(res[k]["median_ms"] for k in ("merge", "oracle", "vote"))
    res["gpu_total_ms"] = total
    res["share"] = {k: res[k]["median_ms"] / total for k in ("merge", "oracle", "vote")}
    res["share"]["align_ids_of_merge"] = res["align_ids_alone"]["median_ms"] / res["merge"]["median_ms"]
    # the restatement, once, on the first REF_UTTS utterances of the same lists
    n = min(a.ref_utts, a.utts)
    t0 = time.perf_counter()
    tabs = [C.table_tokens(h, C.closed_form(h, C.EXACT)) for h in lists[:n]]
    t1 = time.perf_counter()
    orc = [C.dp_oracle(t, r) for t, r in zip(tabs, refs[:n])]
    t2 = time.perf_counter()
    wn = w.numpy()
    votes = [C.vote(t, wn[nb.utt_off[u]:nb.utt_off[u + 1]]) for u, t in enumerate(tabs)]
    t3 = time.perf_counter()
    dist, labels = table.oracle(refs)
    assert [int(d) for d in dist[:n]] == [o[0] for o in orc] and all(labels[u].tolist() == orc[u][1] for u in range(n))
    assert table.tokens()[:n] == tabs and table.vote(wn)[0][:n] == [v[3] for v in votes]
    ref_ms = {"merge": (t1 - t0) * 1e3 / n, "oracle": (t2 - t1) * 1e3 / n, "vote": (t3 - t2) * 1e3 / n}
    res["restatement_ms_per_utt"] = ref_ms
    res["restatement_utts"] = n
    res["gpu_ms_per_utt"] = {k: res[k]["median_ms"] / a.utts for k in ("merge", "oracle", "vote")}
    res["speedup"] = {k: ref_ms[k] / res["gpu_ms_per_utt"][k] for k in ref_ms}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
