"""Step time of MLM training with the head over the labelled rows only (rs_train_step_mlm_labeled,
``MLMTrainer.step(ignore_index=-100)``) against the head over every row (rs_train_step_mlm), on the
BERT-base shape with the CLI's default dropout (0.1 / 0.1), AdamW updates on.

Three steps at 32 rows x 34 tokens (the reference's batch of do_job rows) and again at 32 x 128:
  a  the old entry on 32 do_job rows, a label at every position            (head rows = M)
  b  the new entry on the same rows labelled at their [MASK] only          (head rows = 32)
  c  the new entry on 32 sentences of the same length under 15 % dynamic masks (``train.mask_tokens``)

Method: a step is timed by the host clock around ``MLMTrainer.step``, which ends in a device
synchronise (it includes the step's host work and its small uploads: what a training loop pays).
Every variant is warmed up; the timed repetitions are interleaved (a b c a b c ...), so drift hits
all three alike.  The whole measurement runs in a fresh child process and is repeated over ROUNDS
rounds; reported: the median over all repetitions, the smallest and largest per-round median (the
run-to-run spread), and the ratios b / a and c / a of the medians.

``--parent-tree DIR`` (a checkout of the parent commit with its library built): step a alone is
timed on that build and on this tree, alternating child processes round by round, to show that the
old entry did not move.

The head's workspace bytes (transform pre-GELU / GELU / LN outputs, LN statistics, logits, and for
the new entry the gathered hidden rows) are computed from the layout of ``prepare()``
(csrc/train_api.hip): every region rounded up to 64 floats.

Appends one JSON line per record to profiles/mlm_sparse_bench.jsonl.
Usage: python tools/mlm_sparse_bench.py [--reps 20] [--rounds 3] [--parent-tree DIR]"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 34), (32, 128)]
H, V = 768, 21128


def import_pkg(tree):
    """The package of ``tree`` (this repository or a checkout of another commit)."""
    d = os.path.join(tree, "asr-rescoring_amd")
    spec = importlib.util.spec_from_file_location("asr_rescoring_amd", os.path.join(d, "__init__.py"),
                                                  submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["asr_rescoring_amd"] = mod
    spec.loader.exec_module(mod)


def head_bytes(rows, labelled):
    al = lambda n: (n + 63) // 64 * 64
    return 4 * (3 * al(rows * H) + al(rows * 2) + al(rows * V) + (al(rows * H) if labelled else 0))


def batches(n_rows, T):
    """(a, b, c) step arguments at n_rows x T tokens, seeded."""
    import numpy as np
    from asr_rescoring_amd.train import do_job_rows, pad_rows
    from asr_rescoring_amd.weights import BERT_BASE as S
    rng = np.random.default_rng(T)
    sent = lambda: [S.cls_id] + rng.integers(1000, S.vocab, T - 2).tolist() + [S.sep_id]
    ids, off, lab = do_job_rows([sent()], S.mask_id)
    rows = [ids[off[i]:off[i + 1]].tolist() for i in range(n_rows)]
    labs = [lab[off[i]:off[i + 1]].tolist() for i in range(n_rows)]
    out = {"a": (pad_rows(rows, labs), {})}
    try:
        from asr_rescoring_amd.train import mask_tokens
    except ImportError:                                  # a tree from before the labelled step: a only
        return out
    only = [[l if r == S.mask_id else -100 for r, l in zip(row, lb)] for row, lb in zip(rows, labs)]
    out["b"] = (pad_rows(rows, only, label_pad=-100), {"ignore_index": -100})
    m, l = mask_tokens([sent() for _ in range(n_rows)], S, (1, T), 0.15)
    out["c"] = (pad_rows(m, l, label_pad=-100), {"ignore_index": -100})
    for k in "bc":
        out[k][1]["n_lab"] = int((out[k][0][2] != -100).sum())
    return out


def child(args):
    """One process: a trainer, every requested variant at both shapes, interleaved repetitions."""
    import_pkg(args.tree)
    import torch
    from asr_rescoring_amd.train import MLMTrainer
    from asr_rescoring_amd.weights import BERT_BASE, make_weights
    tr = MLMTrainer(make_weights(BERT_BASE, seed=1234), BERT_BASE, device=0, lr=1e-5, dropout_seed=1)
    res = {"device": torch.cuda.get_device_name(0), "times_ms": {}, "n_lab": {}}
    try:
        for n_rows, T in SHAPES:
            bt = batches(n_rows, T)
            todo = [(k, bt[k][0], {x: y for x, y in bt[k][1].items() if x != "n_lab"}) for k in args.variants
                    if k in bt]
            for k, b, kw in todo:
                res["n_lab"][f"{k}{T}"] = bt[k][1].get("n_lab", n_rows * T)
                for _ in range(args.warmup):
                    tr.step(*b, **kw)
            ms = {k: [] for k, _, _ in todo}
            for _ in range(args.reps):
                for k, b, kw in todo:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tr.step(*b, **kw)
                    ms[k].append((time.perf_counter() - t0) * 1e3)
            for k in ms:
                res["times_ms"][f"{k}{T}"] = ms[k]
    finally:
        tr.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(tree, variants, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--variants", variants,
           "--reps", str(args.reps), "--warmup", str(args.warmup)]
    env = dict(os.environ)
    env.pop("RS_LIBRESCORE", None)                       # each tree loads its own library
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout, check=True).stdout
    print(f"measured {variants} on {tree}", file=sys.stderr, flush=True)
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


def summary(rounds):
    """rounds: per-round lists of step times -> median over all, spread of the per-round medians"""
    meds = [statistics.median(r) for r in rounds]
    return {"median_ms": statistics.median([x for r in rounds for x in r]), "round_median_min_ms": min(meds),
            "round_median_max_ms": max(meds), "reps": sum(len(r) for r in rounds), "rounds": len(rounds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mlm_sparse_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    ap.add_argument("--variants", default="abc", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {"abc": [], "a": [], "parent_a": []}
    for _ in range(args.rounds):
        runs["abc"].append(run_child(REPO, "abc", args))
        if args.parent_tree:
            runs["parent_a"].append(run_child(args.parent_tree, "a", args))
            runs["a"].append(run_child(REPO, "a", args))
    recs = []
    first = runs["abc"][0]
    for n_rows, T in SHAPES:
        M = n_rows * T
        s = {k: summary([r["times_ms"][f"{k}{T}"] for r in runs["abc"]]) for k in "abc"}
        for k in "abc":
            n_lab = first["n_lab"][f"{k}{T}"]
            recs.append({"kind": "step", "variant": k, "rows": n_rows, "T": T, "tokens": M, "head_rows": n_lab,
                         "head_workspace_bytes": head_bytes(n_lab, k != "a"),
                         "ratio_to_a": s[k]["median_ms"] / s["a"]["median_ms"], **s[k], "device": first["device"]})
        if args.parent_tree:
            here = summary([r["times_ms"][f"a{T}"] for r in runs["a"]])
            par = summary([r["times_ms"][f"a{T}"] for r in runs["parent_a"]])
            recs.append({"kind": "old_entry_vs_parent", "rows": n_rows, "T": T, "this_tree": here, "parent": par,
                         "ratio": here["median_ms"] / par["median_ms"], "device": first["device"]})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in recs:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
