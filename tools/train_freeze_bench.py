"""Step time of the native trainers with frozen tensors, and the cost of gradient accumulation and
clipping, on the BERT-base shape with the CLI's default dropout (0.1 / 0.1), AdamW updates on.

Two step shapes, the ones the trainer numbers of DESIGN §8 use (tools/bench_extra.py c2train, mlmtrain):
  rb   RescoreBert MD_MWER, 3 utterances x N=50 hypotheses per step (about 5.3k tokens)
  mlm  MLM fine-tuning, 32 padded do_job rows per step (about 1.1k tokens), a label at every position

Per shape, a full updating step with
  none   nothing frozen
  emb    freeze("bert.embeddings")
  half   freeze("bert.embeddings", "bert.encoder.layer.0" .. "bert.encoder.layer.5")
  head   freeze("bert"): everything but the head (the MLM head's tied decoder weight, being the word
         embeddings, is frozen with them)
and the accumulation path:
  micro  step(update=False), the micro-batch step
  accap  accumulate(1) + apply(max_grad_norm=1): what an optimizer step adds on top of its micro-steps
         (the fp32 accumulate, the float64 norm with its read-back, the scaled AdamW, the clear)

Method: a step is timed by the host clock around the call, which ends in a device synchronise (it
includes the step's host work and its small uploads: what a training loop pays).  Every variant is
warmed up; the timed repetitions are interleaved (none emb half head micro accap none ...), so drift
hits all alike; the trainable set is switched outside the timed region.  The whole measurement runs in
a fresh child process and is repeated over ROUNDS rounds; reported: the median over all repetitions,
the smallest and largest per-round median (the run-to-run spread), and the ratio to "none".

``--parent-tree DIR`` (a checkout of the parent commit with its library built): the "none" step alone
is timed on that build and on this tree, alternating child processes round by round, to show that the
step without any of the options did not move.

Appends one JSON line per record to profiles/train_freeze_bench.jsonl.
Usage: python tools/train_freeze_bench.py [--reps 20] [--rounds 3] [--parent-tree DIR]"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREEZE = {"none": (), "emb": ("bert.embeddings",),
          "half": ("bert.embeddings",) + tuple(f"bert.encoder.layer.{i}" for i in range(6)), "head": ("bert",)}
VARIANTS = ["none", "emb", "half", "head", "micro", "accap"]


def import_pkg(tree):
    """The package of ``tree`` (this repository or a checkout of another commit)."""
    d = os.path.join(tree, "asr-rescoring_amd")
    spec = importlib.util.spec_from_file_location("asr_rescoring_amd", os.path.join(d, "__init__.py"),
                                                  submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["asr_rescoring_amd"] = mod
    spec.loader.exec_module(mod)


def workloads():
    """name -> (trainer, step(update)) on seeded data, the batches of tools/bench_extra.py."""
    import numpy as np
    from asr_rescoring_amd import data as D
    from asr_rescoring_amd.train import MLMTrainer, RescoreBertTrainer, do_job_rows, pad_rows
    from asr_rescoring_amd.weights import BERT_BASE, make_weights

    def rb():
        w = make_weights(BERT_BASE, seed=1234, with_cls_linear=True, with_pooler=True)
        tr = RescoreBertTrainer(w, BERT_BASE, method="MD_MWER", md_loss_weight=1e-4, lr=1e-5, dropout_seed=1)
        nb = D.synthetic_nbest(3, 50, seed=1)
        rng = np.random.default_rng(0)
        tgt = -np.abs(rng.normal(40, 8, nb.n_hyp)).astype(np.float32)
        cer = (rng.integers(0, 6, nb.n_hyp) / 30.0).astype(np.float32)
        am = nb.am.astype(np.float32)
        return tr, int(nb.hyp_off[-1]), lambda update: tr.step(nb.tokens, nb.hyp_off, nb.utt_off, tgt, am, cer,
                                                               update=update)

    def mlm():
        tr = MLMTrainer(make_weights(BERT_BASE, seed=1234), BERT_BASE, lr=1e-5, dropout_seed=1)
        nb = D.synthetic_nbest(32, 1, seed=1)
        seqs = [nb.tokens[nb.hyp_off[h]:nb.hyp_off[h + 1]].tolist() for h in range(nb.n_hyp)]
        ids, off, lab = do_job_rows(seqs)
        rows = [ids[off[i]:off[i + 1]].tolist() for i in range(32)]
        labs = [lab[off[i]:off[i + 1]].tolist() for i in range(32)]
        batch = pad_rows(rows, labs)
        return tr, int(batch[1][-1]), lambda update: tr.step(*batch, update=update)
    return {"rb": rb, "mlm": mlm}


def child(args):
    """One process: per shape one trainer, every requested variant, interleaved repetitions."""
    import_pkg(args.tree)
    import torch
    res = {"device": torch.cuda.get_device_name(0), "times_ms": {}, "tokens": {}}
    variants = args.variants.split(",")
    for name, make in workloads().items():
        tr, tokens, step = make()
        res["tokens"][name] = tokens

        def run(v):
            if len(variants) > 1:                         # (the parent tree has no freeze: "none" alone)
                tr.unfreeze("bert")
                tr.freeze(*FREEZE.get(v, ()))
            if v == "accap":
                step(False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if v in FREEZE:
                step(True)
            elif v == "micro":
                step(False)
            else:
                tr.accumulate(1.0)
                tr.apply(max_grad_norm=1.0)
            return (time.perf_counter() - t0) * 1e3
        try:
            for v in variants:
                for _ in range(args.warmup):
                    run(v)
            ms = {v: [] for v in variants}
            for _ in range(args.reps):
                for v in variants:
                    ms[v].append(run(v))
            for v in variants:
                res["times_ms"][f"{name}:{v}"] = ms[v]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "train_freeze_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    ap.add_argument("--variants", default=",".join(VARIANTS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {"all": [], "none": [], "parent_none": []}
    for _ in range(args.rounds):
        runs["all"].append(run_child(REPO, ",".join(VARIANTS), args))
        if args.parent_tree:
            runs["parent_none"].append(run_child(args.parent_tree, "none", args))
            runs["none"].append(run_child(REPO, "none", args))
    recs = []
    first = runs["all"][0]
    for name in ("rb", "mlm"):
        s = {v: summary([r["times_ms"][f"{name}:{v}"] for r in runs["all"]]) for v in VARIANTS}
        for v in VARIANTS:
            recs.append({"kind": "step", "shape": name, "variant": v, "frozen": list(FREEZE.get(v, ())),
                         "tokens": first["tokens"][name], "ratio_to_none": s[v]["median_ms"] / s["none"]["median_ms"],
                         **s[v], "device": first["device"]})
        if args.parent_tree:
            here = summary([r["times_ms"][f"{name}:none"] for r in runs["none"]])
            par = summary([r["times_ms"][f"{name}:none"] for r in runs["parent_none"]])
            recs.append({"kind": "none_vs_parent", "shape": name, "this_tree": here, "parent": par,
                         "ratio": here["median_ms"] / par["median_ms"], "device": first["device"]})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in recs:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
