"""Trainer attention, forward + backward (k_train.hip through rs_debug_train_attn): form 0 (the
whole-head kernels, T <= 128) and form 1 (the tiled kernels) at the bert-base head shape
(heads 12, H 768), 32 sequences of one length; and one full MLM training step (32 rows of 128
tokens, bert-base shape, seeded random weights) under RS_TRAIN_ATTN=legacy and =tiled.

Each figure is HIP-event time of single calls: 5 warm-up calls, then REPS calls per round in ROUNDS
rounds with the forms / trainers alternating inside a round; reported are the median, the 10th and
90th percentile and the minimum over all timed calls.  The attention entry's time includes its
metadata copies (one small device-to-host and one host-to-device copy and a stream synchronise per
call), the same for both forms.  Writes one JSON line per case; usage:
    python tools/train_attn_bench.py [--out FILE] [--no-step]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

__graft_entry__._import_pkg()
from asr_rescoring_amd import _lib  # noqa: E402

HEADS, H, S = 12, 768, 32
REPS, ROUNDS = 10, 3


def _stats(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), p10_ms=float(a[int(0.1 * (len(a) - 1))]),
                p90_ms=float(a[int(round(0.9 * (len(a) - 1)))]), min_ms=float(a[0]), n=len(a))


def _time_call(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _alternate(fns):
    """fns: name -> callable.  Warm up each, then ROUNDS x (REPS calls of each, alternating)."""
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for _ in range(REPS):
            for k, f in fns.items():
                ms[k].append(_time_call(f))
    return {k: _stats(v) for k, v in ms.items()}


def attention_cases(out):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    for T, forms in [(34, (0, 1)), (128, (0, 1)), (256, (1,)), (512, (1,))]:
        g = torch.Generator(device=dev).manual_seed(T)
        M = S * T
        qkv = torch.randn(M, 3 * H, device=dev, generator=g)
        dctx = torch.randn(M, H, device=dev, generator=g)
        off = torch.arange(0, M + 1, T, dtype=torch.int32, device=dev)
        ctx = torch.empty(M, H, device=dev)
        dqkv = torch.empty(M, 3 * H, device=dev)

        def call(form):
            rc = lib.rs_debug_train_attn(form, qkv.data_ptr(), off.data_ptr(), None, S, H, HEADS, dctx.data_ptr(),
                                         0, 0, 0, 0.0, ctx.data_ptr(), dqkv.data_ptr(), st)
            assert rc == 0, lib.rs_last_error()

        res = _alternate({form: (lambda form=form: call(form)) for form in forms})
        flop = 5 * 2.0 * S * HEADS * T * T * 64          # the five products of forward + backward
        for form, r in res.items():
            rec = dict(case="attention fwd+bwd", form=form, T=T, S=S, heads=HEADS, H=H,
                       tflops_of_5_products=flop / (r["median_ms"] * 1e-3) / 1e12, **r)
            out.append(rec)
            print(json.dumps(rec), flush=True)


def mlm_step_case(out):
    from asr_rescoring_amd.train import MLMTrainer
    from asr_rescoring_amd.weights import BERT_BASE, make_weights
    w = make_weights(BERT_BASE, seed=1)
    rng = np.random.default_rng(1)
    T = 128
    ids = rng.integers(1, BERT_BASE.vocab, S * T).astype(np.int32)
    lab = rng.integers(1, BERT_BASE.vocab, S * T).astype(np.int32)
    off = np.arange(0, S * T + 1, T, dtype=np.int32)
    trs = {}
    old = os.environ.get("RS_TRAIN_ATTN")
    try:
        for mode in ("legacy", "tiled"):
            os.environ["RS_TRAIN_ATTN"] = mode
            trs[mode] = MLMTrainer(w, BERT_BASE, lr=1e-5, hidden_dropout=0.1, attn_dropout=0.1, dropout_seed=1)
    finally:
        if old is None:
            os.environ.pop("RS_TRAIN_ATTN", None)
        else:
            os.environ["RS_TRAIN_ATTN"] = old
    try:
        res = _alternate({m: (lambda t=t: t.step(ids, off, lab)) for m, t in trs.items()})
    finally:
        for t in trs.values():
            t.close()
    for mode, r in res.items():
        rec = dict(case="MLM training step (host call, incl. uploads)", RS_TRAIN_ATTN=mode, T=T, rows=S,
                   shape="bert-base", **r)
        out.append(rec)
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_attn_bench needs a HIP GPU")
    out = []
    attention_cases(out)
    if not a.no_step:
        mlm_step_case(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in out:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
