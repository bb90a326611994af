"""Benchmark: MLM_PLL masked-token BERT-base forwards/s on MI355X (BASELINE.json metric).

One step = one full scoring pass of the hot path over the step's synthetic N-best input
(configs[2]: MLM_PLL full PLL, bert-base, N=50, mean L~32, U utterances per rank):
  tokens resident in HBM -> on-device mask expansion -> 12-layer encoder -> fused
  decoder/log-softmax gather -> fp64 PLL per hypothesis -> RCCL all_gather of
  (am, lm) -> rank 0 fusion + argmax over the 101-weight grid (rs_fuse_rerank).
The corpus-CER numerators of the sweep (rs_ref_edit + rs_corpus_edits) depend only on the
argmax and the fixed reference texts; they run once after the timed loop (the `rerank` block),
as rescore.py computes them once per weight.
Every rank scores its own U utterances (weak scaling; utterances are independent).
``--workload c4``: BASELINE config C4 instead — the full 7176-utterance real-length set at N=100
(alfred test length histogram), one fixed set split over the ranks (strong scaling).
The default C3 run with ``--full`` also reports ``c4_secondary``: one pass of that full C4 set on rank 0 at N=1.

Prints ONE JSON line on rank 0.  A plain run sets up (synthetic set, weights, the MLM fine-tune
that produces the scored checkpoint), warms up, times ``--steps`` steps and prints the line.
``--dump-outputs DIR`` also writes what the last timed step returned (``lm.npy``: the float64 PLL
of every hypothesis of the global set in set order; ``argmax.npy``: rank 0's fused argmax
[101 weights, utterances] as float64); the inputs are seeded, so two builds run with the same
arguments can be compared output for output.
``--full`` adds the legs outside the timed region: a HIP-event per-kernel-kind profile pass
(roofline of the dominant kernel), the reranked-CER check against the oracle's fusion, a bounded
CPU baseline (the oracle's PyTorch-CPU restatement of the reference work pattern), the
reduced-precision fp16 leg and the C4 secondary pass.  --cpu-seconds, --no-profile, --fp16-steps
and --c4-secondary shape those legs and have no effect without --full.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
import __graft_entry__  # noqa: E402

__graft_entry__._import_pkg()
from asr_rescoring_amd import data as D  # noqa: E402
from asr_rescoring_amd import rerank  # noqa: E402
from asr_rescoring_amd.weights import BERT_BASE, make_weights  # noqa: E402

PEAK_FP16_TFLOPS = 2500.0   # MI355X dense FP16/BF16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


DTYPE = {"fp16x3": "fp16x3-split (fp32-accurate: hi/lo fp16 operand split on fp16 MFMA, fp32 accumulate)",
         "fp16": "fp16 (reduced precision: fp16 MFMA operands, fp32 accumulate)"}


def _cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def c4_set():
    """BASELINE config C4's input: 7176 utterances x N=100 at the alfred test set's real hypothesis
    lengths (tests/golden/alfred_test_lengths.json, the length histogram of the reference's data)."""
    lc = json.load(open(os.path.join(REPO, "tests", "golden", "alfred_test_lengths.json")))["length_counts"]
    lengths = np.repeat(np.arange(len(lc)), lc).astype(np.int64)
    return D.synthetic_nbest(7176, 100, seed=1, lengths=lengths, hard=True)


def forward_flops(T: int, s=BERT_BASE) -> float:
    """Canonical algorithmic FLOPs of one MLM_PLL masked forward at length T."""
    H, F, V, nl = s.hidden, s.intermediate, s.vocab, s.layers
    dense = 2 * (4 * H * H + 2 * H * F)
    return float((nl - 1) * (T * dense + 4 * T * T * H) + 4 * T * H * H
                 + (2 * H * H + 4 * T * H + 2 * H * H + 4 * H * F) + 2 * (H * H + H * V))


def c4_secondary(scorer, weights0, device, rerank_utts=500, finetune_steps=300):
    """BASELINE config C4 at one GPU.  Throughput: one timed pass of the full set (7176 x N=100, real
    lengths) through the headline scorer (warm from the C3 steps).  Rerank (the CER half of the
    metric): the reference's pipeline on the set's first ``rerank_utts`` utterances — the seed-1234
    BERT MLM-fine-tuned on THOSE utterances' references (MLM_PLL/main.py:117-161; an LM that never saw
    C4's references leaves the pick AM-only, round-5 VERDICT item 8), their PLL scored by a scorer
    with that checkpoint, the 101-weight HIP fusion + corpus CER, and the argmax over all 101 weights
    from the CPU reference's own lm (the oracle's restatement of the reference work pattern with the
    same checkpoint) against the HIP lm on the two utterances nearest the subset's median cost."""
    from asr_rescoring_amd import shard
    from asr_rescoring_amd.scorer import PLLScorer
    from asr_rescoring_amd.train import finetune_mlm_on_texts
    from oracle import rescore_ref as RR
    import oracle.bert_ref as OB
    t_gen = time.perf_counter()
    nb4 = c4_set()
    t_gen = time.perf_counter() - t_gen
    d4 = torch.from_numpy(nb4.tokens).to(torch.device("cuda", device))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scorer.score_nbest(d4, nb4.hyp_off)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lens = np.diff(nb4.hyp_off)
    del d4
    # ---- rerank leg (untimed): fine-tune on the subset's references, score, fuse
    Nb = 100
    sub = nb4.slice_utts(0, min(rerank_utts, nb4.n_utt))
    t_ft = time.perf_counter()
    w_ft, losses = finetune_mlm_on_texts(weights0, sub.refs, BERT_BASE, steps=finetune_steps, lr=1e-4, seed=0,
                                         device=device)
    t_ft = time.perf_counter() - t_ft
    s4 = PLLScorer(w_ft, BERT_BASE, device=device, max_rows=262144, precision="fp16x3")
    lm_np = s4.score_nbest(sub.tokens, sub.hyp_off).double().cpu().numpy()
    s4.close()
    bw, bcer, _arg, cers = rerank.find_best_weight(sub, lm_np, n_best=Nb, device=device)
    model = OB.TorchBert(w_ft, BERT_BASE)
    cost = shard.utterance_costs(sub).astype(np.float64)
    pick = [int(u) for u in np.argsort(np.abs(cost - np.median(cost)), kind="stable")[:2]]
    idx = [sub.utt_off[u] + i for u in pick for i in range(Nb)]
    ref_lm, rel = [], []
    for hh in idx:
        sub_off = sub.hyp_off[hh:hh + 2] - sub.hyp_off[hh]
        _, ref_pll = OB.pll_reference_pattern(model, sub.tokens[sub.hyp_off[hh]:sub.hyp_off[hh + 1]], sub_off,
                                              batch_size=32, full_head=True)
        ref_lm.append(float(ref_pll[0]))
        rel.append(abs(lm_np[hh] - ref_pll[0]) / abs(ref_pll[0]))
    am_s = sub.am[idx].reshape(2, Nb)
    hyps_s = [[sub.hyp_words(sub.utt_off[u] + i) for i in range(Nb)] for u in pick]
    refs_s = [sub.refs[u] for u in pick]
    _, _, arg_ref = RR.find_best_weight(am_s, np.asarray(ref_lm).reshape(2, Nb), hyps_s, refs_s, Nb)
    _, _, arg_hip = RR.find_best_weight(am_s, lm_np[idx].reshape(2, Nb), hyps_s, refs_s, Nb)
    return {"workload": "C4 MLM_PLL full PLL, full 7176-utterance set x N=100, alfred real lengths, 1 GPU",
            "value": round(nb4.n_forwards() / dt, 2), "unit": "masked fwd/s", "seconds": round(dt, 3),
            "forwards": int(nb4.n_forwards()), "hypotheses": int(nb4.n_hyp),
            "mean_T": round(float(np.average(lens, weights=lens - 2)), 2), "dtype": "fp16x3-split (fp32-accurate)",
            "timing": "one pass, scorer warm from the C3 steps; input generation excluded",
            "input_generation_seconds": round(t_gen, 1),
            "rerank": {"utterances": int(sub.n_utt), "best_weight": round(bw, 2), "cer": bcer,
                       "am_only_cer": float(cers[0]),
                       "lm": (f"seed-1234 BERT MLM-fine-tuned {finetune_steps} steps (batch 64, lr 1e-4, "
                              f"{t_ft:.1f} s) on these {sub.n_utt} utterances' OWN references: an oracle-style LM "
                              "that makes the fused argmax depend on the LM (synthetic token sequences carry no "
                              "structure a held-out fine-tune could learn)"),
                       "finetune_loss_first_final": [round(losses[0], 4), round(losses[-1], 4)],
                       "oracle_check_utterances": pick,
                       "argmax_equal_cpu_reference_lm_all_101_weights": bool(np.array_equal(arg_ref, arg_hip)),
                       "pll_max_rel_err_vs_cpu_reference": float(max(rel))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--utts", type=int, default=200, help="utterances per rank per step (C3: 200)")
    ap.add_argument("--nbest", type=int, default=50)
    ap.add_argument("--max-rows", type=int, default=262144, help="token rows per launch chunk (262144: +0.5 %% over 131072)")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs outside the timed region: per-kernel profile / roofline, rerank check "
                         "against the oracle, CPU baseline, fp16 leg, C4 secondary pass (off: steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs as DIR/lm.npy and DIR/argmax.npy")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="--full: CPU-baseline budget (0 = skip)")
    ap.add_argument("--no-profile", action="store_true", help="--full: skip the per-kernel profile pass")
    ap.add_argument("--precision", default="fp16x3", choices=("fp16x3", "fp16"),
                    help="fp16x3 (default): split-fp16 operands, fp32-accurate (the reference computes "
                         "in fp32); fp16: fp16 operands (reduced precision, reported as a secondary field)")
    ap.add_argument("--fp16-steps", type=int, default=2,
                    help="--full: steps of the reduced-precision fp16 leg (0 = skip)")
    ap.add_argument("--force-gather", action="store_true",
                    help="at one rank too: a one-rank nccl (RCCL) group and the all_gather inside every step")
    ap.add_argument("--finetune-steps", type=int, default=300,
                    help="MLM fine-tuning steps on the synthetic set's reference sentences before scoring "
                         "(the reference's mlm_finetune_bert -> scoring -> fusion pipeline; 0 = random-init LM)")
    ap.add_argument("--finetune-lr", type=float, default=1e-4)
    ap.add_argument("--workload", default="c3", choices=("c3", "c4"),
                    help="c3 (default): U utterances x N=50 per rank (weak scaling); c4: the full 7176 x N=100 "
                         "real-length set split over the ranks (strong scaling)")
    ap.add_argument("--c4-secondary", type=int, default=1,
                    help="--full, C3 runs, rank 0 at N=1: one timed pass of the full C4 set (0 = skip)")
    args = ap.parse_args()

    # --gpus N without a launcher: N fresh rank processes (one per GPU) before any GPU call here;
    # the parent only relays rank 0's JSON line (asr_rescoring_amd/launch.py)
    from asr_rescoring_amd import launch
    if launch.need_spawn(args.gpus):
        rc = launch.spawn_ranks(args.gpus, sys.argv[1:], script=os.path.abspath(__file__))
        sys.exit(rc if rc >= 0 else 128 - rc)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and int(os.environ.get("RANK", "0")) == 0:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: running {world} rank(s)", file=sys.stderr)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # one JSON line on stdout from the whole job (the torch.distributed.run form prints every rank's
    # stdout): ranks > 0 write stdout to stderr from here on, native libraries included (gloo's
    # connection messages go to fd 1)
    if world > 1 and rank != 0:
        sys.stdout.flush()
        os.dup2(2, 1)
    # RS_BENCH_DEVICE (rehearsal only): every rank on this one GPU (a multi-rank run on a 1-GPU box,
    # with RS_DIST_BACKEND=gloo for the exchange); unset on a real node: rank r on GPU LOCAL_RANK
    if os.environ.get("RS_BENCH_DEVICE") is not None:
        local = int(os.environ["RS_BENCH_DEVICE"])
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from asr_rescoring_amd import shard
    if world > 1 or args.force_gather:
        sys.stdout.flush()
        fd1 = os.dup(1)
        os.dup2(2, 1)                             # (rank 0 too, while the group forms)
        try:
            shard.init_from_env(local, force=args.force_gather)
        finally:
            sys.stdout.flush()
            os.dup2(fd1, 1)
            os.close(fd1)
    gather = dist.is_initialized()
    xdev = shard.exchange_device(dist.get_backend() if gather else None, dev, dev)

    from asr_rescoring_amd.scorer import PLLScorer
    weights = weights0 = make_weights(BERT_BASE, seed=1234)
    kx = 3 if args.precision == "fp16x3" else 1

    # ONE global synthetic set of utts x world utterances, split by the product's sharding
    # plan (shard.plan_shards on the cost sum_h L_h (L_h + 2)): every rank scores its
    # contiguous utterance range, the (am, lm) blocks meet in one all-gather (RCCL), rank 0
    # runs the 101-weight fusion sweep over the whole set.  The global set grows with the
    # rank count (weak scaling: per-rank work ~ utts utterances).
    # hard: hypotheses permuted and AM scores unsorted, so the fused argmax moves with the weight
    # and the rerank check below is not the trivial AM-only case (same token counts)
    if args.workload == "c4":
        args.nbest = 100
        nb_all = c4_set()
    else:
        nb_all = D.synthetic_nbest(args.utts * world, args.nbest, seed=1, hard=True)

    # The reference's pipeline: fine-tune BertForMaskedLM on in-domain text (MLM_PLL/main.py:117-161),
    # score with that checkpoint (:184-186), fuse (rescore.py:25-45).  Here the in-domain text is the
    # synthetic set's reference sentences, so the LM learns to prefer the correct hypotheses and the
    # fused argmax depends on the LM.  Native trainer, deterministic; outside the timed region.
    ft = None
    if args.finetune_steps > 0:
        from asr_rescoring_amd.train import finetune_mlm_on_texts
        t_ft = time.perf_counter()
        weights, losses = finetune_mlm_on_texts(weights, nb_all.refs, BERT_BASE, steps=args.finetune_steps,
                                                lr=args.finetune_lr, seed=0, device=local)
        torch.cuda.synchronize()
        ft = {"steps": args.finetune_steps, "lr": args.finetune_lr, "batch_rows": 64,
              "first_loss": round(losses[0], 4), "final_loss": round(losses[-1], 4),
              "seconds": round(time.perf_counter() - t_ft, 2),
              "text": ("the evaluation set's OWN reference sentences (do_job rows, dropout off): an oracle-style "
                       "LM that makes the fused argmax depend on the LM; the rerank CER / best weight measure the "
                       "fusion path, not LM quality (synthetic token sequences carry no structure a held-out "
                       "fine-tune could learn)")}
    scorer = PLLScorer(weights, BERT_BASE, device=local, max_rows=args.max_rows, precision=args.precision)
    parts = shard.plan_shards(shard.utterance_costs(nb_all), world)
    u0, u1 = parts[rank]
    nb = nb_all.slice_utts(u0, u1)
    counts = [int(nb_all.utt_off[b] - nb_all.utt_off[a]) for a, b in parts]
    d_tok = torch.from_numpy(nb.tokens).to(dev)                 # resident in HBM
    am_d = torch.from_numpy(nb.am).to(dev)
    n_fwd = nb.n_forwards()
    n_fwd_all = nb_all.n_forwards()
    lens = np.diff(nb.hyp_off)
    # canonical algorithmic FLOPs of the step (the reference's work: every masked forward in full),
    # NET of the layer-0 dedup (rs_api.hip plan_unique_rows: the layer-0 Q/K/V projection runs over a
    # hypothesis' T rows plus one [MASK] row per copy, not over its L x T copy rows; chunks of T <= 64)
    H3 = 2.0 * BERT_BASE.hidden * 3 * BERT_BASE.hidden
    flops_step = float(sum(forward_flops(int(T)) * (int(T) - 2)
                           - (H3 * ((int(T) - 2) * int(T) - int(T) - (int(T) - 2)) if int(T) <= 64 else 0.0)
                           for T in np.diff(nb_all.hyp_off)))
    grid = rerank.weight_grid("norm")
    hyp_len_all = nb_all.hyp_len()

    def step():
        lm = scorer.score_nbest(d_tok, nb.hyp_off)               # float64 [H_local]
        pair = torch.stack([am_d, lm])                           # (am, lm) [2, H_local]
        if gather and xdev.type == "cpu":                         # gloo rehearsal: host exchange
            out = shard.gather_scores(pair.cpu(), counts).to(dev)
        else:
            out = shard.gather_scores(pair, counts) if gather else pair
        arg = None
        if rank == 0:
            arg = rerank.fuse_rerank(out[0], out[1], hyp_len_all, nb_all.utt_off, grid, "norm", args.nbest, local)
        return out[1], arg

    lm = arg_last = None
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if gather:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        lm, arg_last = step()
    torch.cuda.synchronize()
    if gather:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], dtype=torch.float64, device=xdev)
    if gather:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    total_fwd = n_fwd_all * args.steps
    value = total_fwd / dt

    # ---- --dump-outputs: what the last timed step returned, for build-to-build comparison ----
    if args.dump_outputs and rank == 0 and lm is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "lm.npy"), lm.double().cpu().numpy())
        np.save(os.path.join(args.dump_outputs, "argmax.npy"), arg_last.cpu().numpy().astype(np.float64))

    # ---- profile leg: per-kernel-kind HIP-event timing (separate, untimed pass) ----------
    roof = None
    kinds = {}
    if args.full and not args.no_profile:
        scorer.profile(True)
        scorer.score_nbest(d_tok, nb.hyp_off)
        torch.cuda.synchronize()
        kinds = scorer.profile_read()
        scorer.profile(False)
        gemm_kinds = {k: v for k, v in kinds.items() if v[2] > 0}
        dom = max(gemm_kinds, key=lambda k: gemm_kinds[k][0])
        ms, n, fl = gemm_kinds[dom]
        # fl = MFMA work (2*M*N*K over the kx-wide operand images); algorithmic = fl / kx
        achieved_work = fl / (ms * 1e-3) / 1e12
        achieved_alg = achieved_work / kx
        # HBM(+MALL) bytes per launch from the committed rocprofv3 PMC summary (FETCH_SIZE x2
        # gfx950 correction + WRITE_SIZE, per row), scaled to this run's rows per launch
        traffic, tsrc = None, None
        nk = {"qkv": (2304, 768, "qkv"), "oproj": (768, 768, "oproj"), "ffn1": (3072, 768, "ffn1"),
              "ffn2": (768, 3072, "ffn2")}.get(dom)
        suffix = f"_pmc_gemm_traffic_{args.precision}.json"
        pmc_files = sorted(f for f in os.listdir(os.path.join(REPO, "profiles")) if f.endswith(suffix))
        rows_per_launch = fl / kx / max(n, 1) / (2.0 * nk[0] * nk[1]) if nk else None
        if nk and pmc_files:
            pm = json.load(open(os.path.join(REPO, "profiles", pmc_files[-1])))
            e = pm.get(nk[2], {})
            if e.get("fetch_size_bytes_per_row") and e.get("write_size_bytes_per_row"):
                traffic = (e["fetch_size_bytes_per_row"] + e["write_size_bytes_per_row"]) * rows_per_launch
                tsrc = f"profiles/{pmc_files[-1]}"
        alg_bytes = None
        if nk:
            # operand images in, output out.  fp16: [hi] operands, fp16 out.  fp16x3 (split-operand
            # GEMMs, RS_X3S default): two-part [hi | lo*64] A and W read, fp32 out (QKV / O-proj /
            # FFN2) or the two-part GELU image (FFN1); RS_X3S=0: three-part images, K x 3
            x3s = kx == 3 and os.environ.get("RS_X3S", "1") != "0"
            parts = 2 if x3s else kx
            out_b = (4 if dom != "ffn1" else 2 * parts) if kx == 3 else 2
            if x3s and dom in ("oproj", "ffn2") and os.environ.get("RS_LNFUSE", "1") != "0":
                out_b = 8      # residual + LayerNorm epilogue: the two-part residual image in, its update out
            alg_bytes = rows_per_launch * (parts * nk[1] * 2 + nk[0] * out_b) + parts * nk[0] * nk[1] * 2
        # the roofline figure is ALGORITHMIC: the reference's 2*M*N*K of the projection per launch
        #  / its HIP-event launch time, vs the dense fp16 MFMA peak; the MFMA work
        # the fp16x3 form actually issues (3 fp16 products per algorithmic one) is secondary
        roof = {"kernel": f"gemm_{args.precision}_{dom}", "bound": "mfma", "achieved": round(achieved_alg, 2),
                "peak": PEAK_FP16_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved_alg / PEAK_FP16_TFLOPS, 4),
                "achieved_basis": ("algorithmic: 2*M*N*K of the projection over its valid rows per launch / "
                                   "HIP-event launch time, vs the dense fp16 MFMA peak"),
                "achieved_mfma_work": round(achieved_work, 2),
                "frac_mfma_work": round(achieved_work / PEAK_FP16_TFLOPS, 4),
                "mfma_work_basis": (f"{kx} fp16 MFMA products per algorithmic product (fp16x3: hi.hi + hi.lo + "
                                    "lo.hi), the work the kernel issues"),
                "traffic": traffic, "traffic_source": tsrc, "algorithmic_bytes": alg_bytes,
                "launches": n, "avg_launch_ms": round(ms / max(n, 1), 4),
                "flops_per_launch": fl / max(n, 1), "algorithmic_flops_per_launch": fl / kx / max(n, 1)}
        # MFMA busy of the same kernel kind from a COMMITTED rocprofv3 PMC pass of an earlier run
        # (SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE over the CUs, tools/pmc_mfma.py): not this run's
        # measurement, so it sits under its own key with its source file
        mfma_files = sorted(f for f in os.listdir(os.path.join(REPO, "profiles")) if f.endswith("_pmc_mfma.json"))
        tag = {"qkv": "x3s:qkv", "oproj": "x3s:oproj", "ffn1": "x3s:ffn1", "ffn2": "x3s:ffn2"}.get(dom)
        if tag and kx == 3 and mfma_files:
            pm = json.load(open(os.path.join(REPO, "profiles", mfma_files[-1])))
            hit = [v for k, v in pm.items() if k.startswith(tag)]
            if hit:
                roof["committed_pmc"] = {"mfma_busy": hit[0].get("mfma_busy"), "clock_GHz": hit[0].get("clock_GHz"),
                                         "source": f"profiles/{mfma_files[-1]}",
                                         "note": "committed profile of an earlier build; not measured in this run"}
        if traffic is not None:
            roof["traffic_note"] = "from a committed PMC profile (traffic_source), scaled to this run's rows per launch"

    # ---- reranked 1-best CER (second half of BASELINE.json's metric), rank-0 shard -------
    # HIP fusion over the 101-weight grid + corpus CER on this step's LM scores, checked
    # against the oracle's numpy restatement of rescore.py:25-58 on the same scores.
    rr = None
    if args.full and rank == 0:
        from oracle import rescore_ref as RR
        lm_np = lm.double().cpu().numpy()
        bw, bcer, arg, cers = rerank.find_best_weight(nb_all, lm_np, n_best=args.nbest, device=local)
        U, Nb = nb_all.n_utt, args.nbest
        hyps = [[nb_all.hyp_words(nb_all.utt_off[u] + i) for i in range(Nb)] for u in range(U)]
        obw, obcer, oarg = RR.find_best_weight(nb_all.am.reshape(U, Nb), lm_np.reshape(U, Nb), hyps,
                                               nb_all.refs, n_best=Nb)
        # HIP fusion/CER kernels vs the oracle's numpy fusion on the SAME (HIP) lm: a check of
        # the fusion path; the scoring itself is checked against the CPU reference pattern in
        # cpu_baseline.pll_max_rel_err_vs_gpu and by tests/test_gpu_configs.py
        rr = {"best_weight": round(bw, 2), "cer": bcer, "am_only_cer": float(cers[0]),
              "lm": ("fine-tuned on the evaluation references (lm_finetune.text)" if ft else "random-init"),
              "utterances": U, "fusion_cer_equal_oracle_same_lm": bool(bcer == obcer and bw == obw),
              "fusion_argmax_equal_oracle_same_lm": bool(np.array_equal(np.asarray(arg), oarg))}

    # ---- CPU baseline: oracle restatement of the reference work pattern ------------------
    # Also a scoring-parity spot check at bench scale: the PLL of every sampled hypothesis
    # (reference work pattern, fp32 CPU) against the HIP lm of the timed steps.
    cpu, cpu_model = None, None
    if args.full and rank == 0 and world == 1 and args.cpu_seconds > 0:    # the contract: rank 0 at N = 1 only
        from oracle.bert_ref import TorchBert, set_cpu_threads
        import oracle.bert_ref as OB
        threads = set_cpu_threads()
        model = TorchBert(weights, BERT_BASE)
        cpu_model = model
        lm_np = lm.double().cpu().numpy()
        # whole utterances nearest the step's median utterance cost (sum_h L_h (L_h + 2), the cost
        # the sharding plan balances) first, until the time budget: a sample at the step's length
        # distribution (its mean T is reported next to config.mean_T), covering several
        # utterances for the rerank check below
        Nb = args.nbest
        T_h = np.diff(nb.hyp_off)
        cost_u = shard.utterance_costs(nb).astype(np.float64)
        rows_done, t_cpu, rel, done_u, ref_lm = 0, 0.0, [], [], {}
        for u in np.argsort(np.abs(cost_u - np.median(cost_u)), kind="stable"):
            if t_cpu >= args.cpu_seconds:
                break
            for hh in range(nb.utt_off[u], nb.utt_off[u + 1]):
                sub_off = nb.hyp_off[hh:hh + 2] - nb.hyp_off[hh]
                toks = nb.tokens[nb.hyp_off[hh]:nb.hyp_off[hh + 1]]
                t1 = time.perf_counter()
                _, ref_pll = OB.pll_reference_pattern(model, toks, sub_off, batch_size=32, full_head=True)
                t_cpu += time.perf_counter() - t1
                rel.append(abs(lm_np[hh] - ref_pll[0]) / abs(ref_pll[0]))
                ref_lm[hh] = float(ref_pll[0])
                rows_done += int(sub_off[-1]) - 2
            done_u.append(int(u))
        h = len(ref_lm)
        # the rerank index from the CPU reference's own lm on the sampled utterances, against
        # the HIP lm's (all 101 weights): a check of scoring + fusion
        from oracle import rescore_ref as RR
        uw = len(done_u)
        rerank_same = None
        if uw > 0 and all(nb.utt_off[u + 1] - nb.utt_off[u] == Nb for u in done_u):
            idx = [nb.utt_off[u] + i for u in done_u for i in range(Nb)]
            am_s = nb.am[idx].reshape(uw, Nb)
            hyps_s = [[nb.hyp_words(nb.utt_off[u] + i) for i in range(Nb)] for u in done_u]
            refs_s = [nb.refs[u] for u in done_u]
            _, _, arg_ref = RR.find_best_weight(am_s, np.asarray([ref_lm[i] for i in idx]).reshape(uw, Nb), hyps_s, refs_s, Nb)
            _, _, arg_hip = RR.find_best_weight(am_s, lm_np[idx].reshape(uw, Nb), hyps_s, refs_s, Nb)
            rerank_same = bool(np.array_equal(arg_ref, arg_hip))
        hs = np.asarray(sorted(ref_lm), np.int64)
        Ls = T_h[hs] - 2
        mean_T_sample = float(np.average(T_h[hs], weights=Ls)) if len(hs) else None
        cpu = {"value": round(rows_done / t_cpu, 2), "unit": "masked fwd/s", "cores": threads,
               "cpu_model": _cpu_model(), "kind": "port",
               "sample": f"{uw} whole utterances, {h} hypotheses ({rows_done} masked forwards, mean T "
               f"{mean_T_sample:.2f} per forward; the utterances nearest the median utterance cost of the "
               f"rank-0 step input), reference work pattern (batch 32 padded rows, all-position logits + CE, "
               f"fp64 accumulation), torch {torch.__version__} CPU",
               "sample_mean_T": round(mean_T_sample, 2) if mean_T_sample else None,
               "seconds": round(t_cpu, 2),
               "pll_max_rel_err_vs_gpu": float(max(rel)) if rel else None,
               "rerank_argmax_equal_cpu_reference_lm": rerank_same, "rerank_check_utterances": uw}

    # ---- secondary leg: the reduced-precision fp16 mode on the same input (labelled) ------
    fp16 = None
    if args.full and rank == 0 and world == 1 and args.precision != "fp16" and args.fp16_steps > 0:
        s16 = PLLScorer(weights, BERT_BASE, device=local, max_rows=args.max_rows, precision="fp16")
        lm16 = s16.score_nbest(d_tok, nb.hyp_off)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.fp16_steps):
            lm16 = s16.score_nbest(d_tok, nb.hyp_off)
        torch.cuda.synchronize()
        dt16 = time.perf_counter() - t1
        lm_loc = lm[:nb.n_hyp]                                   # rank 0's shard leads the global order
        rel16 = ((lm16 - lm_loc).abs() / lm_loc.abs()).max().item()
        fp16 = {"value": round(n_fwd * args.fp16_steps / dt16, 2), "unit": "masked fwd/s",
                "dtype": "fp16 operands / fp32 accumulate (reduced precision; not the headline)",
                "steps": args.fp16_steps, "pll_max_rel_vs_headline": rel16}
        s16.close()

    # ---- secondary leg: BASELINE config C4 (full 7176 x N=100 real-length set) at one GPU ------
    c4 = None
    if (args.full and rank == 0 and world == 1 and args.workload == "c3" and args.c4_secondary
            and args.precision == "fp16x3"):
        c4 = c4_secondary(scorer, weights0, local)

    if rank == 0:
        mean_T = float(np.average(lens, weights=lens - 2))
        rec = {"metric": "masked-token BERT forwards/sec (MLM_PLL, N=50, L~32)", "value": round(value, 2),
               "unit": "masked fwd/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "full": bool(args.full),
               "scaling": "strong" if args.workload == "c4" else "weak",
               "vs_baseline": None, "dtype": DTYPE[args.precision],
               "data": ("synthetic (PCG64 seed 1, permuted N-best with unsorted AM scores"
                        + ("; alfred test length histogram" if args.workload == "c4" else "")
                        + "); bert-base weights: random init seed 1234"
                        + (f", then MLM-fine-tuned {args.finetune_steps} steps on the set's reference sentences"
                           if ft else "")),
               "config": {"workload": ("C4 MLM_PLL full PLL, full 7176-utterance set, N=100, real lengths"
                                       if args.workload == "c4" else "C3 MLM_PLL full PLL"),
                          "model": "bert-base-chinese shape (12L/768/12H/3072/V21128)",
                          "utts_per_rank": (None if args.workload == "c4" else args.utts), "n_best": args.nbest,
                          "utts_total": nb_all.n_utt,
                          "forwards_per_step": n_fwd_all, "forwards_rank0_step": n_fwd,
                          "mean_T": round(mean_T, 2),
                          "parallelism": f"dp{world} (cost-balanced utterance shards of one global set + one "
                                         + ("gloo (host) " if gather and xdev.type == "cpu" else "RCCL ") + "all_gather"
                                         + (" in every step" if gather else "; none at one rank") + ")"},
               "achieved_tflops_canonical": round(flops_step * args.steps / dt / 1e12, 2),
               "achieved_tflops_basis": ("canonical algorithmic FLOPs of every masked forward (SURVEY 8d) net of "
                                         "the layer-0 Q/K/V rows the exact dedup skips, per second"),
               "roofline": roof, "cpu_baseline": cpu, "rerank": rr, "lm_finetune": ft, "fp16_secondary": fp16,
               "c4_secondary": c4,
               "kinds_ms": {k: round(v[0], 3) for k, v in kinds.items()}}
        print(json.dumps(rec))
    scorer.close()
    del lm
    if gather:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
