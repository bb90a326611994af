"""Scores of two library builds compared BITWISE on the same inputs (one process per build:
RS_LIBRESCORE selects the library).  Usage:
    bitwise_ab.py LIB_A LIB_B OUTDIR [PRECISION]   (parent: runs both, compares, prints one JSON line;
                                          LIB@VAR=VALUE,...: that library under env switches;
                                          PRECISION: fp16x3 (default) or fp16)
Inputs: the fp16x3 golden tokens (F1), 40 C3 utterances x N=50, 150 C4 utterances x N=100 at the
alfred real lengths; bert-base random init seed 1234, default kernels.  The C3 call runs under the
library's profiler: its launch count and flops per kind are compared for equality like the scores.
Then the ``api_*`` entries (``run_api``): every entry point of scorers and trainers on BERT_TINY."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def run_one(out, precision="fp16x3"):
    import torch
    import __graft_entry__
    __graft_entry__._import_pkg()
    from asr_rescoring_amd import data as D
    from asr_rescoring_amd.scorer import PLLScorer
    from asr_rescoring_amd.weights import BERT_BASE, make_weights
    w = make_weights(BERT_BASE, seed=1234)
    s = PLLScorer(w, BERT_BASE, device=0, max_rows=262144, precision=precision)
    res = {}
    g = np.load(os.path.join(REPO, "tests", "golden", "pll_base.npz"))
    pll, rows = s.score_nbest(g["tokens"], g["hyp_off"], return_rows=True)
    res["f1_pll"], res["f1_rows"] = pll.cpu().numpy(), rows.cpu().numpy()
    nb = D.synthetic_nbest(40, 50, seed=1, hard=True)
    s.profile(True)
    res["c3_pll"] = s.score_nbest(nb.tokens, nb.hyp_off).cpu().numpy()
    prof = s.profile_read()              # kind -> (ms, launches, flops)
    s.profile(False)
    res["c3_launches"] = np.array([prof[k][1] for k in sorted(prof)], np.int64)
    res["c3_flops"] = np.array([prof[k][2] for k in sorted(prof)], np.float64)
    lc = json.load(open(os.path.join(REPO, "tests", "golden", "alfred_test_lengths.json")))["length_counts"]
    lengths = np.repeat(np.arange(len(lc)), lc).astype(np.int64)
    nb4 = D.synthetic_nbest(150, 100, seed=1, lengths=lengths, hard=True)
    res["c4_pll"] = s.score_nbest(nb4.tokens, nb4.hyp_off).cpu().numpy()
    torch.cuda.synchronize()
    s.close()
    run_api(res, precision)
    np.savez(out, **res)


API_LENS = [3, 5, 17, 64, 65, 130]     # both attention kernel families; several chunks at max_rows 512


def run_api(res, precision):
    """The ``api_*`` entries: every scoring entry point, the embeddings, the BERTScore recall and one
    gradient step of both trainers on BERT_TINY (``max_rows`` 512, hypotheses of API_LENS tokens), each
    without (``_plain``) and with (``_typed``) segment ids; and the launch counts of a profiled
    ``score_nbest``."""
    import torch
    from asr_rescoring_amd import data as D
    from asr_rescoring_amd.bertscore import BertScorer
    from asr_rescoring_amd.scorer import PLLScorer, RescoreBertScorer
    from asr_rescoring_amd.train import MLMTrainer, RescoreBertTrainer
    from asr_rescoring_amd.weights import BERT_TINY, make_weights
    sh = BERT_TINY
    w = make_weights(sh, seed=7, with_cls_linear=True, with_pooler=True)
    rng = np.random.default_rng(41)
    hyps = [[D.CLS_ID] + rng.integers(D.FIRST_WORD_ID, sh.vocab, size=T - 2).tolist() + [D.SEP_ID] for T in API_LENS]
    tok = np.concatenate([np.asarray(h, np.int32) for h in hyps])
    off = np.concatenate([[0], np.cumsum(API_LENS)]).astype(np.int32)
    ws = (rng.random(len(tok)) < 0.5).astype(np.uint8)
    sf = np.array([1, 2, 5, 30, 1, 100], np.int32)
    utt = np.array([0, 3, 6], np.int32)
    # a shuffled span plan: the whole-word rows of every hypothesis in a seeded order
    roff, lo, hi, q = D.pll_spans(off, ws, "whole_word")
    perm = np.concatenate([roff[h] + rng.permutation(roff[h + 1] - roff[h]) for h in range(len(API_LENS))])
    lo, hi, q = lo[perm], hi[perm], q[perm]
    # the hypotheses as a padded batch, one [MASK] per row
    mp = [1, 3, 9, 62, 33, 128]
    lab = torch.zeros(len(hyps), max(API_LENS), dtype=torch.int64)
    for i, h in enumerate(hyps):
        lab[i, :len(h)] = torch.tensor(h)
    att = (torch.arange(max(API_LENS))[None, :] < torch.tensor(API_LENS)[:, None]).long()
    ids = lab.clone()
    ids[torch.arange(len(hyps)), torch.tensor(mp)] = sh.mask_id
    types = rng.integers(0, sh.type_vocab, len(tok)).astype(np.int32)
    types_pad = torch.zeros_like(ids)
    types_pad[att.bool()] = torch.from_numpy(types).long()

    def put(name, out):
        for i, t in enumerate(out if isinstance(out, tuple) else (out,)):
            res[f"api_{name}_{i}"] = np.atleast_1d(t.cpu().numpy() if isinstance(t, torch.Tensor) else t)

    pll = PLLScorer(w, sh, device=0, max_rows=512, precision=precision)
    cls = RescoreBertScorer(w, sh, device=0, max_rows=512, precision=precision)
    bs = BertScorer(w, sh, device=0, max_rows=512, precision=precision)
    for tag, tt, ttp in (("plain", None, None), ("typed", types, types_pad)):
        for v in D.PLL_VARIANTS:
            put(f"score_{v}_{tag}", pll.score_nbest(tok, off, return_rows=True, variant=v, word_start=ws, token_types=tt))
        put(f"score_from_{tag}", pll.score_nbest(tok, off, return_rows=True, token_types=tt, score_from=sf))
        put(f"spans_{tag}", pll.score_spans(tok, off, roff, lo, hi, q, return_rows=True, token_types=tt))
        put(f"topk_{tag}", pll.topk_nbest(tok, off, k=3, return_pll=True, token_types=tt))
        put(f"masked_logprob_{tag}", pll.masked_logprob(ids, att, lab, mp, token_type_ids=ttp))
        put(f"masked_topk_{tag}", pll.masked_topk(ids, att, mp, k=3, token_type_ids=ttp))
        put(f"cls_{tag}", cls.score_nbest(tok, off, token_types=tt))
        put(f"embed_{tag}", bs.embed(tok, off, token_types=tt))
        keep = bs._set_types(tt)      # noqa: F841  (recall_matrices takes the pending segment ids)
        put(f"recall_{tag}", bs.recall_matrices(tok, off, utt)[:2])
        rb = RescoreBertTrainer(w, sh, device=0, method="MD_MWER", hidden_dropout=0.0, attn_dropout=0.0)
        loss, sc = rb.step(tok, off, utt, rng.standard_normal(len(hyps)), rng.standard_normal(len(hyps)),
                           rng.random(len(hyps)), update=False, token_types=tt)
        put(f"train_cls_{tag}", (np.float64(loss), sc) + tuple(rb.grad(k) for k in sorted(rb.shapes)))
        rb.close()
        ml = MLMTrainer(w, sh, device=0, hidden_dropout=0.0, attn_dropout=0.0)
        loss = ml.step(ids[att.bool()].numpy(), off, lab[att.bool()].numpy(), update=False, token_types=tt)
        put(f"train_mlm_{tag}", (np.float64(loss),) + tuple(ml.grad(k) for k in sorted(ml.shapes)))
        ml.close()
    pll.profile(True)
    pll.score_nbest(tok, off)
    prof = pll.profile_read()
    res["api_launches"] = np.array([prof[k][1] for k in sorted(prof)], np.int64)
    for s in (pll, cls, bs):
        s.close()


if __name__ == "__main__":
    if sys.argv[1] == "--one":
        run_one(*sys.argv[2:4])
        sys.exit(0)
    la, lb, od = sys.argv[1:4]
    prec = sys.argv[4:5]
    os.makedirs(od, exist_ok=True)
    outs = []
    for tag, spec in (("a", la), ("b", lb)):
        # LIB or LIB@VAR=VALUE,...: the same library under other environment switches
        lib, _, envs = spec.partition("@")
        o = os.path.join(od, f"scores_{tag}.npz")
        env = dict(os.environ, RS_LIBRESCORE=os.path.abspath(lib))
        env.update(dict(kv.split("=", 1) for kv in envs.split(",") if kv))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--one", o] + prec, env=env, check=True, timeout=600)
        outs.append(np.load(o))
    rec = {"lib_a": la, "lib_b": lb, "precision": (prec or ["fp16x3"])[0]}
    for k in outs[0].files:
        a, b = outs[0][k], outs[1][k]
        rec[k] = {"n": int(a.size), "bitwise_equal": bool(np.array_equal(a.view(np.uint8), b.view(np.uint8))),
                  "max_rel_diff": float(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-30)))}
    print(json.dumps(rec))
