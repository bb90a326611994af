"""Top-k token candidates at masked positions (rs_masked_topk / rs_pll_topk; include/rescore.h).

1. The kernels through rs_debug_decoder_topk — launch_mlm_decoder_topk, the function head_mlm runs for
   a top-k call: EPI_LSE_TOPK on the 256 x 256 / 256 x 128 tile, topk_merge, lse_finalize — against the
   float64 reference and the three checkers of tests/topk_ref.py (values, completeness, exact ids
   where float64 decides the order).
2./3. The product (PLLScorer.topk_nbest / masked_topk) against rs_pll_score bitwise and against the
   fp32 oracle (oracle.bert_ref.TorchBert), tiny BERT in both precisions and BERT-base.
4. Errors.  5. The CLI command mlm_topk.
"""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from asr_rescoring_amd import _lib
from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_BASE, BERT_TINY, make_weights
import tail_ref as R
import topk_ref as T

pytestmark = pytest.mark.gpu

REL = 1e-3                                                                   # the project's tolerance on log-probs
ROWS = [(256, 1), (256, 37), (256, 256), (512, 300)]                        # (M_pad, m_valid)
SENT32 = 0x7FC12345                                                          # NaN sentinel (bit pattern)
# (V, K): (130, 256) vpad 256, slabs of 64 / 64 / 2 / 0 valid columns; (1000, 256) vpad 1024: 256 x 256
# tile; (1100, 256) vpad 1152: 256 x 128 tile; (21128, 2304): the product's decoder (fp16x3 image)
SHAPES = [(130, 256), (1000, 256), (1100, 256), (21128, 3 * 768)]
KS = (1, 5, 16)
CASES = [(f, V, K) + r + (k,) for V, K in SHAPES for f in T.FAMILIES for r in ROWS for k in KS]
_dec = {}


def _case_id(c):
    return f"{c[0]}-V{c[1]}-K{c[2]}-M{c[3]}-v{c[4]}-k{c[5]}"


def _decoder_case(family, V, K):
    """Operands for 512 rows and their float64 reference, once per (family, V, K); the weight once
    per (V, K).  Never modified."""
    wkey, key = ("W", V, K), (family, V, K)
    if wkey not in _dec:
        _dec.clear()
        _dec[wkey] = R.decoder_weight(V, K, seed=V + K, device="cuda")
    W = _dec[wkey]
    if key not in _dec:
        for old in [q for q in _dec if q[0] != "W"]:
            del _dec[old]
        A, b, lab = T.operands(family, 512, V, K, W, seed=V + K + len(family), device="cuda")
        _dec[key] = (A, b, lab, T.Ref(A, W, b, V))
    return (W,) + _dec[key]


def _sentinel(shape, dtype=torch.float32):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch_topk(A, W, b, lab, M_pad, m_valid, V, k):
    """One rs_debug_decoder_topk launch on sentinel-filled buffers of M_pad rows."""
    vpad, K = W.shape
    A = A[:M_pad].contiguous()
    part = _sentinel((M_pad, vpad // 64, 2))
    llog = _sentinel((M_pad,))
    out = _sentinel((M_pad,))
    cand = _sentinel((M_pad, vpad // 64, k, 2))
    top_id = _sentinel((M_pad, k), torch.int32)
    top_lp = _sentinel((M_pad, k))
    labw = torch.full((m_valid,), -12345, dtype=torch.int32, device="cuda")
    lab = lab[:m_valid].contiguous()
    rc = _lib.load().rs_debug_decoder_topk(A.data_ptr(), W.data_ptr(), b.data_ptr(), lab.data_ptr(), M_pad, m_valid, vpad,
                                           V, K, labw.data_ptr(), part.data_ptr(), llog.data_ptr(), out.data_ptr(), k,
                                           cand.data_ptr(), top_id.data_ptr(), top_lp.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {"out": out, "part": part, "llog": llog, "cand": cand, "top_id": top_id, "top_lp": top_lp}


def _launch_decoder(A, W, b, lab, M_pad, m_valid, V):
    """rs_debug_decoder (the label form) -> out [m_valid]."""
    vpad, K = W.shape
    A = A[:M_pad].contiguous()
    part = _sentinel((M_pad, vpad // 64, 2))
    llog = _sentinel((M_pad,))
    out = _sentinel((m_valid,))
    labw = torch.empty((m_valid,), dtype=torch.int32, device="cuda")
    lab = lab[:m_valid].contiguous()
    rc = _lib.load().rs_debug_decoder(A.data_ptr(), W.data_ptr(), b.data_ptr(), lab.data_ptr(), M_pad, m_valid, vpad, V,
                                      K, labw.data_ptr(), part.data_ptr(), llog.data_ptr(), out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, part


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_decoder_topk_vs_float64(case):
    family, V, K, M_pad, m_valid, k = case
    W, A, b, lab, ref = _decoder_case(family, V, K)
    got = _launch_topk(A, W, b, lab, M_pad, m_valid, V, k)
    ids, lp = got["top_id"][:m_valid], got["top_lp"][:m_valid]
    for name in ("top_id", "top_lp", "cand", "part", "llog", "out"):
        assert (_bits(got[name][m_valid:]) == SENT32).all(), f"{name}: rows >= m_valid written"
    worst = T.check_values(ids, lp, ref)
    T.check_complete(ids, ref)
    share = T.check_exact(ids, ref)
    print(f"TOPK {_case_id(case)} tile 256x{R.decoder_tile(W.shape[0])}: lp err/bound {worst:.3f} clear {share:.3f}")
    if family == "ties":
        assert ids.tolist() == [T.ties_expected(V, k)] * m_valid
    again = _launch_topk(A, W, b, lab, M_pad, m_valid, V, k)
    for name in ("top_id", "top_lp", "cand", "part", "out"):
        assert torch.equal(_bits(got[name][:m_valid]), _bits(again[name][:m_valid])), f"run-to-run: {name}"
    if m_valid < M_pad:
        A2 = A[:M_pad].clone()
        A2[m_valid:] = float("nan")
        nan_pad = _launch_topk(A2, W, b, lab, M_pad, m_valid, V, k)
        for name in ("top_id", "top_lp"):
            assert torch.equal(_bits(got[name][:m_valid]), _bits(nan_pad[name][:m_valid])), \
                f"{name}: valid rows depend on the pad rows of A"
    # the log-prob of the best id is the label form's log-prob of that id, bit for bit (and the
    # slab pairs and the label log-prob of the top-k form are the label form's)
    out0, part0 = _launch_decoder(A, W, b, ids[:, 0].contiguous(), M_pad, m_valid, V)
    assert torch.equal(_bits(lp[:, 0]), _bits(out0)), "top_lp[:, 0] != rs_debug_decoder(label = top_id[:, 0])"
    assert torch.equal(_bits(got["part"][:m_valid]), _bits(part0[:m_valid]))
    own = _launch_decoder(A, W, b, lab, M_pad, m_valid, V)[0]
    assert torch.equal(_bits(got["out"][:m_valid]), _bits(own)), "the label log-prob of the top-k form differs"


# ---- the product -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def w_tiny():
    return make_weights(BERT_TINY, seed=7, with_cls_linear=True, with_pooler=True)


@pytest.fixture(scope="module")
def w_base():
    return make_weights(BERT_BASE, seed=1234, with_cls_linear=False, with_pooler=False)   # cli._weights' call


@pytest.fixture(scope="module")
def pll_base(w_base):
    from asr_rescoring_amd.scorer import PLLScorer
    s = PLLScorer(w_base, BERT_BASE, device=0, max_rows=4096, precision="fp16x3")
    yield s
    s.close()


def _oracle_logprobs(w, shape, tokens, hyp_off):
    """float64 log_softmax of the oracle's fp32 logits at every masked row: [R, vocab] (CPU)."""
    from oracle.bert_ref import TorchBert, _pad, pll_rows, set_cpu_threads
    set_cpu_threads()
    model = TorchBert(w, shape)
    rows = list(pll_rows(tokens, hyp_off, shape.mask_id))
    out = []
    with torch.no_grad():
        for b0 in range(0, len(rows), 32):
            chunk = rows[b0:b0 + 32]
            ids = _pad([r[1] for r in chunk])
            am = _pad([[1] * len(r[1]) for r in chunk])
            hid = model.encoder(ids, am)
            logits = model.mlm_logits(hid[list(range(len(chunk))), [r[2] for r in chunk], :])
            out.append(logits.double().log_softmax(dim=-1))
    return torch.cat(out)


def _check_vs_oracle(ids, lp, lp64, what):
    """check_values / check_complete / check_exact with the project's REL on log-probs: a log-prob within
    REL |reference|; the margin of completeness and of a clear row 2 REL max |log-prob| over the row's
    reference top k + 1 (both compared values lie there, each off by at most REL of its size)."""
    ids, lp = ids.cpu(), lp.cpu()
    k = ids.shape[1]
    top = torch.sort(lp64, dim=1, descending=True).values[:, :k + 1]
    ref = T.Ref.from_logprobs(lp64, REL * top.abs().max(dim=1).values)
    T.check_values(ids, lp, ref, lp_bound=REL * lp64.gather(1, ids.long()).abs())
    T.check_complete(ids, ref)
    clear = T.check_exact(ids, ref)
    exact = float((ids.long() == T.topk_ref(lp64, k)).all(dim=1).double().mean())
    print(f"TOPK oracle {what}: rows {ids.shape[0]} k {k} clear share {clear:.3f} exact-match share {exact:.3f}")


def _padded_rows(tokens, hyp_off, mask_id):
    from oracle.bert_ref import _pad, pll_rows
    rows = list(pll_rows(tokens, hyp_off, mask_id))
    return _pad([r[1] for r in rows]), _pad([[1] * len(r[1]) for r in rows]), [r[2] for r in rows]


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_topk_nbest_tiny(w_tiny, precision):
    from asr_rescoring_amd.scorer import PLLScorer
    nb = D.synthetic_nbest(4, 3, seed=31, vocab=BERT_TINY.vocab, len_lo=3, len_hi=20)
    k = 5
    s = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=2048, precision=precision)
    s512 = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=512, precision=precision)
    try:
        pll0, rows0 = s.score_nbest(nb.tokens, nb.hyp_off, return_rows=True)
        ids, lp, pll, rows = s.topk_nbest(nb.tokens, nb.hyp_off, k, return_pll=True)
        ids2, lp2 = s.topk_nbest(nb.tokens, nb.hyp_off, k)                         # no pll / rows asked
        ids512, lp512 = s512.topk_nbest(nb.tokens, nb.hyp_off, k)
        pids, pam, mp = _padded_rows(nb.tokens, nb.hyp_off, BERT_TINY.mask_id)
        mids, mlp = s.masked_topk(pids, pam, mp, k)
        pll3 = s.score_nbest(nb.tokens, nb.hyp_off)                                # the default path afterwards
        # (random weights rarely rank a row's own token among the best: the same claim for every
        # returned id — rs_masked_logprob with that id as the label gives its log-prob bit for bit)
        as_label = []
        for j in range(k):
            labels = torch.zeros_like(pids)
            labels[torch.arange(len(mp)), torch.tensor(mp)] = ids[:, j].cpu().long()
            as_label.append(s.masked_logprob(pids, pam, labels, mp))
    finally:
        s.close()
        s512.close()
    assert ids.shape == (rows0.numel(), k) and ids.dtype == torch.int32 and lp.dtype == torch.float32
    assert torch.equal(pll.view(torch.int64), pll0.view(torch.int64)) and torch.equal(_bits(rows), _bits(rows0))
    assert torch.equal(pll3.view(torch.int64), pll0.view(torch.int64))
    assert torch.equal(ids, ids2) and torch.equal(_bits(lp), _bits(lp2))
    # a row's own token, where it is among the candidates, has the row's log-prob
    own = torch.from_numpy(np.concatenate([nb.tokens[nb.hyp_off[h] + 1:nb.hyp_off[h + 1] - 1]
                                           for h in range(nb.n_hyp)]).astype(np.int32)).cuda()
    hit = ids == own[:, None]
    print(f"TOPK tiny {precision}: own token among the top {k} in {int(hit.any(dim=1).sum())} of {len(own)} rows")
    assert torch.equal(_bits(lp[hit]), _bits(rows0[:, None].expand(-1, k)[hit]))
    assert torch.equal(_bits(torch.stack(as_label, dim=1)), _bits(lp)), "top_lp != rs_masked_logprob(label = top_id)"
    print(f"TOPK tiny {precision}: max_rows 512 vs 2048 max |dlp| {(lp512 - lp).abs().max().item():.3e}; "
          f"masked_topk vs topk_nbest max |dlp| {(mlp - lp).abs().max().item():.3e}")
    assert torch.equal(ids512, ids) and torch.equal(_bits(lp512), _bits(lp)), "max_rows 512 vs 2048"
    assert torch.equal(mids, ids) and torch.equal(_bits(mlp), _bits(lp)), "masked_topk vs topk_nbest"
    _check_vs_oracle(ids, lp, _oracle_logprobs(w_tiny, BERT_TINY, nb.tokens, nb.hyp_off), f"tiny {precision}")


def test_topk_decoder_sub_batches(w_tiny):
    """More than 2048 scored rows in one chunk: the top-k decoder runs its GEMM over row sub-batches
    (2048 + the rest, the candidate workspace reused), rs_pll_score's in one launch.  Scores bitwise
    rs_pll_score's, candidates bitwise those of chunks below one sub-batch (max_rows 2048)."""
    from asr_rescoring_amd.scorer import PLLScorer
    nb = D.synthetic_nbest(14, 5, seed=41, vocab=BERT_TINY.vocab, len_lo=30, len_hi=40)
    n_rows = int((np.diff(nb.hyp_off) - 2).sum())
    assert 2048 < n_rows < 2 * 2048 and n_rows % 256 != 0
    big = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=262144)
    small = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=2048)
    try:
        pll0, rows0 = big.score_nbest(nb.tokens, nb.hyp_off, return_rows=True)
        ids, lp, pll, rows = big.topk_nbest(nb.tokens, nb.hyp_off, 16, return_pll=True)
        ids_s, lp_s = small.topk_nbest(nb.tokens, nb.hyp_off, 16)
    finally:
        big.close()
        small.close()
    assert torch.equal(pll.view(torch.int64), pll0.view(torch.int64)) and torch.equal(_bits(rows), _bits(rows0))
    assert torch.equal(ids, ids_s) and torch.equal(_bits(lp), _bits(lp_s))
    assert (lp[:, 1:] <= lp[:, :-1]).all() and ((ids >= 0) & (ids < BERT_TINY.vocab)).all()


def test_topk_nbest_base(pll_base, w_base):
    """2 utterances x 3 hypotheses, one of 70 tokens: its chunk leaves the T <= 64 attention and dedup path."""
    rng = np.random.default_rng(5)
    lens = [[4, 5, 4], [68, 5, 6]]
    nb = D.from_lists([[rng.integers(106, BERT_BASE.vocab, size=n).tolist() for n in u] for u in lens])
    assert int(np.diff(nb.hyp_off).max()) == 70
    k = 5
    ids, lp, pll, rows = pll_base.topk_nbest(nb.tokens, nb.hyp_off, k, return_pll=True)
    pll0, rows0 = pll_base.score_nbest(nb.tokens, nb.hyp_off, return_rows=True)
    assert torch.equal(pll.view(torch.int64), pll0.view(torch.int64)) and torch.equal(_bits(rows), _bits(rows0))
    _check_vs_oracle(ids, lp, _oracle_logprobs(w_base, BERT_BASE, nb.tokens, nb.hyp_off), "base fp16x3")


# ---- errors ----------------------------------------------------------------------------------------

def test_topk_bad_k_and_null_outputs(w_tiny):
    from asr_rescoring_amd._lib import RescoreError
    from asr_rescoring_amd.scorer import PLLScorer
    nb = D.synthetic_nbest(1, 2, seed=5, vocab=BERT_TINY.vocab, len_lo=3, len_hi=6)
    pids, pam, mp = _padded_rows(nb.tokens, nb.hyp_off, BERT_TINY.mask_id)
    s = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=2048)
    try:
        for k in (0, 17, BERT_TINY.vocab + 1):
            with pytest.raises(RescoreError, match="error -1"):
                s.topk_nbest(nb.tokens, nb.hyp_off, k)
            with pytest.raises(RescoreError, match="error -1"):
                s.masked_topk(pids, pam, mp, k)
        lib, st = _lib.load(), _lib.stream_ptr(0)
        off = np.ascontiguousarray(nb.hyp_off, np.int32)
        tok = torch.from_numpy(nb.tokens.astype(np.int32)).cuda()
        n = int((np.diff(off) - 2).sum())
        tid = torch.empty((n, 3), dtype=torch.int32, device="cuda")
        tlp = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        assert lib.rs_pll_topk(s.handle, tok.data_ptr(), off.ctypes.data, len(off) - 1, 3, None, None, None,
                               tlp.data_ptr(), st) == -1
        assert lib.rs_pll_topk(s.handle, tok.data_ptr(), off.ctypes.data, len(off) - 1, 3, None, None, tid.data_ptr(),
                               None, st) == -1
        # d_pll and d_row_lp are optional
        assert lib.rs_pll_topk(s.handle, tok.data_ptr(), off.ctypes.data, len(off) - 1, 3, None, None, tid.data_ptr(),
                               tlp.data_ptr(), st) == 0
        assert torch.isfinite(tlp).all() and ((tid >= 0) & (tid < BERT_TINY.vocab)).all()
    finally:
        s.close()


def test_topk_needs_the_mlm_head(w_tiny):
    from asr_rescoring_amd.scorer import RescoreBertScorer
    nb = D.synthetic_nbest(1, 2, seed=5, vocab=BERT_TINY.vocab, len_lo=3, len_hi=6)
    s = RescoreBertScorer(w_tiny, BERT_TINY, device=0, max_rows=2048)
    try:
        lib, st = _lib.load(), _lib.stream_ptr(0)
        off = np.ascontiguousarray(nb.hyp_off, np.int32)
        tok = torch.from_numpy(nb.tokens.astype(np.int32)).cuda()
        n = int((np.diff(off) - 2).sum())
        tid = torch.empty((n, 3), dtype=torch.int32, device="cuda")
        tlp = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        q = np.ones(len(off) - 1, np.int32)
        assert lib.rs_pll_topk(s.handle, tok.data_ptr(), off.ctypes.data, len(off) - 1, 3, None, None, tid.data_ptr(),
                               tlp.data_ptr(), st) == -3                                           # RS_ESTATE
        assert lib.rs_masked_topk(s.handle, tok.data_ptr(), off.ctypes.data, q.ctypes.data, len(off) - 1, 3,
                                  tid.data_ptr(), tlp.data_ptr(), st) == -3
        assert b"MLM head" in lib.rs_last_error()
    finally:
        s.close()


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_topk_range_guard(w_tiny, precision):
    """test_fp16_range_guard's input (the embedding LayerNorm's gamma scaled until the first GEMM operand
    leaves the fp16 range): rs_pll_topk fails with RS_EUNSUP; deferred mode reports it at check()."""
    from asr_rescoring_amd._lib import RescoreError
    from asr_rescoring_amd.scorer import PLLScorer
    nb = D.synthetic_nbest(2, 3, seed=5, vocab=BERT_TINY.vocab, len_lo=3, len_hi=12)
    g = "bert.embeddings.LayerNorm.weight"
    for scale, ok in ((30.0, True), (1e6, False)):
        w = dict(w_tiny)
        w[g] = w_tiny[g] * scale
        s = PLLScorer(w, BERT_TINY, device=0, max_rows=2048, precision=precision)
        try:
            if ok:
                assert torch.isfinite(s.topk_nbest(nb.tokens, nb.hyp_off, 4)[1]).all()
                continue
            with pytest.raises(RescoreError, match="error -5.*non-finite"):
                s.topk_nbest(nb.tokens, nb.hyp_off, 4)
            s.set_sync_check(False)
            s.topk_nbest(nb.tokens, nb.hyp_off, 4)                       # no exception: deferred
            with pytest.raises(RescoreError, match="non-finite"):
                s.check()
            s.check()                                                    # cleared
            s.set_sync_check(True)
        finally:
            s.close()


# ---- CLI -------------------------------------------------------------------------------------------

def test_cli_mlm_topk(golden_dir, tmp_path, pll_base):
    from asr_rescoring_amd import cli
    g = json.load(open(os.path.join(golden_dir, "c1_plumbing.json"), encoding="utf-8"))
    d = tmp_path
    json.dump(g["hyps_text"], open(d / "hyps_text.json", "w", encoding="utf-8"), ensure_ascii=False)
    special = {0: "[PAD]", 100: "[UNK]", 101: "[CLS]", 102: "[SEP]", 103: "[MASK]"}
    lines = [special.get(i, f"[unused{i}]") for i in range(106)] + list(g["charset"])
    (d / "vocab.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    cfg = d / "topk.yaml"
    cfg.write_text(yaml.safe_dump({
        "task": "scoring", "device": "cuda:0", "random_init_seed": 1234, "top_k": 3, "n_best": 2, "max_utt": 2,
        "max_rows": 4096, "train_hyps_text_path": str(d / "hyps_text.json"), "output_path": str(d) + "/",
        "model": {"bert": "bert-base-chinese", "vocab": str(d / "vocab.txt")}}, allow_unicode=True), encoding="utf-8")
    assert "mlm_topk" in cli.COMMANDS
    assert cli.main(["mlm_topk", "--config", str(cfg)]) == 0
    path = d / "train_topk.json"
    assert path.exists()
    got = json.load(open(path, encoding="utf-8"))
    utts = g["utt_ids"][:2]
    assert list(got) == utts
    from asr_rescoring_amd.frontend import NativeTokenizer
    nb, keys = cli._nbest_tokens(g["hyps_text"], NativeTokenizer(str(d / "vocab.txt")), 2, 2)
    ids, lp = pll_base.topk_nbest(nb.tokens, nb.hyp_off, 3)
    ids, lp = ids.cpu().tolist(), lp.cpu().tolist()
    r = 0
    for h, (u, hid) in enumerate(keys):
        L = int(nb.hyp_off[h + 1] - nb.hyp_off[h]) - 2
        e = got[u][hid]
        assert list(got[u]) == list(g["hyps_text"][u])[:2]
        assert len(e["ids"]) == L and len(e["logprob"]) == L and all(len(x) == 3 for x in e["ids"] + e["logprob"])
        assert e["ids"] == ids[r:r + L] and e["logprob"] == lp[r:r + L]
        r += L
    assert r == len(ids)
