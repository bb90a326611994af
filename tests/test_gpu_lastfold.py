"""GPU: the folded last-layer attention (RS_LASTFOLD): the K / V projections applied to the query
side, so that no K / V row of the chunk is projected.

Direct parity (rs_debug_attention_fold -> launch_attention_fold: fold_gemm_kernel<false>,
attn_fold_kernel, fold_gemm_kernel<true>), heads 12, H 768, against numpy float64 of the UNFOLDED
formulation on the same inputs: K = x Wk^T + bk and V = x Wv^T + bv for every row x of the sequence
(the values the two-part image holds), then softmax(q_h . K_h^T / 8) . V_h for the scored row.  The
kernels never see bk: q_h . bk_h is the same for every key and cancels in the softmax, which the
bk x 100 case shows.  ctxq is held to the bound tests/test_gpu_attn_query.py has for the kx = 3
ctxq of launch_attention_query: err <= 4 max(e32, 2^-21 max|y|), e32 the same unfolded expression in
float32, after the exact checks of the image alone (tail_ref.image3_defects).  resq: hi + lo/64 of
the scored row's image, bitwise.  Every launch runs sequences [1, 1 + n) of a metadata array with a
leading and a trailing sequence, gaps between the row ranges, and output buffers one row per sequence
of the whole array whose rows past n must keep their sentinel.

Shapes: T = 3; 48, 49, 64, 65 (the staged-key boundaries of the neighbouring attention kernels; the
fold kernel's own tile is 24 rows, so 48 / 49 is also its two / three tile edge); 512 (the model's
longest); five sequences of T = 3, 24, 25, 130, 7 in one launch (n = 5 is no multiple of the GEMM
tiles' 32 rows), the query at the first, last and an interior position; that chunk again with bk x 100,
and with a scratch buffer of two sequences (the launcher's batches: 2 + 2 + 1).  The other hidden sizes
the fold accepts, H = 256, 512, 1024 with heads = H / 64 (attn_fold_kernel<1>, <2>, <4>: 256 / 512 / 1024
threads, 24 / 48 / 96 KiB of LDS), run T3, T49, chunk5 and chunk5-batches with the same reference,
sentinel checks and bound.

Through the scorer: RS_LASTFOLD=0 / 1 both within the golden test's bounds of tests/golden/
pll_base.npz and not array-equal (the switch takes effect), also at max_rows = 512 (hypotheses cut
across chunks; a chunk's G and U no longer fit the QKV buffer at once); two folded calls bitwise
equal, and equal to the folded call under RS_LASTQ=0 (the scored rows' Q gathered out of the full
Q/K/V GEMM's output: the same bits, as tests/test_gpu_bert.py::test_lastq_full_layer_is_exact asks); RS_X3S=0, RS_X3S_IMGRES=0 and the fp16 mode the same bits with RS_LASTFOLD=0 and 1 (the fold
is not taken there).

Measured on MI355X (printed per case, LASTFOLD lines): err 1.4e-6 .. 3.5e-6 with e32 1.7e-6 .. 2.6e-6,
err / e32 0.79 .. 1.37, err / bound 0.20 .. 0.34 (the worst sequence of the chunk is its T = 3 one);
bk x 100: the same err (3.5e-6, the kernels' bits do not depend on bk) against an e32 of 1.5e-5 (the
unfolded float32 scores carry the large constant), err / bound 0.06.  H 256 / 512 / 1024: err 3.1e-7 ..
5.6e-6, err / e32 0.71 .. 2.07, err / bound 0.14 .. 0.52 (the worst: H 1024 chunk5).  Scorer on the fixture: PLL
1.8e-7 / rows 1.4e-6 folded, 1.5e-7 / 1.2e-6 with RS_LASTFOLD=0 (bounds 1e-6 / 5e-6), the two within
7.5e-8 (PLL) and 5.4e-7 (rows) of each other, the same figures at max_rows 512.
"""
import os

import numpy as np
import pytest
import torch

from asr_rescoring_amd import _lib
from asr_rescoring_amd.weights import BERT_BASE, make_weights
import tail_ref as R
from x3s_image import _split2, _unsplit2

pytestmark = pytest.mark.gpu

H, HEADS = 768, 12
SENT32, SENT16 = 0x7FC12345, 0x7E5A
# name -> (T per sequence, query position per sequence, bk scale, scratch sequences (0: all))
CASES = {
    "T3": ([3], [1], 1.0, 0),
    "T48": ([48], [0], 1.0, 0),
    "T49": ([49], [48], 1.0, 0),
    "T64": ([64], [63], 1.0, 0),
    "T65": ([65], [0], 1.0, 0),
    "T512": ([512], [511], 1.0, 0),
    "chunk5": ([3, 24, 25, 130, 7], [0, 23, 12, 129, 6], 1.0, 0),
    "chunk5-bk100": ([3, 24, 25, 130, 7], [0, 23, 12, 129, 6], 100.0, 0),
    "chunk5-batches": ([3, 24, 25, 130, 7], [0, 23, 12, 129, 6], 1.0, 2),
}


# the other hidden sizes attention_fold_ok accepts (heads = H / 64): attn_fold_kernel<1>, <2>, <4>
OTHER_H = (256, 512, 1024)
OTHER_H_CASES = ("T3", "T49", "chunk5", "chunk5-batches")
H_CASES = [(H, n) for n in CASES] + [(h, n) for h in OTHER_H for n in OTHER_H_CASES]
H_CASE_IDS = [n if h == H else f"H{h}-{n}" for h, n in H_CASES]


@pytest.fixture(scope="module")
def fold_weights():
    """H -> Wk, bk, Wv, bv (fp32, shared by every case of that H and left unchanged)."""
    made = {}

    def get(H):
        if H not in made:
            gen = torch.Generator().manual_seed(4242)
            rn = lambda *s: torch.randn(*s, generator=gen)
            made[H] = {"wk": (0.05 * rn(H, H)).contiguous(), "bk": (0.3 * rn(H)).contiguous(),
                       "wv": (0.05 * rn(H, H)).contiguous(), "bv": (0.3 * rn(H)).contiguous()}
        return made[H]
    return get


def _layout(Ts, qs, gap=3):
    """One leading and one trailing sequence (T = 5) around the case's, row ranges `gap` rows apart."""
    T = [5] + list(Ts) + [5]
    query = [2] + list(qs) + [2]
    row, r = [], gap
    for t in T:
        row.append(r)
        r += t + gap
    return T, row, query, r


def _unfolded(x, q, w, bk_scale, T, row, query, dtype):
    """softmax(q_h . K_h^T / 8) . V_h of sequences [1, len(T) - 1) with K, V projected for every row."""
    f = lambda t: t.numpy().astype(dtype)
    wk, wv, bk, bv = f(w["wk"]), f(w["wv"]), f(w["bk"]) * dtype(bk_scale), f(w["bv"])
    H = wk.shape[0]
    HEADS = H // 64
    out = np.zeros((len(T) - 2, H), dtype)
    for i, s in enumerate(range(1, len(T) - 1)):
        xs = x[row[s]:row[s] + T[s]].astype(dtype)
        K, V = xs @ wk.T + bk, xs @ wv.T + bv
        for h in range(HEADS):
            c = slice(64 * h, 64 * h + 64)
            sc = (K[:, c] @ q[i, c].astype(dtype)) * dtype(0.125)
            p = np.exp(sc - sc.max())
            out[i, c] = (p / p.sum()) @ V[:, c]
    return out


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("H,name", H_CASES, ids=H_CASE_IDS)
def test_fold_vs_float64_unfolded(H, name, fold_weights):
    HEADS = H // 64
    fold_weights = fold_weights(H)
    Ts, qs, bk_scale, scratch = CASES[name]
    T, row, query, rows = _layout(Ts, qs)
    n, n_seq = len(Ts), len(T)
    gen = torch.Generator().manual_seed(100 + sum(Ts))
    himg = _split2(torch.randn(rows, H, generator=gen))          # every row distinct, gaps included
    x = _unsplit2(himg, torch.float64).numpy()                   # the values the image holds
    q = (1.4 * torch.randn(n, H, generator=gen)).contiguous()
    ref = _unfolded(x, q.numpy(), fold_weights, bk_scale, T, row, query, np.float64)
    e32 = np.abs(_unfolded(x, q.numpy(), fold_weights, bk_scale, T, row, query, np.float32).astype(np.float64) - ref).max()

    w = fold_weights
    d = lambda t: t.cuda().contiguous()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    dT, drow, dq = i32(T), i32(row), i32(query)
    himg_d, wkf, wvt, bv = d(himg), d(w["wk"] * 0.125), d(w["wv"].t()), d(w["bv"])
    # rows [0, n): the launch's Q; the rest other rows (never read)
    tq = d(torch.cat([q, 3.0 - 0.5 * q[:1].expand(n_seq - n, H)]))
    n_work = scratch if scratch else n
    work = torch.empty(n_work * 2 * HEADS * H, dtype=torch.float32, device="cuda")

    def run():
        ctxq = torch.full((n_seq, 3 * H), SENT16, dtype=torch.int16, device="cuda").view(torch.float16)
        resq = torch.full((n_seq, H), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
        rc = _lib.load().rs_debug_attention_fold(
            himg_d.data_ptr(), tq.data_ptr(), wkf.data_ptr(), wvt.data_ptr(), bv.data_ptr(), dT.data_ptr(),
            drow.data_ptr(), dq.data_ptr(), 1, 1 + n, 0, H, HEADS, 3, work.data_ptr(), work.numel() * 4,
            ctxq.data_ptr(), resq.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return ctxq, resq

    ctxq, resq = run()
    assert (_bits(ctxq[n:]) == SENT16).all() and (_bits(resq[n:]) == SENT32).all(), "rows past s1 - s0 written"
    got = ctxq[:n].cpu()
    assert R.image3_defects(got) == []
    val = R._unsplit3(got, torch.float64).numpy()
    assert np.isfinite(val).all()
    err_s = np.abs(val - ref).max(axis=1)
    err = err_s.max()
    bound = 4 * max(e32, 2.0 ** -21 * np.abs(ref).max())
    print(f"LASTFOLD H{H} {name}: err {err:.3e} (T of the worst sequence {Ts[int(err_s.argmax())]}) e32 {e32:.3e} "
          f"err/e32 {err / max(e32, 1e-300):.2f} err/bound {err / bound:.3f}")
    qrow = torch.tensor([row[s] + query[s] for s in range(1, 1 + n)])
    assert torch.equal(resq[:n].cpu().double(), _unsplit2(himg[qrow], torch.float64)), "resq != hi + lo/64"
    again = run()
    assert torch.equal(_bits(ctxq), _bits(again[0])) and torch.equal(_bits(resq), _bits(again[1])), "run-to-run"
    assert err <= bound, (H, name, err, e32, bound)


def test_fold_rejects_bad_arguments():
    """The entry's argument checks (no kernel runs)."""
    z = torch.zeros(64 * 1024, device="cuda")
    meta = torch.zeros(4, dtype=torch.int32, device="cuda")
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream

    def call(H_=768, heads=12, kx=3, s1=1, work_bytes=z.numel() * 4, bv=z.data_ptr()):
        p = z.data_ptr()
        return lib.rs_debug_attention_fold(p, p, p, p, bv, meta.data_ptr(), meta.data_ptr(), meta.data_ptr(), 0, s1, 0,
                                           H_, heads, kx, p, work_bytes, p, p, st)
    assert call(H_=128, heads=2) != 0        # H % 256
    assert call(H_=768, heads=6) != 0        # H != 64 heads
    assert call(kx=2) != 0
    assert call(s1=0) != 0
    assert call(bv=None) != 0
    assert call(work_bytes=2 * 12 * 768 * 4 - 4) != 0     # not one sequence's G and U
    torch.cuda.synchronize()
    assert not z.any()


# ---- through the scorer ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def w_base():
    return make_weights(BERT_BASE, seed=1234, with_cls_linear=True, with_pooler=True)


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pll_base.npz"), allow_pickle=False)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


def _score(s, g, monkeypatch, fold):
    monkeypatch.setenv("RS_LASTFOLD", fold)
    pll, rows = s.score_nbest(g["tokens"], g["hyp_off"], return_rows=True)
    return pll.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("max_rows", [4096, 512])
def test_switch_equivalence_and_determinism(w_base, golden_dir, monkeypatch, max_rows):
    """RS_LASTFOLD=0 and =1: both within the golden test's bounds (1e-6 PLL, 5e-6 rows) of the fixture,
    not array-equal; the folded call twice: the same bits."""
    from asr_rescoring_amd.scorer import PLLScorer
    g = _golden(golden_dir)
    s = PLLScorer(w_base, BERT_BASE, device=0, max_rows=max_rows, precision="fp16x3")
    try:
        off = _score(s, g, monkeypatch, "0")
        on = _score(s, g, monkeypatch, "1")
        on2 = _score(s, g, monkeypatch, "1")
        monkeypatch.setenv("RS_LASTQ", "0")                      # Q out of the full Q/K/V GEMM, still folded
        on_fullq = _score(s, g, monkeypatch, "1")
    finally:
        s.close()
    for tag, (pll, rows) in (("RS_LASTFOLD=0", off), ("RS_LASTFOLD=1", on)):
        e_pll, e_rows = _rel(pll, g["pll"]).max(), _rel(rows, g["row_lp"]).max()
        print(f"LASTFOLD golden max_rows={max_rows} {tag}: pll {e_pll:.3e} rows {e_rows:.3e}")
        assert e_pll < 1e-6, tag
        assert e_rows < 5e-6, tag
    print(f"LASTFOLD max_rows={max_rows} on vs off: pll {_rel(on[0], off[0]).max():.3e} rows {_rel(on[1], off[1]).max():.3e}")
    assert not np.array_equal(on[1], off[1])                     # the switch really took effect
    assert np.array_equal(on[0], on2[0]) and np.array_equal(on[1], on2[1]), "run-to-run"
    assert np.array_equal(on[0], on_fullq[0]) and np.array_equal(on[1], on_fullq[1]), "RS_LASTQ=0 folded"


@pytest.mark.parametrize("precision,env", [("fp16x3", ("RS_X3S", "0")), ("fp16x3", ("RS_X3S_IMGRES", "0")), ("fp16", None)],
                         ids=["x3s0", "imgres0", "fp16"])
def test_fallback_paths_ignore_the_switch(w_base, golden_dir, monkeypatch, precision, env):
    """Where the fold is not taken, RS_LASTFOLD changes no bit."""
    from asr_rescoring_amd.scorer import PLLScorer
    g = _golden(golden_dir)
    if env:
        monkeypatch.setenv(*env)
    s = PLLScorer(w_base, BERT_BASE, device=0, max_rows=4096, precision=precision)
    try:
        off = _score(s, g, monkeypatch, "0")
        on = _score(s, g, monkeypatch, "1")
    finally:
        s.close()
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
