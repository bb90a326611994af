"""GPU: the GEMM launches of the scoring tail — the last layer's one-row-per-sequence GEMMs and
the MLM head — through the production launchers, against float64.

* rs_debug_gemm_epi: one launch_gemm per case, i.e. the pipelined gemm_f16_kernel with the
  EPI_RES_F32 / EPI_GELU_F32 / EPI_BIAS_F32 / EPI_RESLN_F32 (plain, in place; deferred res_o16)
  epilogues and the persistent kernel's GELU images (EPI_GELU_F16, kx = 3: P_X3IMG; kx = 1).
* rs_debug_decoder: launch_mlm_decoder, the function rs_api.hip's head_mlm runs — labels (and the
  label logits' -inf), the EPI_LSE GEMM on the 256 x 256 (vpad % 256 == 0) or the 256 x 128 tile,
  lse_finalize.
* the out-of-range label through the product (rs_masked_logprob, rs_pll_score) and a PLLScorer
  whose decoder runs on the 256 x 128 tile (vocab 1100).

Reference (tests/tail_ref.py): float64 on the values the fp16 operands hold.  Yardstick: the same
expression in torch fp32, e32 = its max |error| against float64.  Asserted per case:
    err <= 4 max(e32, q)
q twice the output's own quantisation: 2^-23 max|y| (fp32 outputs), 2^-21 max|y| (three-part image
decoded as hi + lo/64), 2^-10 max|y| (kx = 1 fp16 image), 2^-23 max(|label logit|, |lse|) (decoder
log-prob).  Operand families: random fp16, and the real K-concatenated images [hi | hi/64 | lo*64] .
[W_hi | W_lo*64 | W_hi/64] (image3).

Every case: out starts as a NaN sentinel and rows >= m_valid must keep it bitwise; rows < m_valid
are bitwise the same with NaN in the pad rows of A; a repeat run is bitwise equal.  Three-part
images are checked exactly on their own (tail_ref.image3_defects) before they are decoded.

Measured err / e32 on MI355X (m_valid 1 / 37 / 256 / 300), every epilogue case at or below 0.75 of
its bound; the image3 family sits at err ~ e32 like the fp16 one, so the fp16 MFMA keeps subnormal
operands (flushed, they would cost 48 .. 95 e32, the hi/64 sections alone 2.8 .. 4.9: test_tail_ref.py):
    res     image3 N 256 K 768   1.22 0.75 0.87 2.92    fp16  1.06 0.99 0.75 2.10
            image3 N 256 K 3072  1.36 1.74 1.98 2.41    fp16  0.89 1.39 1.45 2.28
            image3 N 768 K 2304  0.53 0.37 0.70 0.66    fp16  0.63 0.58 0.53 0.49
            image3 N 768 K 9216  0.38 0.29 0.33 0.51    fp16  0.22 0.62 0.48 0.46
    gelu32  image3 N 256 K 768   1.58 1.02 1.42 3.00    fp16 N 256 K 768  0.99 0.85 0.73 2.69
            image3 N 768 K 2304  0.99 0.89 0.63 0.74    fp16 N 768 K 768  1.01 0.83 0.88 0.68
    window  image3 N 512 K 768   0.83 1.32 1.17 0.39    fp16  0.86 1.62 1.32 0.40
            image3 N 1536 K 2304 0.43 0.34 0.41 0.36    fp16  0.39 0.37 0.31 0.41
    resln   fp16 N 768 K 768     0.99 0.64 0.68 0.72    image3 N 768 K 9216  0.39 0.37 0.34 0.38
    defer   fp16 N 768 K 3072    0.98 0.48 0.46 0.48
    gelu16  kx 3 N 1024 K 768    1.90 1.04 1.07 0.92    kx 3 N 3072 K 2304  0.36 0.62 0.76 0.77
            kx 1: err / bound 0.07 .. 0.11 (the fp16 rounding of the output, far above e32)
    decoder (every case at or below 0.33 of its bound, on both tiles)
            plain        V 1000 6.44 0.98 1.31 1.31   V 1025 2.47 0.95 0.79 0.79   V 1100 2.35 1.01 1.11 1.11
                         V 1153 1.00 0.42 0.67 0.67   V 21128 0.06 0.23 0.48 0.48  V 30522 41.8 1.07 0.89 0.89
                         (m_valid 1: one row, e32 down to 2e-8; err / bound <= 0.20 there)
            flat         0.42 .. 2.82
            peaked       0.69 .. 1.07 (m_valid 1: err = e32 = 0)
            slab_spread  0.88 .. 1.53 (V 30522, m_valid 1: 0.14)
    PLLScorer vocab 1100 against the oracle: max rel err 1.4e-4 (fp16), 9.3e-8 (fp16x3).

The peaked and slab_spread families found a loss of accuracy in the decoder GEMM: at first 18 of
their 48 cases exceeded the bound, by up to 2.3 times (err up to 2.3e-4, err / e32 up to 11; worst
at K 2304, the same on both tiles).  Cause (not __expf): gemm_f16_kernel started the accumulators of
every epilogue at the bias, to hide the bias loads behind the K loop, so every one of the K / 16
MFMA steps rounded at the magnitude of the bias — 80 and 200 here, one ulp 7.6e-6 / 1.5e-5 — where
the reference adds the bias once, to a product of magnitude ~1: an error of about |b| sqrt(K) 2^-24.
Emulated on the CPU in fp32 (acc = b, then += A[:, k:k+16] . W[:, k:k+16]^T): 8.3e-5 (slab_spread
V 1153 K 768; measured 1.2e-4) and 5.0e-5 (peaked; measured 6.2e-5), against 8.0e-6 / 4.2e-6 with the
bias added last.  EPI_LSE now starts its accumulators at 0 and adds the bias after the K loop (the
figures above); valid-input log-probs move in their last bits (PLL: see DESIGN.md section 2), and the
other epilogues, whose bias and residual are of the size of the product, keep their form.

Scratch builds (not kept), one run each (made while the bias still started the accumulators):
    (a) EPI_LSE without the `col + e < n_valid` mask: plain and flat fail at all 48 cases by 5e6 ..
        3e7 times the bound (the poisoned pad columns), peaked at 21 of 24, slab_spread at 7 of 24
        (next to the +200 slab a pad logit of ~30 vanishes), and the flat, out-of-range-label and
        vocab-1100 PLLScorer tests fail;
    (b) the label compared with col + e + 1: all 96 decoder cases fail (label 0 matches no column:
        -inf; the others are off by the difference of two logits, up to 2e6 times the bound), with
        the same three tests;
    (c) lse_finalize without the `p[k].y > 0` guard: nothing changes — a wholly masked slab stores
        (-inf, 0), the row maximum is finite as soon as one column is valid, and 0 * exp(-inf - mx)
        is 0: the guard only matters for a row with no valid column, which vocab >= 1 excludes.
    The parent commit's library fails the four out-of-range-label product tests (the calls return
    finite numbers).
"""
import ctypes

import numpy as np
import pytest
import torch

from asr_rescoring_amd import _lib
import tail_ref as R

pytestmark = pytest.mark.gpu

ROWS = [(256, 1), (256, 37), (256, 256), (512, 300)]                        # (M_pad, m_valid)
SENT32, SENT16 = 0x7FC12345, 0x7E5A                                          # NaN sentinels (bit patterns)

# (kind, family, N, K); kind as tail_ref.epi_operands, plus "window" (EPI_BIAS_F32 into columns
# [H, 3H) of an ldc = 3H buffer, N = 2H), "resln" in place (out == res) and "gelu16x3" / "gelu16x1"
EPI_SHAPES = (
    [("res", f, N, K) for N, K in ((256, 3 * 256), (256, 3 * 1024), (768, 3 * 768), (768, 3 * 3072))
     for f in ("image3", "fp16")]
    + [("gelu32", "image3", 256, 3 * 256), ("gelu32", "fp16", 256, 768), ("gelu32", "fp16", 768, 768),
       ("gelu32", "image3", 768, 3 * 768)]
    + [("window", f, 2 * H, 3 * H) for H in (256, 768) for f in ("image3", "fp16")]
    + [("resln", "fp16", 768, 768), ("resln", "image3", 768, 3 * 3072)]
    + [("defer", "fp16", 768, 3072)]
    + [("gelu16x3", "image3", 1024, 3 * 256), ("gelu16x3", "image3", 3072, 3 * 768),
       ("gelu16x1", "fp16", 1024, 256), ("gelu16x1", "fp16", 3072, 768)])
EPI_CASES = [s + r for s in EPI_SHAPES for r in ROWS]
_EPI = {"res": R.EPI_RES_F32, "gelu32": R.EPI_GELU_F32, "window": R.EPI_BIAS_F32, "resln": R.EPI_RESLN_F32,
        "defer": R.EPI_RESLN_F32, "gelu16x3": R.EPI_GELU_F16, "gelu16x1": R.EPI_GELU_F16}
_REF_KIND = {"window": "bias", "gelu16x3": "gelu16", "gelu16x1": "gelu16"}


def _id(c):
    return "-".join(str(x) for x in c[:2]) + f"-N{c[2]}-K{c[3]}-M{c[4]}-v{c[5]}"


_ops = {}


def _operands(kind, family, N, K, M_pad):
    """Operands, float64 reference and e32 per row of one (shape, M_pad): computed once, never modified."""
    key = (kind, family, N, K, M_pad)
    if key not in _ops:
        if len(_ops) >= 3:
            _ops.pop(next(iter(_ops)))
        rk = _REF_KIND.get(kind, kind)
        op = R.epi_operands(rk, family, M_pad, N, K, seed=N + K + M_pad + 7 * len(kind) + len(family), device="cuda")
        y = R.epi_ref(rk, op, torch.float64)
        e_rows = (R.epi_ref(rk, op, torch.float32).double() - y).abs().max(dim=1).values
        _ops[key] = (op, y, e_rows)
    return _ops[key]


def _sentinel(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(torch.float16)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _launch_epi(kind, op, N, K, M_pad, m_valid, A=None):
    """One rs_debug_gemm_epi launch on fresh sentinel-filled buffers -> (whole out buffer, window)."""
    A = op["A"] if A is None else A
    a = _lib.DebugGemmEpi()
    a.bias, a.m_valid, a.kx, a.nlog = op["b"].data_ptr(), m_valid, 1, N
    keep = [A]
    if kind in ("gelu16x3", "gelu16x1"):
        kx = 3 if kind == "gelu16x3" else 1
        buf = _sentinel((M_pad, kx * N), torch.float16)
        win, a.ldc, a.kx = buf, kx * N, kx
    elif kind == "window":
        H = N // 2
        buf = _sentinel((M_pad, 3 * H), torch.float32)
        win, a.ldc = buf[:, H:], 3 * H
    elif kind == "resln":
        # in place: the residual buffer is the output; its pad rows hold the sentinel
        buf = op["res"].clone()
        buf[m_valid:] = _sentinel((M_pad - m_valid, N), torch.float32)
        win, a.ldc, a.res = buf, N, buf.data_ptr()
    else:
        buf = _sentinel((M_pad, N), torch.float32)
        win, a.ldc = buf, N
    a.out = win.data_ptr()
    if kind in ("res", "defer"):
        a.res = op["res"].data_ptr()
    if kind in ("resln", "defer"):
        a.res_stats, a.res_g, a.res_b = op["stats"].data_ptr(), op["g"].data_ptr(), op["beta"].data_ptr()
    if kind == "defer":
        a.res_o16, a.res_stats0 = op["o16"].data_ptr(), op["stats0"].data_ptr()
        a.res_g0, a.res_b0 = op["g0"].data_ptr(), op["beta0"].data_ptr()
    assert A.is_contiguous() and A.shape == (M_pad, K) and op["W"].shape == (N, K) and op["W"].is_contiguous()
    rc = _lib.load().rs_debug_gemm_epi(_EPI[kind], A.data_ptr(), op["W"].data_ptr(), M_pad, N, K, ctypes.byref(a),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return buf, win


@pytest.mark.parametrize("case", EPI_CASES, ids=_id)
def test_epilogue_vs_float64(case):
    """Parity, untouched pad rows, run-to-run and pad-row independence of one epilogue case.
    (gemm_persist_kernel's stores used to be unconditional — whole 256-row panels, pad rows included —
    where EpiArgs.m_valid says "rows >= m_valid are not stored"; with this test its last row panel
    skips those rows, which the gelu16 cases with m_valid < M_pad pin.)"""
    kind, family, N, K, M_pad, m_valid = case
    op, y, e_rows = _operands(kind, family, N, K, M_pad)
    y, e32 = y[:m_valid], e_rows[:m_valid].max().item()
    buf, win = _launch_epi(kind, op, N, K, M_pad, m_valid)
    dt = buf.dtype
    # rows >= m_valid (and the columns outside a window) keep the sentinel bitwise
    sent = SENT32 if dt == torch.float32 else SENT16
    assert (_bits(buf[m_valid:]) == sent).all(), "pad rows written"
    if kind == "window":
        assert (_bits(buf[:, :N // 2]) == SENT32).all(), "columns [0, H) of the window buffer written"
    got = win[:m_valid]
    if kind == "gelu16x3":
        assert R.image3_defects(got) == []
        val, q = R._unsplit3(got, torch.float64), 2.0 ** -21
    else:
        val, q = got.double(), 2.0 ** (-10 if kind == "gelu16x1" else -23)
    assert torch.isfinite(val).all()
    err = (val - y).abs().max().item()
    bound = 4 * max(e32, q * y.abs().max().item())
    print(f"EPI {_id(case)}: err {err:.3e} e32 {e32:.3e} err/e32 {err / max(e32, 1e-300):.2f} err/bound {err / bound:.3f}")
    # a repeat run; NaN in the pad rows of A
    _, again = _launch_epi(kind, op, N, K, M_pad, m_valid)
    assert torch.equal(_bits(got), _bits(again[:m_valid])), "run-to-run"
    if m_valid < M_pad:
        A = op["A"].clone()
        A[m_valid:] = float("nan")
        _, nan_pad = _launch_epi(kind, op, N, K, M_pad, m_valid, A=A)
        assert torch.equal(_bits(got), _bits(nan_pad[:m_valid])), "valid rows depend on the pad rows of A"
    assert err <= bound, (_id(case), err, e32, bound)


def test_gemm_epi_rejects_bad_arguments():
    """The entry's argument checks (no kernel runs): an epilogue it does not serve, a missing
    residual / statistics / deferred set, an image narrower than kx nlog."""
    op = R.epi_operands("defer", "fp16", 256, 256, 256, seed=3, device="cuda")
    out = _sentinel((256, 768), torch.float32)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream

    def call(epi, **kw):
        a = _lib.DebugGemmEpi()
        a.bias, a.out, a.ldc, a.m_valid, a.kx, a.nlog = op["b"].data_ptr(), out.data_ptr(), 256, 256, 1, 256
        a.res, a.res_stats, a.res_g, a.res_b = (op[k].data_ptr() for k in ("res", "stats", "g", "beta"))
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.rs_debug_gemm_epi(epi, op["A"].data_ptr(), op["W"].data_ptr(), 256, 256, 256, ctypes.byref(a), st)
    assert call(0) != 0 and call(4) != 0 and call(7) != 0        # EPI_BIAS_F16, EPI_LSE, EPI_LNRES_IMG
    assert call(R.EPI_RES_F32, res=None) != 0
    assert call(R.EPI_RESLN_F32, res_stats=None) != 0
    assert call(R.EPI_RESLN_F32, res_o16=op["o16"].data_ptr()) != 0          # deferred set incomplete
    assert call(R.EPI_GELU_F16, kx=3, ldc=512) != 0
    assert call(R.EPI_GELU_F16, kx=2, ldc=512) != 0
    assert call(R.EPI_BIAS_F32, m_valid=257) != 0
    assert call(R.EPI_BIAS_F32, out=None) != 0
    torch.cuda.synchronize()
    assert (_bits(out) == SENT32).all()


# ---- decoder -------------------------------------------------------------------------------------

# (V, K): vpad = ceil(V / 128) 128; launch_epi routes vpad % 256 == 0 to the 256 x 256 tile, else 256 x 128
DEC_SHAPES = [(1000, 256), (1153, 3 * 256), (21128, 3 * 768),      # vpad 1024, 1280, 21248: 256 x 256
              (1025, 256), (1100, 256), (30522, 768)]              # vpad 1152, 1152, 30592: 256 x 128
DEC_CASES = [(f, V, K) + r for V, K in DEC_SHAPES for f in R.DECODER_FAMILIES for r in ROWS]
_dec = {}


def _dec_id(c):
    return f"{c[0]}-V{c[1]}-K{c[2]}-M{c[3]}-v{c[4]}"


def _decoder_case(family, V, K):
    """Operands for 512 rows and the float64 / fp32 references per row, once per (family, V, K);
    the weight once per (V, K)."""
    wkey, key = ("W", V, K), (family, V, K)
    if wkey not in _dec:
        for k in [k for k in _dec if k[0] == "W"]:
            del _dec[k]
        _dec[wkey] = R.decoder_weight(V, K, seed=V + K, device="cuda")
    W = _dec[wkey]
    if key not in _dec:
        A, b, lab = R.decoder_operands(family, 512, V, K, W, seed=V + K + len(family), device="cuda")
        lp, ll, lse = R.decoder_ref(A, W, b, lab, V, torch.float64)
        lp32 = R.decoder_ref(A, W, b, lab, V, torch.float32)[0]
        _dec[key] = (A, b, lab, lp, (lp32.double() - lp).abs(), torch.maximum(ll.abs(), lse.abs()))
    return (W,) + _dec[key]


def _launch_decoder(A, W, b, lab, M_pad, m_valid, V):
    """One rs_debug_decoder launch on sentinel-filled workspace -> out [m_valid], part, llog."""
    vpad, K = W.shape
    A = A[:M_pad].contiguous()
    part = _sentinel((M_pad, vpad // 64, 2), torch.float32)
    llog = _sentinel((M_pad,), torch.float32)
    out = _sentinel((m_valid,), torch.float32)
    labw = torch.full((m_valid,), -12345, dtype=torch.int32, device="cuda")
    lab = lab[:m_valid].contiguous()
    rc = _lib.load().rs_debug_decoder(A.data_ptr(), W.data_ptr(), b.data_ptr(), lab.data_ptr(), M_pad, m_valid, vpad, V,
                                      K, labw.data_ptr(), part.data_ptr(), llog.data_ptr(), out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(labw, lab)
    return out, part, llog


@pytest.mark.parametrize("case", DEC_CASES, ids=_dec_id)
def test_decoder_vs_float64(case):
    family, V, K, M_pad, m_valid = case
    W, A, b, lab, lp, e_rows, scale = _decoder_case(family, V, K)
    out, part, llog = _launch_decoder(A, W, b, lab, M_pad, m_valid, V)
    assert (_bits(part[m_valid:]) == SENT32).all() and (_bits(llog[m_valid:]) == SENT32).all(), "pad rows written"
    assert torch.isfinite(out).all()
    err = (out.double() - lp[:m_valid]).abs().max().item()
    e32 = e_rows[:m_valid].max().item()
    bound = 4 * max(e32, 2.0 ** -23 * scale[:m_valid].max().item())
    print(f"DEC {_dec_id(case)} tile 256x{R.decoder_tile(W.shape[0])}: err {err:.3e} e32 {e32:.3e} "
          f"err/e32 {err / max(e32, 1e-300):.2f} err/bound {err / bound:.3f}")
    again = _launch_decoder(A, W, b, lab, M_pad, m_valid, V)
    for x, y, what in zip((out, part[:m_valid], llog[:m_valid]), (again[0], again[1][:m_valid], again[2][:m_valid]),
                          ("out", "part", "llog")):
        assert torch.equal(_bits(x), _bits(y)), f"run-to-run: {what}"
    if m_valid < M_pad:
        A2 = A[:M_pad].clone()
        A2[m_valid:] = float("nan")
        nan_pad = _launch_decoder(A2, W, b, lab, M_pad, m_valid, V)[0]
        assert torch.equal(_bits(out), _bits(nan_pad)), "valid rows depend on the pad rows of A"
    assert err <= bound, (_dec_id(case), err, e32, bound)


@pytest.mark.parametrize("V,K", [(1000, 256), (1100, 256)])
def test_decoder_flat_is_bias_log_softmax(V, K):
    """A = 0: every row is b[label] - logsumexp(b[:V]), whatever the (poisoned) pad columns hold."""
    W, A, b, lab, lp, _, scale = _decoder_case("flat", V, K)
    out = _launch_decoder(A, W, b, lab, 256, 256, V)[0]
    want = torch.log_softmax(b[:V].double(), dim=0)[lab[:256].long()]
    assert (out.double() - want).abs().max().item() <= 4 * 2.0 ** -23 * scale[:256].max().item()


@pytest.mark.parametrize("V,K", [(1000, 256), (1100, 256)])
def test_decoder_out_of_range_label_is_minus_inf(V, K):
    """A label outside [0, V) — V, vpad - 1, vpad, vpad + 5, -1, -7, 2^31 - 1 — gives -inf for its row
    on every call (no stale label logit), and leaves the other rows bitwise what they are."""
    W, A, b, lab, _, _, _ = _decoder_case("plain", V, K)
    vpad = W.shape[0]
    base = _launch_decoder(A, W, b, lab, 256, 37, V)[0]
    bad = lab.clone()
    rows = [1, 5, 9, 13, 20, 29, 36]
    bad[rows] = torch.tensor([V, vpad - 1, vpad, vpad + 5, -1, -7, 2 ** 31 - 1], dtype=torch.int32, device="cuda")
    out = _launch_decoder(A, W, b, bad, 256, 37, V)[0]
    assert (out[rows] == float("-inf")).all(), out[rows]
    keep = [i for i in range(37) if i not in rows]
    assert torch.equal(_bits(out[keep]), _bits(base[keep]))


# ---- the out-of-range label through the product ------------------------------------------------

def _tiny():
    from asr_rescoring_amd.weights import BERT_TINY, make_weights
    return make_weights(BERT_TINY, seed=7), BERT_TINY


@pytest.fixture(scope="module")
def pll_tiny():
    from asr_rescoring_amd.scorer import PLLScorer
    w, shape = _tiny()
    s = PLLScorer(w, shape, device=0, max_rows=2048)
    yield s
    s.close()


def _mlm_batch(shape, n=6, T=9, seed=11):
    rng = np.random.default_rng(seed)
    ids = torch.from_numpy(rng.integers(106, shape.vocab, size=(n, T)).astype(np.int64))
    mp = rng.integers(1, T - 1, size=n)
    labels = ids.clone()
    for i, p in enumerate(mp):
        ids[i, p] = shape.mask_id
    return ids, torch.ones(n, T, dtype=torch.int64), labels, mp


@pytest.mark.parametrize("off", ["vpad", "vpad+5", "-7"])
def test_masked_logprob_label_out_of_range_fails(pll_tiny, off):
    """rs_masked_logprob after a valid batch, with one label of vpad, vpad + 5 or -7: RS_EUNSUP
    ("non-finite"), never the finite log-prob a stale label logit gives; deferred mode reports it too;
    the valid batch scores bitwise the same afterwards."""
    from asr_rescoring_amd._lib import RescoreError
    shape = pll_tiny.shape
    vpad = R.vocab_pad(shape.vocab)
    bad_label = {"vpad": vpad, "vpad+5": vpad + 5, "-7": -7}[off]
    ids, am, labels, mp = _mlm_batch(shape)
    good = pll_tiny.masked_logprob(ids, am, labels, mp).cpu()
    assert torch.isfinite(good).all()
    bad = labels.clone()
    bad[2, mp[2]] = bad_label
    with pytest.raises(RescoreError, match="non-finite"):
        pll_tiny.masked_logprob(ids, am, bad, mp)
    pll_tiny.set_sync_check(False)
    try:
        pll_tiny.masked_logprob(ids, am, labels, mp)
        pll_tiny.masked_logprob(ids, am, bad, mp)                # no exception: deferred
        with pytest.raises(RescoreError, match="non-finite"):
            pll_tiny.check()
        pll_tiny.check()                                         # cleared
    finally:
        pll_tiny.set_sync_check(True)
    assert torch.equal(pll_tiny.masked_logprob(ids, am, labels, mp).cpu(), good)


def test_pll_score_token_out_of_range_fails(pll_tiny):
    """rs_pll_score after a valid n-best, with a token id of vpad + 5 at a scored position: the
    embedding clamps the id, the label is not clamped — RS_EUNSUP, not a finite PLL."""
    from asr_rescoring_amd import data as D
    from asr_rescoring_amd._lib import RescoreError
    shape = pll_tiny.shape
    nb = D.synthetic_nbest(2, 3, seed=5, vocab=shape.vocab, len_lo=3, len_hi=12)
    good = pll_tiny.score_nbest(nb.tokens, nb.hyp_off).cpu()
    assert torch.isfinite(good).all()
    tok = np.array(nb.tokens, np.int32).copy()
    tok[int(nb.hyp_off[1]) + 1] = R.vocab_pad(shape.vocab) + 5
    with pytest.raises(RescoreError, match="non-finite"):
        pll_tiny.score_nbest(tok, nb.hyp_off)
    assert torch.equal(pll_tiny.score_nbest(nb.tokens, nb.hyp_off).cpu(), good)


@pytest.mark.parametrize("precision", ["fp16", "fp16x3"])
def test_pll_vocab_1100_runs_the_256x128_decoder_tile(precision):
    """A model whose decoder width (vpad = 1152) is no multiple of 256, end to end against the
    oracle, at the tolerance tests/test_gpu_bert.py test_edge_lengths holds the tiny model to."""
    from asr_rescoring_amd import data as D
    from asr_rescoring_amd.scorer import PLLScorer
    from asr_rescoring_amd.weights import BertShape, make_weights
    from oracle.bert_ref import TorchBert, pll_reference_pattern
    shape = BertShape(vocab=1100, hidden=256, layers=2, heads=4, intermediate=1024)
    assert R.decoder_tile(R.vocab_pad(shape.vocab)) == 128
    w = make_weights(shape, seed=7)
    rng = np.random.default_rng(0)
    hyps = [[rng.integers(106, shape.vocab, size=n).tolist() for n in (1, 9, 70)],
            [[shape.vocab - 1, 106, shape.vocab - 1], rng.integers(106, shape.vocab, size=5).tolist()]]
    nb = D.from_lists(hyps, [[0.0] * 3, [0.0] * 2])
    s = PLLScorer(w, shape, device=0, max_rows=2048, precision=precision)
    try:
        got = s.score(nb)
    finally:
        s.close()
    _, ref = pll_reference_pattern(TorchBert(w, shape), nb.tokens, nb.hyp_off, full_head=False)
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)
    print(f"PLL vocab 1100 {precision}: max rel err {rel.max():.3e}")
    assert rel.max() < 1e-3
