"""GPU: the fused residual + LayerNorm epilogue of the split-operand GEMM
(gemm_x3s_kernel<EPI_LNRES_IMG>, O-projection and BertOutput of the fp16x3 path) through the
rs_debug_x3s entry, i.e. through the production launcher, against a float64 LayerNorm.

Reference (tests/x3s_image.py): on the values the images hold,
    x = unsplit(A2) . unsplit(W2)^T + b + unsplit(h2),   y = LN(x; gamma, beta, 1e-12)   in float64,
compared with unsplit(out) on rows < m_valid.  Yardstick: the same expression in torch fp32 (fp32
matmul, F.layer_norm), e32 = its max |error| against float64.  Asserted per case:
    err <= 4 max(e32, 2^-21 max|y|)
(4: another summation order and the dropped lo.lo product; 2^-21 max|y|: twice the output image's
own 2^-22 quantisation).

Covered: one / two / three / four column tiles (no peers .. three peers), both K instances
(K <= 1024 and K > 1024), m_valid 1 / 255 / 256 / 300, more row panels than gangs (a second
round and the list hand-over), and input families where a wrong cross-tile combination
m2 = sum_c (M2_c + 256 (mean_c - mean)^2), a swapped tile, a wrong 1/H or a permuted gamma / beta
moves the output by far more than the bound (x3s_image.lnres_operands).  Bitwise: repeat runs,
RS_LNGANG=ticket vs the default, independence of rows < m_valid from the pad rows, constant rows
-> split2(beta) exactly.  Every launch leaves lnerr == 0 and lncnt all zero; all launches of
this module share one lnx / lncnt / lnerr, never re-zeroed, as the scorer's launches do.

Measured err / e32 on MI355X (family plain unless named; m_valid 1 / 255 / 256 / 300 of M_pad 512 /
the two-round case), every case at or below 0.29 of its bound:
    N  768 K  768   0.69  0.67  0.67  0.72  0.69      N  256 K 256   0.83  0.59  0.59  0.53
    N  768 K 3072   0.47  0.61  0.61  0.60  0.76      N  512 K 256   0.60  0.90  0.90  0.61
    N 1024 K  256   0.56  0.76  0.76  0.71  0.68
    families at N 768 K 768 M_pad 512:  plain 0.69  offset 1.01  tile_means 0.97  distinct_affine 0.49
             constant: bitwise image(beta) (e32 is meaningless there: torch's fp32 LayerNorm
             leaves a rounding-level variance, which 1 / sqrt(1e-12) turns into a 4e-2 error)
    families at N 1024 K 256 M_pad 512: plain 0.68  offset 1.15  tile_means 1.37
So the kernel is as accurate as the fp32 evaluation everywhere; nothing needed the factor 4.
With the between-tile term 256 (mean_c - mean)^2 dropped from m2, or the row total formed from
the workgroup's own tile only (scratch builds, not kept), every case with more than one column tile
fails — plain by 1e3 .. 1e4 times the bound, offset by 18 .. 630, tile_means by 5e5 .. 1e7 — while
the one-tile shape and the constant family, which do not depend on either term, pass.
"""
import ctypes

import pytest
import torch

from asr_rescoring_amd import _lib
from x3s_image import LN_EPS, _split2, _unsplit2, lnres_operands, lnres_ref32, lnres_ref64

pytestmark = pytest.mark.gpu

EPI_LNRES_IMG = 7
SHAPES = [(768, 768), (768, 3072), (256, 256), (512, 256), (1024, 256)]      # (N, K)
ROWS = [(256, 1), (256, 255), (256, 256), (512, 300)]                         # (M_pad, m_valid)
# M_pad None: 256 (gangs + 2) row panels, gangs = workgroups(N) / (N / 256)
CASES = [("plain", N, K, mp, mv) for N, K in SHAPES for mp, mv in ROWS] + \
        [("plain", 768, 768, None, None), ("plain", 768, 3072, None, None), ("plain", 1024, 256, None, None)]
FAMILY_CASES = [(f, 768, 768, 512, 512) for f in ("plain", "offset", "tile_means", "constant", "distinct_affine")] + \
               [(f, 1024, 256, 512, 512) for f in ("plain", "offset", "tile_means")]
PAD_CASES = [("plain", N, K, mp, mv) for N, K in SHAPES for mp, mv in ROWS if mv < mp]


def _id(c):
    f, N, K, mp, mv = c
    return f"{f}-N{N}-K{K}-" + ("rounds" if mp is None else f"M{mp}-v{mv}")


def _sizes(M_pad, N):
    out = (ctypes.c_int64 * 3)()
    assert _lib.load().rs_debug_lnres_sizes(M_pad, N, out) == 0
    return int(out[0]), int(out[1]), int(out[2])


def _rows(case):
    f, N, K, mp, mv = case
    if mp is None:
        gangs = _sizes(256, N)[2] // (N // 256)
        mp = 256 * (gangs + 2)
        mv = mp - 3
    return mp, mv


class _Bufs:
    """lnx / lncnt / lnerr of every launch of this module: zeroed once, grown (and zeroed) only when
    a case needs more granules."""

    def __init__(self):
        self.lnx = None
        self.lncnt = torch.zeros(_sizes(256, 256)[1] // 4, dtype=torch.int32, device="cuda")
        self.lnerr = torch.zeros(4, dtype=torch.int32, device="cuda")

    def ensure(self, M_pad, N):
        need = _sizes(M_pad, N)[0]
        if self.lnx is None or self.lnx.numel() * 8 < need:
            self.lnx = torch.zeros((need + 7) // 8, dtype=torch.int64, device="cuda")


@pytest.fixture(scope="module")
def bufs():
    b = _Bufs()
    b.ensure(256 * 90, 1024)
    return b


def _launch(bufs, op, N, K, M_pad, m_valid, A2=None, h2=None):
    """One launch on a copy of the residual image; asserts the launch's postconditions."""
    A2 = op["A2"] if A2 is None else A2
    out = (op["h2"] if h2 is None else h2).clone()
    assert A2.shape == (M_pad, 2 * K) and op["W2"].shape == (N, 2 * K) and out.shape == (M_pad, 2 * N)
    assert A2.is_contiguous() and op["W2"].is_contiguous() and out.is_contiguous()
    bufs.ensure(M_pad, N)
    rc = _lib.load().rs_debug_x3s(EPI_LNRES_IMG, A2.data_ptr(), op["W2"].data_ptr(), op["b"].data_ptr(),
                                  op["g"].data_ptr(), op["beta"].data_ptr(), LN_EPS, out.data_ptr(), 2 * N, M_pad, m_valid,
                                  N, K, bufs.lnx.data_ptr(), bufs.lncnt.data_ptr(), bufs.lnerr.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(bufs.lnerr[0].item()) == 0, "a statistics or gang wait timed out"
    # common.h: lncnt (ticket words and gang slots) is "left zeroed by every launch"
    nz = bufs.lncnt.nonzero().flatten()
    assert nz.numel() == 0, f"{nz.numel()} non-zero words in lncnt, first at word {int(nz[0])}"
    return out


_cache = {}


def _case(case):
    """Operands (device), and for the small cases the float64 reference and the fp32 yardstick,
    computed once per case and never modified."""
    f, N, K, _, _ = case
    M_pad, m_valid = _rows(case)
    if case in _cache:
        return _cache[case]
    op = lnres_operands(f, M_pad, N, K, seed=1000 + len(f) + N + K + M_pad, device="cuda")
    y = lnres_ref64(op["A2"], op["W2"], op["b"], op["h2"], op["g"], op["beta"])[:m_valid]
    y32 = lnres_ref32(op["A2"], op["W2"], op["b"], op["h2"], op["g"], op["beta"])[:m_valid]
    e32 = (y32.double() - y).abs().max().item()
    ent = (op, y, e32, M_pad, m_valid)
    if M_pad <= 512:
        _cache[case] = ent
    return ent


def _check(name, out, y, e32, m_valid):
    got = _unsplit2(out[:m_valid], torch.float64)
    assert torch.isfinite(got).all(), name
    err = (got - y).abs().max().item()
    bound = 4 * max(e32, 2.0 ** -21 * y.abs().max().item())
    print(f"LNRES {name}: err {err:.3e} e32 {e32:.3e} err/e32 {err / max(e32, 1e-300):.2f} err/bound {err / bound:.3f}")
    assert err <= bound, (name, err, e32, bound)


@pytest.mark.parametrize("case", CASES + FAMILY_CASES, ids=_id)
def test_lnres_vs_float64(bufs, case, monkeypatch):
    """Parity with the float64 LayerNorm, two equal runs, and RS_LNGANG=ticket equal to the default."""
    f, N, K, _, _ = case
    op, y, e32, M_pad, m_valid = _case(case)
    monkeypatch.delenv("RS_LNGANG", raising=False)
    out = _launch(bufs, op, N, K, M_pad, m_valid)
    _check(_id(case), out, y, e32, m_valid)
    if f == "constant":
        # variance exactly 0: (x - mean) rstd = 0 exactly, the output is image(beta) on every row
        want = _split2(op["beta"].view(1, N)).expand(M_pad, 2 * N)
        assert torch.equal(out.view(torch.int16), want.contiguous().view(torch.int16))
    again = _launch(bufs, op, N, K, M_pad, m_valid)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "run-to-run"
    monkeypatch.setenv("RS_LNGANG", "ticket")
    tick = _launch(bufs, op, N, K, M_pad, m_valid)
    assert torch.equal(out.view(torch.int16), tick.view(torch.int16)), "RS_LNGANG=ticket vs default"


@pytest.mark.parametrize("case", PAD_CASES, ids=_id)
def test_lnres_valid_rows_ignore_pad_rows(bufs, case, monkeypatch):
    """Rows < m_valid are bitwise the same whether the pad rows of A2 and h2 hold zeros or hi parts
    of 6.0e4 (nothing is asserted about the pad rows: the kernel stores whole 256-row panels)."""
    f, N, K, _, _ = case
    op, _, _, M_pad, m_valid = _case(case)
    monkeypatch.delenv("RS_LNGANG", raising=False)
    outs = []
    for fill in (0.0, 6.0e4):
        A2, h2 = op["A2"].clone(), op["h2"].clone()
        for img in (A2, h2):
            pad = img[m_valid:].view(M_pad - m_valid, -1, 2, 32)
            pad.zero_()
            pad[:, :, 0] = fill                                     # hi parts; lo parts 0
        outs.append(_launch(bufs, op, N, K, M_pad, m_valid, A2=A2, h2=h2)[:m_valid])
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_lnres_buffer_reuse_across_instances(bufs, monkeypatch):
    """The O-projection (K = 768) and then the BertOutput (K = 3072) instance on the same lnx /
    lncnt / lnerr without re-zeroing, as every layer of the scorer runs them: both meet the
    tolerance, and each leaves lnerr == 0 and every word of lncnt zero (_launch, after every launch
    of this module).  (Until this test existed the last workgroup re-zeroed only the ticket words:
    328 of the 2816 words, all gang slots, stayed non-zero — harmless while the slots' launch tags
    are unique, but not what common.h promises the owner of the buffer; lnr_done now zeroes both.)"""
    monkeypatch.delenv("RS_LNGANG", raising=False)
    for rep in range(2):
        for case in (("plain", 768, 768, 512, 300), ("plain", 768, 3072, 512, 300)):
            op, y, e32, M_pad, m_valid = _case(case)
            out = _launch(bufs, op, case[1], case[2], M_pad, m_valid)
            _check(f"reuse{rep}-" + _id(case), out, y, e32, m_valid)


def test_lnres_rejects_bad_arguments(bufs):
    """The launcher's argument checks (no kernel runs): missing buffers, a residual image that is
    not [M_pad, 2N], more than four column tiles."""
    op, _, _, M_pad, m_valid = _case(("plain", 256, 256, 256, 256))
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = op["h2"].clone()

    def call(ldc=512, N=256, lnx=None):
        lnx = bufs.lnx.data_ptr() if lnx is None else lnx
        return lib.rs_debug_x3s(EPI_LNRES_IMG, op["A2"].data_ptr(), op["W2"].data_ptr(), op["b"].data_ptr(),
                                op["g"].data_ptr(), op["beta"].data_ptr(), LN_EPS, out.data_ptr(), ldc, 256, 256, N, 256,
                                lnx, bufs.lncnt.data_ptr(), bufs.lnerr.data_ptr(), st)
    assert call(lnx=0) != 0
    assert call(ldc=1024) != 0
    assert call(N=1280, ldc=2560) != 0
    torch.cuda.synchronize()
    assert torch.equal(out, op["h2"])
