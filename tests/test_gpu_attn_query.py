"""GPU: attn_query_kernel, the last layer's attention over the scored row of every sequence,
through the production launcher (rs_debug_attention_query -> launch_attention_query), against
float64.

One launch covers sequences [s0, s1) = [2, 11) of a 12-sequence metadata array: T = 1, 2, 3, 63, 64,
65, 128, 129, 512 (one key, the 64-key block edge, the online softmax over two to eight blocks), gaps
between the row ranges, query = 0, T - 1 or interior, every row of every buffer with contents of its
own.  All per-sequence buffers (qd, ctxq, resq) have one row per sequence of the WHOLE array and
the rows past s1 - s0 must keep their sentinel: an index by s where s - s0 is meant lands there.
Crossed: fp16 QKV with the kx = 1 image / fp32 QKV with the three-part image; qd null / dense (the
Q columns of qkv then hold other values); the residual from (x32, stats, g, b) / from the two-part
image; H 256 / 768; the plain and the peaked family (tail_ref.attn_operands).

Reference: float64 softmax(q.K^T / 8).V per head on the values held; yardstick e32: the same in
torch fp32.  Asserted: err <= 4 max(e32, q), q = 2^-10 max|y| (kx = 1) or 2^-21 max|y| (kx = 3, after
the exact checks of the image alone, tail_ref.image3_defects).  resq from the image: hi + lo/64
bitwise (exact in fp32).  resq from the statistics: within 4 * 2^-23 max|y| of ln_apply's expression
((x - mean) rstd) g + b in float64 on the fp32 inputs given.

Measured on MI355X, every case at or below 0.07 of its bound:
    fp32 QKV, kx = 3, plain:  err / e32 0.96 .. 1.99 (H 768), 1.07 .. 1.99 (H 256); err <= 1.8e-7
    fp32 QKV, kx = 3, peaked: e32 = 0 (the softmax is one-hot to e^-80 in fp32 as in float64), err
                              1.2e-7 .. 2.4e-7 = at most 0.06 of the image's 4 * 2^-21 max|y|
    fp16 QKV, kx = 1, plain:  err 4.0e-4 .. 4.9e-4, the fp16 rounding of the output (e32 ~ 1e-7)
    fp16 QKV, kx = 1, peaked: err 0 (the output is the planted key's fp16 V row)
    resq from the statistics: 0.12 .. 0.20 of 4 * 2^-23 max|y|; from the image: bitwise.
One or two elements of a kx = 3 launch hold an exact tie (lo/64 rounded up to half a spacing of hi);
tail_ref.image3_defects accepts hi there, and only there, as the other nearest fp16 number.
With ctxq indexed by s where s - s0 is meant (a scratch build, not kept) all 32 cases fail: rows
past s1 - s0 are written.
"""
import pytest
import torch

from asr_rescoring_amd import _lib
import tail_ref as R
from x3s_image import _unsplit2

pytestmark = pytest.mark.gpu

SENT32, SENT16 = 0x7FC12345, 0x7E5A
CASES = [(H, heads, q32, dense, img, fam)
         for H, heads in ((256, 4), (768, 12)) for q32 in (False, True) for dense in (False, True)
         for img in (False, True) for fam in ("plain", "peaked")]


def _id(c):
    H, heads, q32, dense, img, fam = c
    return f"H{H}-{'f32kx3' if q32 else 'f16kx1'}-{'qd' if dense else 'qrow'}-{'himg' if img else 'stats'}-{fam}"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(qkv, qd_all, res, layout, H, heads, q32, kx, img):
    T, row, query, s0, s1, rows = layout
    n_seq = T.numel()
    d = lambda t: t.cuda().contiguous()
    dT, drow, dq = d(T), d(row), d(query)
    ctxq = torch.full((n_seq, kx * H), SENT16, dtype=torch.int16, device="cuda").view(torch.float16)
    resq = torch.full((n_seq, H), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    p = lambda t: None if t is None else t.data_ptr()
    use = (None, None, None, None, res["himg"]) if img else (res["x32"], res["stats"], res["g"], res["b"], None)
    rc = _lib.load().rs_debug_attention_query(qkv.data_ptr(), int(q32), dT.data_ptr(), drow.data_ptr(), dq.data_ptr(),
                                              s0, s1, 0, H, heads, kx, p(qd_all), *[p(t) for t in use],
                                              ctxq.data_ptr(), resq.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ctxq, resq


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_attn_query_vs_float64(case):
    H, heads, q32, dense, img, fam = case
    kx = 3 if q32 else 1
    layout = R.attn_layout()
    T, row, query, s0, s1, rows = layout
    n, n_seq = s1 - s0, T.numel()
    seed = H + 2 * q32 + 4 * dense + 8 * img + 16 * (fam == "peaked")
    qkv, qd, q = R.attn_operands(fam, H, q32, dense, layout, seed=seed, device="cuda")
    res = R.attn_residual_operands(rows, H, seed=seed, device="cuda")
    ref = R.attn_query_ref(qkv, q, layout, H, heads, torch.float64)
    e32 = (R.attn_query_ref(qkv, q, layout, H, heads, torch.float32).double() - ref).abs().max().item()
    dt = torch.float32 if q32 else torch.float16
    qkv_d = qkv.to(dt).contiguous()
    assert torch.equal(qkv_d.float(), qkv)                     # the kernel's operands hold the reference's values
    qd_all = None
    if dense:
        # rows [0, n): the launch's Q; rows [n, n_seq): other distinct rows (never read)
        qd_all = torch.cat([qd, qd[:n_seq - n] * -0.5 + 3.0]).to(dt).contiguous()
    ctxq, resq = _run(qkv_d, qd_all, res, layout, H, heads, q32, kx, img)
    assert (_bits(ctxq[n:]) == SENT16).all() and (_bits(resq[n:]) == SENT32).all(), "rows past s1 - s0 written"
    got = ctxq[:n]
    if kx == 3:
        assert R.image3_defects(got) == []
        val, qz = R._unsplit3(got, torch.float64), 2.0 ** -21
    else:
        val, qz = got.double(), 2.0 ** -10
    assert torch.isfinite(val).all()
    err_s = (val - ref).abs().max(dim=1).values
    err = err_s.max().item()
    bound = 4 * max(e32, qz * ref.abs().max().item())
    print(f"ATTNQ {_id(case)}: err {err:.3e} (T of the worst sequence {int(T[s0 + int(err_s.argmax())])}) e32 {e32:.3e} "
          f"err/e32 {err / max(e32, 1e-300):.2f} err/bound {err / bound:.3f}")
    # the residual of the scored row
    qrow = (row[s0:s1] + query[s0:s1]).long().cuda()
    if img:
        want = _unsplit2(res["himg"][qrow], torch.float64)
        assert torch.equal(resq[:n].double(), want), "resq != hi + lo/64 of the scored row's image"
    else:
        want = R.ln_apply(res["x32"][qrow], res["stats"][qrow], res["g"], res["b"], torch.float64)
        rerr = (resq[:n].double() - want).abs().max().item()
        rbound = 4 * 2.0 ** -23 * want.abs().max().item()
        print(f"ATTNQ {_id(case)}: resq err {rerr:.3e} err/bound {rerr / rbound:.3f}")
        assert rerr <= rbound, (rerr, rbound)
    again = _run(qkv_d, qd_all, res, layout, H, heads, q32, kx, img)
    assert torch.equal(_bits(ctxq), _bits(again[0])) and torch.equal(_bits(resq), _bits(again[1])), "run-to-run"
    assert err <= bound, (_id(case), err, e32, bound)


def test_attention_query_rejects_bad_arguments():
    """The entry's argument checks (no kernel runs)."""
    layout = R.attn_layout()
    T, row, query, s0, s1, rows = layout
    qkv = torch.zeros(rows, 3 * 256, device="cuda")
    res = R.attn_residual_operands(rows, 256, device="cuda")
    out = torch.zeros(T.numel(), 3 * 256, device="cuda")
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    dT, drow, dq = T.cuda(), row.cuda(), query.cuda()

    def call(kx=3, H=256, heads=4, s1_=s1, x32=res["x32"].data_ptr(), himg=None, qry=dq.data_ptr()):
        return lib.rs_debug_attention_query(qkv.data_ptr(), 1, dT.data_ptr(), drow.data_ptr(), qry, s0, s1_, 0, H, heads,
                                            kx, None, x32, res["stats"].data_ptr(), res["g"].data_ptr(),
                                            res["b"].data_ptr(), himg, out.data_ptr(), out.data_ptr(), st)
    assert call(kx=2) != 0
    assert call(H=256, heads=3) != 0
    assert call(s1_=s0) != 0
    assert call(x32=None) != 0                                  # neither residual source
    assert call(qry=None) != 0
    torch.cuda.synchronize()
    assert not out.any()
