"""GPU: the attention kernels layer 0 of every default MLM call runs — the DEDUP = true instantiations
attn16x3v2_kernel<true, 48>, <true, 64>, attn16_kernel<true>, attn_tr_kernel<true> — and the multi-query tail
attn_mquery_kernel, through the production launchers (rs_debug_attention_plan -> launch_attention_full,
rs_debug_attention_mquery -> launch_attention_mquery).  Layouts, operands, references: tests/front_ref.py.

Dedup.  The chunk of front_ref.dedup_chunk (a PLL run, a run cut at the chunk start with absent copies,
overlapping wide spans, a one-copy run, T = 3; T in {3, 16, 17, 33, 48} under max_len 48, + 49 and 64 under 64,
+ 65 and 130 for the fp16 kernels), launched over [s0, s1) with s0 = 2, the outside sequences poisoned.
qkv_u [pad_to(urows, 256) + 8, 3H] holds contents of its own on every unique row (flat 0.6 randn, and the
peaked family of test_gpu_attention._peaked); qkv_full is qkv_u gathered through the layout, one row per
(s, t), gaps between the ranges.  Asserted: the dedup = 1 launch on qkv_u (row0 = 0) and the dedup = 0 launch
on qkv_full (row0 = 5) give BITWISE equal ctx rows — same kernel arithmetic, only SeqRows' addressing
differs — and every other ctx row keeps its sentinel; the dedup = 0 result is within the bounds
test_gpu_attention.py asserts: fp32 -> kx = 2 image 2e-6 (flat) / 4 e32 (peaked), fp16 -> kx = 1
2^-10 max(1, max|v|) per (sequence, head).  H in {256, 768}.  Rejected with ctx untouched: fp32 dedup with
max_len 65, dedup with the other type's kx, H != 64 heads.

Multi-query.  tail_ref.attn_layout's array launched over [2, 11) (T = 1, 2, 3, 63, 64, 65, 128, 129, 512), 1, 2,
3, 4, 5, 8, 9 queries per sequence with 0 and T - 1, q0 = first[s0] != 0, ctxq / resq one sentinel row per query
of the whole list; crossed as test_gpu_attn_query.py.  Asserted: every query's ctxq and resq BITWISE those of
rs_debug_attention_query with query = pos (one launch per query rank), rows outside [q0, q0 + nq) keep the
sentinel, the float64 bound of test_gpu_attn_query.py on the multi-query output, two runs bitwise equal.

Measured on MI355X (every bit equality held in all 20 + 32 cases):
    dedup = 0, fp32 -> kx 2, flat:    err 1.5e-7 .. 2.3e-7, e32 1.4e-7 .. 1.5e-7, err / e32 1.11 .. 1.55
    dedup = 0, fp32 -> kx 2, peaked:  err 1.7e-6 .. 4.5e-6, e32 3.8e-6 .. 1.3e-5, err / e32 0.28 .. 0.67
    dedup = 0, fp16 -> kx 1:          0.21 .. 0.30 (flat), 0.29 .. 0.45 (peaked) of 2^-10 max(1, max|v|)
    mquery, fp32, kx 3, plain:   err 1.5e-7 .. 3.2e-7, err / e32 1.07 .. 2.56, 0.04 .. 0.09 of the bound
    mquery, fp32, kx 3, peaked:  err 4.3e-6 .. 7.9e-6, err / e32 0.86 .. 1.68, 0.22 .. 0.42 of the bound
    mquery, fp16, kx 1:          err 4.1e-4 .. 9.7e-4, the fp16 rounding of the output, 0.05 .. 0.11 of the bound
Scratch builds (not kept; each reads and writes only inside the over-sized buffers) and the cases that
fail on them:
    SeqRows taking `base` for the last position of a span: all 20 dedup cases (523 .. 1940 ctx rows differ);
    attn_mquery storing at q - qa instead of q - q0: all 32 multi-query cases (the sequences' rows collide, so
        already two runs differ).
"""
import ctypes

import pytest
import torch

from asr_rescoring_amd import _lib
import front_ref as F
import tail_ref as R
from x3s_image import _unsplit2

pytestmark = pytest.mark.gpu

SENT32, SENT16 = 0x7FC12345, 0x7E5A
ROW0 = 5


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _sent16(rows, cols):
    return torch.full((rows, cols), SENT16, dtype=torch.int16, device="cuda").view(torch.float16)


def _plan(qkv, q32, meta, s0, s1, row0, max_len, H, heads, kx, dedup, ctx):
    dm, keep = F.meta_struct(meta)
    rc = _lib.load().rs_debug_attention_plan(_p(qkv), int(q32), ctypes.addressof(dm), s0, s1, row0, max_len, H, heads, kx,
                                             int(dedup), _p(ctx), _stream())
    torch.cuda.synchronize()
    return rc


DEDUP_CASES = [(H, heads, q32, max_len, fam)
               for H, heads in ((256, 4), (768, 12)) for q32, lens in ((True, (48, 64)), (False, (48, 64, 130)))
               for max_len in lens for fam in ("flat", "peaked")]


def _did(c):
    H, heads, q32, max_len, fam = c
    return f"H{H}-{'f32kx2' if q32 else 'f16kx1'}-L{max_len}-{fam}"


def _chunk_operands(fam, ch, H, q32, seed):
    """qkv_u [alloc, 3H] and qkv_full [ROW0 + rows, 3H] (absolute rows; other contents in the gaps) in the
    kernel's type, and the float32 tensor of the values qkv_full holds."""
    alloc = F.pad_to(ch["urows"], 256) + 8
    qkv_u = F.unique_qkv(fam, ch, H, alloc, seed=seed, device="cuda")
    dt = torch.float32 if q32 else torch.float16
    qkv_u = qkv_u.to(dt).contiguous()
    urow, _, _ = F.unique_map(ch)
    own, _, _ = F.launch_rows(ch["meta"], ch["s0"], ch["s1"], 0)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    full = (torch.randn(ROW0 + ch["rows"], 3 * H, device="cuda", generator=g) * 0.6).to(dt)
    full[own.cuda()] = qkv_u[urow.cuda()]
    return qkv_u, full.contiguous(), own


@pytest.mark.parametrize("case", DEDUP_CASES, ids=_did)
def test_dedup_attention_is_materialised_attention(case):
    H, heads, q32, max_len, fam = case
    kx = 2 if q32 else 1
    ch = F.dedup_chunk(F.RUNS[max_len], row0=ROW0)
    m, s0, s1 = ch["meta"], ch["s0"], ch["s1"]
    assert int(m["len"][s0:s1].max()) == max_len
    qkv_u, full, own = _chunk_operands(fam, ch, H, q32, seed=H + max_len + 7 * q32)
    rows_a = ROW0 + ch["rows"]
    ctx_a, ctx_b = _sent16(rows_a, kx * H), _sent16(ch["rows"], kx * H)
    assert _plan(qkv_u, q32, m, s0, s1, 0, max_len, H, heads, kx, True, ctx_a) == 0
    assert _plan(full[ROW0:], q32, m, s0, s1, ROW0, max_len, H, heads, kx, False, ctx_b) == 0
    own_a, own_b = own.cuda(), (own - ROW0).cuda()
    for ctx, idx, name in ((ctx_a, own_a, "dedup"), (ctx_b, own_b, "materialised")):
        keep = torch.ones(ctx.shape[0], dtype=torch.bool, device="cuda")
        keep[idx] = False
        assert (_bits(ctx)[keep] == SENT16).all(), f"{name}: a ctx row outside the launch was written"
    a, b = _bits(ctx_a[own_a]), _bits(ctx_b[own_b])
    if not torch.equal(a, b):
        bad = torch.nonzero((a != b).any(dim=1))[:, 0].cpu()
        _, ss, ts = F.launch_rows(m, s0, s1, 0)
        raise AssertionError(f"{len(bad)} ctx rows differ between dedup and materialised rows; first (s, t): "
                             f"{[(int(ss[i]), int(ts[i])) for i in bad[:6]]}")
    # the materialised launch (s0 != 0, row0 != 0) against float64
    T, row = m["len"][s0:s1], m["row"][s0:s1]
    held = full.float()
    ref = torch.cat(F.attn_rows_ref(held, T, row, H, heads, torch.float64))
    got = ctx_b[own_b]
    if q32:
        assert F.image2_defects(got) == []
        val = _unsplit2(got, torch.float64)
        assert torch.isfinite(val).all()
        e32 = (torch.cat(F.attn_rows_ref(held, T, row, H, heads, torch.float32)).double() - ref).abs().max().item()
        err = (val - ref).abs().max().item()
        print(f"PLAN {_did(case)}: err {err:.3e} e32 {e32:.3e} err/e32 {err / max(e32, 1e-300):.2f}")
        if fam == "flat":
            assert err < 2e-6, (err, e32)
        else:
            assert err <= 4 * e32, (err, e32)
    else:
        val = got.double()
        assert torch.isfinite(val).all()
        worst, n = 0.0, 0
        for r0, t in zip(row.tolist(), T.tolist()):
            err = (val[n:n + t] - ref[n:n + t]).abs().view(t, heads, 64).amax(dim=(0, 2))
            vmax = held[r0:r0 + t, 2 * H:].double().abs().view(t, heads, 64).amax(dim=(0, 2))
            worst = max(worst, (err / (2.0 ** -10 * vmax.clamp_min(1.0))).max().item())
            n += t
        print(f"PLAN {_did(case)}: worst err / bound {worst:.3f}")
        assert worst <= 1.0, worst


def test_attention_plan_rejections():
    """The launcher's and the entry's rejections: an error, and ctx untouched."""
    H, heads = 256, 4
    ch = F.dedup_chunk(F.RUNS[130], row0=0)
    m, s0, s1 = ch["meta"], ch["s0"], ch["s1"]
    alloc = F.pad_to(ch["urows"], 256) + 8
    q32 = torch.zeros(alloc, 3 * H, device="cuda")
    q16 = q32.half()
    ctx = _sent16(ch["rows"], 3 * H)
    assert _plan(q32, True, m, s0, s1, 0, 65, H, heads, 2, True, ctx) != 0          # fp32 dedup past one key block
    assert _plan(q32, True, m, s0, s1, 0, 48, H, heads, 3, True, ctx) != 0          # dedup, the other form's kx
    assert _plan(q32, True, m, s0, s1, 0, 48, H, heads, 1, True, ctx) != 0
    assert _plan(q16, False, m, s0, s1, 0, 48, H, heads, 2, True, ctx) != 0
    assert _plan(q16, False, m, s0, s1, 0, 48, H, 3, 1, True, ctx) != 0             # H != 64 heads
    assert _plan(q16, False, m, s0, s1, 0, 48, H, heads, 4, False, ctx) != 0        # no such image
    assert _plan(q16, False, m, s1, s1, 0, 48, H, heads, 1, False, ctx) != 0        # s1 <= s0
    assert _plan(q16, False, m, s0, s1, 0, 0, H, heads, 1, False, ctx) != 0         # no max_len
    assert _plan(None, False, m, s0, s1, 0, 48, H, heads, 1, False, ctx) != 0
    assert _plan(q16, False, dict(m, urow_m=None), s0, s1, 0, 48, H, heads, 1, True, ctx) != 0
    assert (_bits(ctx) == SENT16).all()


# ---- multi-query attention -----------------------------------------------------------------------------

MQ_CASES = [(H, heads, q32, dense, img, fam)
            for H, heads in ((256, 4), (768, 12)) for q32 in (False, True) for dense in (False, True)
            for img in (False, True) for fam in ("plain", "peaked")]


def _mid(c):
    H, heads, q32, dense, img, fam = c
    return f"H{H}-{'f32kx3' if q32 else 'f16kx1'}-{'qd' if dense else 'qrow'}-{'himg' if img else 'stats'}-{fam}"


def _res_args(res, img):
    use = (None, None, None, None, res["himg"]) if img else (res["x32"], res["stats"], res["g"], res["b"], None)
    return [_p(t) for t in use]


def _mquery(qkv, q32, meta, s0, s1, H, heads, kx, qd, res, img, n_rows):
    dm, keep = F.meta_struct(meta)
    ctxq = _sent16(n_rows, kx * H)
    resq = torch.full((n_rows, H), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    rc = _lib.load().rs_debug_attention_mquery(qkv.data_ptr(), int(q32), ctypes.addressof(dm), s0, s1, H, heads, kx, _p(qd),
                                               *_res_args(res, img), ctxq.data_ptr(), resq.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ctxq, resq


def _query(qkv, q32, T, row, query, s0, s1, H, heads, kx, qd, res, img):
    d = [t.cuda().contiguous() for t in (T, row, query)]
    ctxq = _sent16(T.numel(), kx * H)
    resq = torch.full((T.numel(), H), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    rc = _lib.load().rs_debug_attention_query(qkv.data_ptr(), int(q32), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                              s0, s1, 0, H, heads, kx, _p(qd), *_res_args(res, img), ctxq.data_ptr(),
                                              resq.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ctxq, resq


@pytest.mark.parametrize("case", MQ_CASES, ids=_mid)
def test_mquery_is_attn_query_per_query(case):
    H, heads, q32, dense, img, fam = case
    kx = 3 if q32 else 1
    base = R.attn_layout()
    T, row, _, s0, s1, rows = base
    first, seq, pos = F.mquery_lists(base)
    n, nq_all = s1 - s0, pos.numel()
    q0, nq = int(first[s0]), int(first[s1] - first[s0])
    assert q0 != 0 and q0 + nq < nq_all
    seed = H + 2 * q32 + 4 * dense + 8 * img + 16 * (fam == "peaked")
    # the peaked family plants its key for every sequence's second list position (the last of a shorter list)
    qkv, _, _ = R.attn_operands(fam, H, q32, False, (T, row, F.rank_queries(first, pos, 1), s0, s1, rows), seed=seed,
                                device="cuda")
    qrow = (row[seq.long()] + pos).long().cuda()
    q_all = qkv[qrow, :H].clone()                                  # the Q of every query of the whole list
    if dense:
        qkv[qrow, :H] = -q_all - 1.0                               # the Q columns of qkv hold other values
        if not q32:
            qkv = qkv.half().float()
    res = R.attn_residual_operands(rows, H, seed=seed, device="cuda")
    dt = torch.float32 if q32 else torch.float16
    qkv_d = qkv.to(dt).contiguous()
    assert torch.equal(qkv_d.float(), qkv)
    qd = None
    if dense:
        # rows [0, nq): the launch's queries; then the other queries' rows (never read)
        qd = torch.cat([q_all[q0:q0 + nq], q_all[:q0], q_all[q0 + nq:]]).to(dt).contiguous()
    meta = {"len": T, "row": row, "first": first, "seq": seq, "pos": pos}
    ctxq, resq = _mquery(qkv_d, q32, meta, s0, s1, H, heads, kx, qd, res, img, nq_all)
    assert (_bits(ctxq[nq:]) == SENT16).all() and (_bits(resq[nq:]) == SENT32).all(), "rows past q0 + nq written"
    again = _mquery(qkv_d, q32, meta, s0, s1, H, heads, kx, qd, res, img, nq_all)
    assert torch.equal(_bits(ctxq), _bits(again[0])) and torch.equal(_bits(resq), _bits(again[1])), "run-to-run"
    ref = torch.empty(nq, H, dtype=torch.float64, device="cuda")
    r32 = torch.empty(nq, H, dtype=torch.float32, device="cuda")
    counts = [int(first[s + 1] - first[s]) for s in range(s0, s1)]
    done = 0
    for r in range(max(counts)):
        qr = F.rank_queries(first, pos, r)
        ql = torch.tensor([int(first[s]) + min(r, c - 1) for s, c in zip(range(s0, s1), counts)])
        q_r = q_all[ql.cuda()]
        one_c, one_r = _query(qkv_d, q32, T, row, qr, s0, s1, H, heads, kx, q_r.to(dt).contiguous() if dense else None, res, img)
        lay = (T, row, qr, s0, s1, rows)
        ref_r = R.attn_query_ref(qkv, q_r, lay, H, heads, torch.float64)
        r32_r = R.attn_query_ref(qkv, q_r, lay, H, heads, torch.float32)
        for i, c in enumerate(counts):
            if r >= c:
                continue
            j = int(ql[i]) - q0
            assert torch.equal(_bits(ctxq[j]), _bits(one_c[i])), f"ctxq of query {j + q0} (sequence {s0 + i}, rank {r})"
            assert torch.equal(_bits(resq[j]), _bits(one_r[i])), f"resq of query {j + q0} (sequence {s0 + i}, rank {r})"
            ref[j], r32[j] = ref_r[i], r32_r[i]
            done += 1
    assert done == nq
    got = ctxq[:nq]
    if kx == 3:
        assert R.image3_defects(got) == []
        val, qz = R._unsplit3(got, torch.float64), 2.0 ** -21
    else:
        val, qz = got.double(), 2.0 ** -10
    assert torch.isfinite(val).all()
    e32 = (r32.double() - ref).abs().max().item()
    err = (val - ref).abs().max().item()
    bound = 4 * max(e32, qz * ref.abs().max().item())
    print(f"MQUERY {_mid(case)}: err {err:.3e} e32 {e32:.3e} err/e32 {err / max(e32, 1e-300):.2f} err/bound {err / bound:.3f}")
    assert err <= bound, (_mid(case), err, e32, bound)


def test_attention_mquery_rejects_bad_arguments():
    """The entry's argument checks, those of the query entry (no kernel runs)."""
    base = R.attn_layout()
    T, row, _, s0, s1, rows = base
    first, seq, pos = F.mquery_lists(base)
    qkv = torch.zeros(rows, 3 * 256, device="cuda")
    res = R.attn_residual_operands(rows, 256, device="cuda")
    out = torch.zeros(pos.numel(), 3 * 256, device="cuda")
    meta = {"len": T, "row": row, "first": first, "seq": seq, "pos": pos}
    lib = _lib.load()

    def call(kx=3, H=256, heads=4, s1_=s1, x32=res["x32"].data_ptr(), himg=None, meta_=meta):
        dm, keep = F.meta_struct(meta_)
        return lib.rs_debug_attention_mquery(qkv.data_ptr(), 1, ctypes.addressof(dm), s0, s1_, H, heads, kx, None, x32,
                                             res["stats"].data_ptr(), res["g"].data_ptr(), res["b"].data_ptr(), himg,
                                             out.data_ptr(), out.data_ptr(), _stream())
    assert call(kx=2) != 0
    assert call(H=256, heads=3) != 0
    assert call(s1_=s0) != 0
    assert call(x32=None) != 0                                  # neither residual source
    assert call(meta_=dict(meta, pos=None)) != 0
    assert call(meta_=dict(meta, first=None)) != 0
    torch.cuda.synchronize()
    assert not out.any()
