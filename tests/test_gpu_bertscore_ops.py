"""GPU: the BERTScore kernels one by one, without an encoder, against float64 —
bs_recall_kernel through rs_debug_bertscore_recall (the production layout checks, planner, upload and
launch_bertscore_recall on a hand-made embedding buffer), embed_out_kernel through rs_debug_embed_out
(launch_embed_out), mbr_scores_bs_kernel through rs_mbr_scores_bs on hand-made matrices.  References,
layouts and input families: tests/bertscore_ref.py (their properties: tests/test_bertscore_ref.py).

Recall kernel.  Every H in {256, 512, 768, 1024} x {fp16, two-part} — all eight instantiations of
launch_bertscore_recall's dispatch — on one ragged layout per instantiation (bertscore_ref.
recall_layout: ref lengths 2, 3, COLS - 1 .. COLS + 2, 2 COLS, 2 COLS + 1; runs of exactly COLS and
COLS + 1 columns; utterances of 1, 0, NG - 1, NG, NG + 1 hypotheses; 5, 32, 33, 255, 256, 257 and 521
cand rows; hypotheses across three row tiles and across the 256-row sweep), for the families plain,
twin, negative, onehot and spiky.  rmat and rmat0 start as a NaN sentinel and every element of every
block, the diagonal included, must be written; a second run and a run with rmat0 null must give
the same bits.  Asserted per case:
    err = max|got - ref64| <= 4 e32 + c
e32: the float32 evaluation's own error on the case (fp32 matmul, max, the chain acc += v * w in
column order); c = 0 (fp16) or 2^-24 max |a||b| (two-part: the lo.lo/4096 product the kernel omits
by design).  onehot asserts bit equality with the float32 chain instead.

embed_out_kernel.  The same H x {fp16, two-part}, from (x32, stats, g, b) or from the interleaved
image, sequences [2, 10) of a 12-sequence metadata array with row0 = 11, gaps between the row
ranges, token offsets in the reverse order, T = 1, 2, 3, 4, 5, 9, 64, 65, a plain and an offset
family.  out starts as a bit sentinel that must survive outside the launch's token rows.  Asserted:
|decoded - ref64| <= 4 max(e32, q max|e|), q = 2^-11 (fp16) or 2^-21 (two-part, after the exact
checks of the image alone, bertscore_ref.planar_defects), and the float64 norm of every decoded row
within the same bound of 1.

rs_mbr_scores_bs.  P, R and F for k in {2, 8, 9, 40, 100} (both branches of torch_sum_f32) over 1, 64
and 65 utterances with n > k hypotheses each (the matrix is read with stride n), negative recalls,
p = r = 0 (F = NaN -> 0), p = -r (F = -inf, kept) and exact ties: the scores equal torch.sum of the
same float32 vector on the CPU bit for bit and the argmax is the first maximum.

Measured on MI355X, recall kernel, err / e32 (largest over R and R0; onehot: bit equality held):
                 plain   twin   negative   spiky        err        e32
    H 256 fp16    0.95   0.81     1.20      0.83    <= 4.7e-7  2.5e-7 .. 3.9e-7
    H 512 fp16    0.92   0.66     0.88      1.11    <= 5.8e-7  3.3e-7 .. 5.2e-7
    H 768 fp16    1.01   1.13     1.37      0.98    <= 6.2e-7  3.2e-7 .. 6.3e-7
    H1024 fp16    1.17   1.31     1.23      1.74    <= 5.4e-7  2.5e-7 .. 4.4e-7
    H 256 two     1.03   1.03     1.03      1.00    <= 2.15e-6   2.08e-6 .. 2.15e-6
    H 512 two     1.03   1.03     1.03      1.03    <= 2.16e-6   2.09e-6
    H 768 two     1.03   1.03     1.03      1.06    <= 2.22e-6   2.08e-6 .. 2.09e-6
    H1024 two     1.03   1.03     1.03      1.06    <= 2.22e-6   2.09e-6 .. 2.10e-6
Every case is at 0.17 .. 0.44 of its bound.  In the two-part form err and e32 are both the chain's own
rounding on the diagonal of a long hypothesis (198 additions of fp32(1/198) to cosines of 1 +- 1e-7
give 1 - 2.1e-6 in the kernel and in the float32 evaluation alike; onehot shows the same 2.086e-6 in
both forms); the fp16 form's diagonal cosines |fp16(e)|^2 scatter by 1e-3 and dither that bias away.
spiky stays inside the bound in every instantiation: no finding about subnormal hi/64 and lo*64.
embed_out_kernel: fp16 err 6.0e-5 .. 1.14e-4, the fp16 rounding of the output, 0.13 .. 0.19 of the
bound; two-part err 2.5e-8 .. 4.7e-8, err / e32 0.88 .. 1.60, 0.05 .. 0.10 of the bound; the norm of a
decoded row within 0.08 .. 0.29 of the bound of 1; no image defect.  rs_mbr_scores_bs: bitwise.
Scratch builds (not kept) of bs_recall_kernel and the cases that fail on them: without the
a_lo.(b_hi/64) product all 16 two-part cases but onehot (H 1024 plain 2.6 times the bound, spiky
39 times); `row <= hi` in the fold, rows past r1 folded into the group's last hypothesis, the
read-modify-write of *dst replaced by 0, the interior clip off by one at either end: all 40 cases;
cm cleared to the key of 0.0f: the 32 cases other than onehot (negative by 0.8).
"""
import numpy as np
import pytest
import torch

from asr_rescoring_amd import _lib
import bertscore_ref as B

pytestmark = pytest.mark.gpu

SENT32, SENT16 = 0x7FC12345, 0x7E5A
RECALL_CASES = [(H, two, fam) for H in B.HIDDEN for two in (False, True) for fam in B.RECALL_FAMILIES]


def _rid(c):
    H, two, fam = c
    return f"H{H}-{'two' if two else 'f16'}-{fam}"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _recall(emb, H, two, hyp_off, utt_off, total, with_r0=True):
    """One rs_debug_bertscore_recall call into sentinel-filled matrices -> (rmat, rmat0 or None)."""
    hyp_off = np.ascontiguousarray(hyp_off, np.int32)
    utt_off = np.ascontiguousarray(utt_off, np.int32)
    assert emb.is_cuda and emb.dtype == torch.float16 and emb.is_contiguous()
    assert emb.shape == (int(hyp_off[utt_off[-1]]), H * (2 if two else 1))           # every row the kernel reads exists
    rmat = torch.full((total,), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    rmat0 = torch.full((total,), SENT32, dtype=torch.int32, device="cuda").view(torch.float32) if with_r0 else None
    rc = _lib.load().rs_debug_bertscore_recall(emb.data_ptr(), H, int(two), hyp_off.ctypes.data, utt_off.ctypes.data,
                                               len(utt_off) - 1, rmat.data_ptr(), rmat0.data_ptr() if with_r0 else None,
                                               _stream())
    assert rc == 0, (rc, _lib.load().rs_last_error().decode())
    torch.cuda.synchronize()
    return rmat, rmat0


@pytest.mark.parametrize("case", RECALL_CASES, ids=_rid)
def test_recall_kernel_vs_float64(case):
    H, two, fam = case
    c = B.recall_case(fam, H, two)
    total = int(B.mat_offsets(c["utt_off"])[-1])
    emb = c["emb"].cuda()
    rmat, rmat0 = _recall(emb, H, two, c["hyp_off"], c["utt_off"], total)
    for name, m in (("rmat", rmat), ("rmat0", rmat0)):
        left = int((_bits(m) == SENT32).sum())
        assert left == 0, f"{name}: {left} of {total} elements never written"
    got, got0 = rmat.double().cpu(), rmat0.double().cpu()
    assert torch.isfinite(got).all() and torch.isfinite(got0).all()
    ref, ref0 = c["ref"]
    err = max((got - ref).abs().max().item(), (got0 - ref0).abs().max().item())
    bound = 4 * c["e32"] + c["c"]
    print(f"BSRECALL {_rid(case)}: err {err:.3e} e32 {c['e32']:.3e} err/e32 {err / max(c['e32'], 1e-300):.2f} "
          f"c {c['c']:.3e} err/bound {err / max(bound, 1e-300):.3f}")
    again, again0 = _recall(emb, H, two, c["hyp_off"], c["utt_off"], total)
    assert torch.equal(_bits(rmat), _bits(again)) and torch.equal(_bits(rmat0), _bits(again0)), "run-to-run"
    alone, _ = _recall(emb, H, two, c["hyp_off"], c["utt_off"], total, with_r0=False)
    assert torch.equal(_bits(rmat), _bits(alone)), "rmat differs when rmat0 is null"
    if fam == "onehot":
        # every cosine is exactly 0 or 1 in every precision: the fp32 column-order chain, bit for bit
        w, w0 = c["r32"][0].float(), c["r32"][1].float()
        assert torch.equal(_bits(rmat.cpu()), _bits(w)) and torch.equal(_bits(rmat0.cpu()), _bits(w0)), \
            (int((rmat.cpu() != w).sum()), err)
    else:
        assert err <= bound, (_rid(case), err, c["e32"], bound)


def test_recall_entry_rejects_bad_arguments():
    """The entry's argument checks, those of rs_bertscore_recall (no kernel runs)."""
    lib = _lib.load()
    emb = torch.zeros(16, 256, dtype=torch.float16, device="cuda")
    out = torch.zeros(16, device="cuda")
    i32 = lambda v: np.asarray(v, np.int32)

    def call(ho=(0, 3, 8), uo=(0, 2), H=256, e=emb.data_ptr(), r=out.data_ptr(), n=None):
        ho, uo = i32(ho), i32(uo)
        return lib.rs_debug_bertscore_recall(e, H, 0, ho.ctypes.data, uo.ctypes.data, len(uo) - 1 if n is None else n, r,
                                             None, _stream())
    assert call(uo=(1, 2)) != 0 and b"utt_off[0]" in lib.rs_last_error()
    assert call(uo=(0, 2, 1)) != 0 and b"ascending" in lib.rs_last_error()
    assert call(ho=(1, 3, 8)) != 0 and b"hyp_off[0]" in lib.rs_last_error()
    assert call(ho=(0, 3, 4)) != 0 and b"hypothesis 1 has fewer than 2 tokens" in lib.rs_last_error()
    assert call(H=300) != 0 and call(H=0) != 0 and call(H=1280) != 0
    assert call(e=None) != 0 and call(r=None) != 0 and call(n=-1) != 0
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert not out.any()


# ---- embed_out_kernel ----------------------------------------------------------------------------

EMBED_CASES = [(H, two, img, fam) for H in B.HIDDEN for two in (False, True) for img in (False, True)
               for fam in ("plain", "offset")]


def _eid(c):
    H, two, img, fam = c
    return f"H{H}-{'two' if two else 'f16'}-{'himg' if img else 'stats'}-{fam}"


def _embed_out(op, layout, H, two, img):
    T, row, tok, s0, s1, row0, rows, tokens = layout
    d = lambda t: t.cuda().contiguous()
    dT, drow, dtok = d(T), d(row), d(tok)
    use = {k: d(v) for k, v in op.items()}
    assert use["x32"].shape == (rows, H) and use["stats"].shape == (rows, 2) and use["himg"].shape == (rows, 2 * H)
    # every row and token the launch touches lies inside the buffers
    assert int((row[s0:s1] - row0).min()) >= 0 and int((row[s0:s1] - row0 + T[s0:s1]).max()) <= rows
    assert int(tok[s0:s1].min()) >= 0 and int((tok[s0:s1] + T[s0:s1]).max()) <= tokens
    out = torch.full((tokens, H * (2 if two else 1)), SENT16, dtype=torch.int16, device="cuda").view(torch.float16)
    p = lambda k: use[k].data_ptr()
    src = (None, None, None, None, p("himg")) if img else (p("x32"), p("stats"), p("g"), p("b"), None)
    rc = _lib.load().rs_debug_embed_out(*src, dT.data_ptr(), drow.data_ptr(), dtok.data_ptr(), s0, s1, row0, H, int(two),
                                        out.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("case", EMBED_CASES, ids=_eid)
def test_embed_out_vs_float64(case):
    H, two, img, fam = case
    layout = B.embed_layout()
    T, row, tok, s0, s1, row0, rows, tokens = layout
    op = B.embed_operands(fam, H, rows, seed=H + 2 * two + 4 * img)
    out = _embed_out(op, layout, H, two, img)
    src = torch.cat([torch.arange(int(row[s]) - row0, int(row[s]) - row0 + int(T[s])) for s in range(s0, s1)])
    dst = torch.cat([torch.arange(int(tok[s]), int(tok[s]) + int(T[s])) for s in range(s0, s1)])
    keep = torch.ones(tokens, dtype=torch.bool)
    keep[dst] = False
    assert (_bits(out[keep]) == SENT16).all(), "a token row outside the launch was written"
    got = out[dst]
    assert not (_bits(got) == SENT16).all(dim=1).any(), "a token row of the launch was not written"
    ref = B.embed_out_ref(op, img, torch.float64)[src]
    e32 = (B.embed_out_ref(op, img, torch.float32).double()[src] - ref).abs().max().item()
    if two:
        assert B.planar_defects(got) == []                         # hi == fp16(hi + lo/64), lo finite
        val, q = B.decode_planar(got), 2.0 ** -21
    else:
        val, q = got.double(), 2.0 ** -11
    assert torch.isfinite(val).all()
    bound = 4 * max(e32, q * ref.abs().max().item())
    err = (val - ref).abs().max().item()
    nerr = (val.norm(dim=1) - 1.0).abs().max().item()
    print(f"EMBEDOUT {_eid(case)}: err {err:.3e} e32 {e32:.3e} err/e32 {err / max(e32, 1e-300):.2f} "
          f"err/bound {err / bound:.3f} norm err {nerr:.3e} ({nerr / bound:.3f} of the bound)")
    again = _embed_out(op, layout, H, two, img)
    assert torch.equal(_bits(out), _bits(again)), "run-to-run"
    assert err <= bound, (_eid(case), err, e32, bound)
    assert nerr <= bound, (_eid(case), nerr, bound)


def test_embed_out_entry_rejects_bad_arguments():
    """The entry's argument checks (no kernel runs)."""
    layout = B.embed_layout()
    T, row, tok, s0, s1, row0, rows, tokens = layout
    op = {k: v.cuda() for k, v in B.embed_operands("plain", 256, rows).items()}
    out = torch.zeros(tokens, 256, dtype=torch.float16, device="cuda")
    dT, drow, dtok = T.cuda(), row.cuda(), tok.cuda()
    lib = _lib.load()

    def call(x32=op["x32"].data_ptr(), himg=None, H=256, s1_=s1, ln=dT.data_ptr(), o=out.data_ptr()):
        return lib.rs_debug_embed_out(x32, op["stats"].data_ptr(), op["g"].data_ptr(), op["b"].data_ptr(), himg, ln,
                                      drow.data_ptr(), dtok.data_ptr(), s0, s1_, row0, H, 0, o, _stream())
    assert call(x32=None) != 0                                   # neither source
    assert call(H=320) != 0 and call(s1_=s0) != 0 and call(ln=None) != 0 and call(o=None) != 0
    torch.cuda.synchronize()
    assert not out.any()


# ---- rs_mbr_scores_bs ----------------------------------------------------------------------------

def _mbr_matrices(k, n_utt, seed):
    """Hand-made recall blocks of n > k hypotheses per utterance, cycling through four kinds:
    0 uniform in [-0.5, 1) (negative recalls); 1 the same with one hypothesis z < k whose row and
    column are 0 (p = r = 0 against every other: F = 0/0 = NaN -> 0) and rows / columns past k poisoned
    with NaN (never read); 2 a constant 0.25 with the rows and columns of two hypotheses a < b < k at
    0.75 (their scores tie exactly, and are the largest); 3 kind 0 with one pair p = -r (F = -inf)."""
    rng = np.random.default_rng(seed)
    ns = [k + 1 + (u % 3) for u in range(n_utt)]
    mats = []
    for u, n in enumerate(ns):
        m = rng.uniform(-0.5, 1.0, (n, n)).astype(np.float32)
        kind = u % 4
        if kind == 1:
            z = int(rng.integers(0, k))
            m[z, :] = 0.0
            m[:, z] = 0.0
            m[k:, :] = np.nan
            m[:, k:] = np.nan
        elif kind == 2:
            a, b = sorted(rng.choice(k, size=2, replace=False).tolist())
            m[:] = 0.25
            for h in (a, b):
                m[h, :] = 0.75
                m[:, h] = 0.75
        elif kind == 3:
            a, b = rng.choice(k, size=2, replace=False).tolist()
            m[a, b], m[b, a] = 0.25, -0.25
        mats.append(m)
    return ns, mats


def _mbr_ref(mats, k, which):
    """scores [U, k] float32 = torch.sum (CPU) of the k - 1 utilities of cand i in the order
    j = 0 .. i-1, i+1 .. k-1, and the first maximum."""
    scores = np.zeros((len(mats), k), np.float32)
    for u, m in enumerate(mats):
        r, p = m[:k, :k], m[:k, :k].T
        if which == "R":
            val = r
        elif which == "P":
            val = p
        else:
            with np.errstate(all="ignore"):
                val = ((np.float32(2.0) * p) * r) / (p + r)
            val = np.where(np.isnan(val), np.float32(0.0), val).astype(np.float32)
        for i in range(k):
            vec = np.ascontiguousarray(np.delete(val[i], i), np.float32)
            scores[u, i] = torch.from_numpy(vec).sum().item()
    assert not np.isnan(scores).any()
    return scores, np.argmax(scores, axis=1)


@pytest.mark.parametrize("n_utt", [1, 64, 65])
@pytest.mark.parametrize("k", [2, 8, 9, 40, 100])
def test_mbr_scores_bs_hand_made(k, n_utt):
    from asr_rescoring_amd.bertscore import WHICH
    ns, mats = _mbr_matrices(k, n_utt, seed=1000 * k + n_utt)
    assert all(n > k for n in ns) and any((m[:k, :k] < 0).any() for m in mats)       # negative recalls are read
    flat = torch.from_numpy(np.concatenate([m.ravel() for m in mats])).cuda()
    moff = torch.from_numpy(np.concatenate([[0], np.cumsum([n * n for n in ns])]).astype(np.int64)).cuda()
    uoff = torch.from_numpy(np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)).cuda()
    lib = _lib.load()
    for which in ("P", "R", "F"):
        want, want_am = _mbr_ref(mats, k, which)
        scores = torch.full((n_utt, k), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
        am = torch.full((n_utt,), -7, dtype=torch.int32, device="cuda")
        rc = lib.rs_mbr_scores_bs(flat.data_ptr(), moff.data_ptr(), uoff.data_ptr(), n_utt, k, WHICH[which],
                                  scores.data_ptr(), am.data_ptr(), _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        got = scores.cpu().numpy()
        diff = got.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), (which, int(diff.sum()), got[diff][:4], want[diff][:4])
        assert np.array_equal(am.cpu().numpy(), want_am.astype(np.int32)), which
        # the cases are there: an exact tie at the top won by the first, -inf kept, NaN -> 0
        if n_utt >= 4:
            u = 2
            top = np.flatnonzero(want[u] == want[u].max())
            assert len(top) == 2 and want_am[u] == top[0]
            if which == "F":
                assert np.isneginf(want[3]).sum() == 2 and np.isfinite(want[1]).all()
