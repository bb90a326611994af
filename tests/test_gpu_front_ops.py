"""GPU: the kernels a default MLM call starts and ends in, one by one and without an encoder, through
their production launchers — embed_ln_kernel / embed_ln_set_kernel / embed_unique_kernel
(rs_debug_embed -> launch_embed_ln / _set / _unique), the four gathers (rs_debug_gather), cls_linear_kernel
and segsum_f64_kernel.  Layouts, operands and references: tests/front_ref.py (their properties:
tests/test_front_ref.py).  Tables are tiny (vocab 64, type_vocab 2, 160 positions); every output buffer
is bit-sentinel filled and larger than the launch.

Embedding, form 0 (embed_ln).  Sequences [2, 11) of a 12-sequence metadata array with row0 = 11 (the
nine lengths 1, 2, 3, 4, 5, 9, 64, 65, 130 need nine launched sequences, so the launch ends at 11 where
the embed_out test's eight end at 10), gaps between the row ranges, the outside sequences' rows inside
the sentinel rows; ids -5 and vocab + 7, types -1 and type_vocab + 3 (clamped), types on / null; spans none,
one position, three wide, ending at T - 1; H in {256, 512, 768, 1024} x kx in {1, 2, 3}; a plain and an
offset (word + 30) family.  Asserted: x32 bitwise (word[id] + type[ty]) + pos[t] in fp32; the decoded
image (after the exact checks of the image alone) within 4 max(e32, q max|y|) of the float64 LayerNorm of
the held x32, q = 2^-11 (kx 1) or 2^-21 (kx 2 / 3), e32 the error of torch's fp32 layer_norm; mean and
rstd within 4 times the error of their fp32 evaluation, both errors taken in the max norm over the
launch's rows relative to the largest |value| (the per-row relative error of a mean near zero is
unbounded for every summation order, so it is no yardstick); rows outside the launch keep their
sentinel in x32, stats and h16; two runs bitwise equal; with x32 / stats null or h16 null the outputs
given keep their bits.
Form 1 (embed_ln_set): the three outputs of every row bitwise those of embed_ln on a copy whose
one-position span is the row's position (an unmasked row: the unmasked copy's).
Form 2 (embed_unique) on the dedup chunk (PLL run, cut run with absent copies, overlapping wide spans,
one-copy run, T = 3, up to T = 130): every unique row bitwise the h16 row embed_ln writes for the same
(hypothesis, position, masked?) — both on a layout holding every triple once and on the chunk's own
copies through SeqRows' addressing — and the rows at and past urows untouched; kx 1 and 2, all four H.

Gathers: dst bitwise the gathered rows for ld = H, 2H, 3H (H = 256), [s0, s1) / q0 != 0 / row0 != 0, rows past n
sentinel, ld % 8 != 0 rejected; labels for n = 1, 255, 256, 257.  cls_linear: err <= 4 max(e32, 2^-23 max|y|),
e32 the error of torch's fp32 dot.  segsum_f64: bitwise the sequential float64 sum.

Measured on MI355X (all 24 + 24 + 16 embedding cases, both families; every bit equality held):
    image, kx 2 / 3, plain:   err 1.2e-6 .. 1.8e-6, e32 9.0e-7 .. 1.6e-6, err / e32 0.80 .. 1.84, 0.08 .. 0.12 of the bound
    image, kx 2 / 3, offset:  err 2.8e-6 .. 5.9e-6, e32 2.9e-6 .. 4.9e-6, err / e32 0.82 .. 1.24, 0.19 .. 0.31 of the bound
    image, kx 1:              err 1.95e-3 .. 3.5e-3, the fp16 rounding of the output (e32 ~ 1e-6): 0.12 .. 0.21 of the bound
    mean:  rel err 6.6e-8 .. 1.5e-7, the fp32 evaluation's 6.6e-8 .. 1.7e-7, ratio 0.54 .. 1.45
    rstd:  rel err 8.2e-8 .. 1.4e-7, the fp32 evaluation's 8.6e-8 .. 1.6e-7, ratio 0.81 .. 1.39
    cls_linear: err 1.0e-8 .. 8.3e-7, e32 1.1e-7 .. 5.7e-7, 0.02 .. 0.27 of the bound
Scratch builds (not kept; each reads and writes only inside the over-sized buffers) and the cases that
fail on them:
    embed_unique writing n_mask + 1 rows: all 16 embed_unique cases ("a row at or past urows was written": the
        last run's extra row lands in the sentinel rows);
    embed_row taking the type of position 0 for a [MASK] row: the 12 embed_ln cases with types (x32 bitwise);
        the set / unique comparisons hold, as they must — both sides go through the same embed_row;
    gather_query_rows_list indexing dst by q instead of q - q0: the three gather cases with a valid ld.
"""
import ctypes

import numpy as np
import pytest
import torch

from asr_rescoring_amd import _lib
import front_ref as F
import tail_ref as R
from x3s_image import _unsplit2, ln_ref64

pytestmark = pytest.mark.gpu

SENT32, SENT16 = 0x7FC12345, 0x7E5A
EPS = 1e-12


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float16: torch.int16, torch.float64: torch.int64,
                                torch.int32: torch.int32}[t.dtype])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sent(shape, dtype):
    if dtype == torch.float16:
        return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(torch.float16)
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _embed(form, lay, tok, typ, tab, H, kx, want=("x32", "stats", "h16"), urows=0, h16_rows=None, expect=0):
    """One rs_debug_embed launch into sentinel-filled buffers -> dict of the outputs asked for."""
    dm, keep = F.meta_struct(lay["meta"])
    rows = lay["rows"] if h16_rows is None else h16_rows
    out = {"x32": _sent((rows, H), torch.float32) if "x32" in want else None,
           "stats": _sent((rows, 2), torch.float32) if "stats" in want else None,
           "h16": _sent((rows, kx * H), torch.float16) if "h16" in want else None}
    rc = _lib.load().rs_debug_embed(form, tok.data_ptr(), _p(typ), ctypes.addressof(dm), lay["s0"], lay["s1"],
                                    lay["row0"] if form == 0 else 0, urows, F.MASK_ID, F.VOCAB, F.TYPE_VOCAB,
                                    tab["word"].data_ptr(), tab["pos"].data_ptr(), tab["typetab"].data_ptr(),
                                    tab["g"].data_ptr(), tab["b"].data_ptr(), EPS, H, _p(out["x32"]), _p(out["stats"]),
                                    _p(out["h16"]), kx, _stream())
    torch.cuda.synchronize()
    assert (rc == 0) == (expect == 0), rc
    return out


def _untouched(out, own):
    """Every row outside ``own`` keeps the bit sentinel in every output given."""
    for k, t in out.items():
        if t is None:
            continue
        keep = torch.ones(t.shape[0], dtype=torch.bool, device="cuda")
        keep[own.cuda()] = False
        sent = SENT16 if t.dtype == torch.float16 else SENT32
        assert (_bits(t)[keep] == sent).all(), f"{k}: a row outside the launch was written"


def _decode(h16, kx):
    if kx == 1:
        return h16.double(), 2.0 ** -11
    if kx == 2:
        assert F.image2_defects(h16) == []
        return _unsplit2(h16, torch.float64), 2.0 ** -21
    assert R.image3_defects(h16) == []
    return R._unsplit3(h16, torch.float64), 2.0 ** -21


def _tokens(n_tok, types, seed=0):
    tok, typ = F.embed_tokens(n_tok, seed)
    return tok.cuda(), (typ.cuda() if types else None), tok, (typ if types else None)


GRID = [(H, kx, types) for H in F.HIDDEN for kx in (1, 2, 3) for types in (True, False)]


def _gid(c):
    return f"H{c[0]}-kx{c[1]}-{'types' if c[2] else 'notypes'}"


@pytest.mark.parametrize("case", GRID, ids=_gid)
def test_embed_ln_vs_float64(case):
    H, kx, types = case
    lay = F.embed_layout()
    m, s0, s1, row0 = lay["meta"], lay["s0"], lay["s1"], lay["row0"]
    own, _, _ = F.launch_rows(m, s0, s1, row0)
    tok_d, typ_d, tok, typ = _tokens(lay["n_tok"], types)
    for fam in ("plain", "offset"):
        tab = F.embed_tables(fam, H, seed=H + kx, device="cuda")
        out = _embed(0, lay, tok_d, typ_d, tab, H, kx)
        _untouched(out, own)
        x32 = out["x32"][own.cuda()]
        want = F.embed_sum(tok, typ, m, s0, s1, tab)
        assert torch.equal(_bits(x32), _bits(want)), f"x32 != (word + type) + pos in fp32 at {int((x32 != want).sum())}"
        # statistics: the max-norm relative error against that of the fp32 evaluation
        m64, r64 = F.row_stats_in(x32, torch.float64)
        m32, r32 = F.row_stats_in(x32, torch.float32)
        st = out["stats"][own.cuda()].double()
        for name, got, ref, y32 in (("mean", st[:, 0], m64, m32), ("rstd", st[:, 1], r64, r32)):
            scale = ref.abs().max().item()
            err, e32 = (got - ref).abs().max().item() / scale, (y32.double() - ref).abs().max().item() / scale
            print(f"EMBED {_gid(case)}-{fam}: {name} rel err {err:.3e} fp32 {e32:.3e} ratio {err / e32:.2f}")
            assert err <= 4 * e32, (name, err, e32)
        # the image against the float64 LayerNorm of the held x32
        val, q = _decode(out["h16"][own.cuda()], kx)
        assert torch.isfinite(val).all()
        y64 = ln_ref64(x32, tab["g"], tab["b"], EPS)
        e32 = (torch.nn.functional.layer_norm(x32, (H,), tab["g"], tab["b"], EPS).double() - y64).abs().max().item()
        err, bound = (val - y64).abs().max().item(), 4 * max(e32, q * y64.abs().max().item())
        print(f"EMBED {_gid(case)}-{fam}: err {err:.3e} e32 {e32:.3e} err/e32 {err / e32:.2f} err/bound {err / bound:.3f}")
        again = _embed(0, lay, tok_d, typ_d, tab, H, kx)
        for k in out:
            assert torch.equal(_bits(out[k]), _bits(again[k])), f"run-to-run: {k}"
        assert err <= bound, (_gid(case), fam, err, e32, bound)


@pytest.mark.parametrize("H", F.HIDDEN)
def test_embed_ln_null_outputs(H):
    """The null-output combinations production uses: x32 / stats null with h16 given (the dedup copy rows
    are never written), h16 null with x32 / stats given (dedup: the image comes from embed_unique)."""
    lay = F.embed_layout()
    own, _, _ = F.launch_rows(lay["meta"], lay["s0"], lay["s1"], lay["row0"])
    tok_d, typ_d, _, _ = _tokens(lay["n_tok"], True)
    tab = F.embed_tables("plain", H, seed=H, device="cuda")
    for kx in (1, 2):
        full = _embed(0, lay, tok_d, typ_d, tab, H, kx)
        img = _embed(0, lay, tok_d, typ_d, tab, H, kx, want=("h16",))
        res = _embed(0, lay, tok_d, typ_d, tab, H, kx, want=("x32", "stats"))
        _untouched(img, own)
        _untouched(res, own)
        assert torch.equal(_bits(img["h16"]), _bits(full["h16"]))
        assert torch.equal(_bits(res["x32"]), _bits(full["x32"])) and torch.equal(_bits(res["stats"]), _bits(full["stats"]))


@pytest.mark.parametrize("case", GRID, ids=_gid)
def test_embed_ln_set_rows_are_embed_ln_rows(case):
    H, kx, types = case
    lay = F.embed_layout(row0=0)
    ex, src = F.expand_queries(lay)
    own, _, _ = F.launch_rows(lay["meta"], lay["s0"], lay["s1"], 0)
    tok_d, typ_d, _, _ = _tokens(lay["n_tok"], types, seed=1)
    tab = F.embed_tables("plain", H, seed=2 * H + kx, device="cuda")
    got = _embed(1, lay, tok_d, typ_d, tab, H, kx)
    ref = _embed(0, ex, tok_d, typ_d, tab, H, kx)
    _untouched(got, own)
    for k in ("x32", "stats", "h16"):
        a, b = _bits(got[k][own.cuda()]), _bits(ref[k][src.cuda()])
        assert torch.equal(a, b), f"{k}: {int((a != b).any(dim=1).sum())} rows differ from embed_ln's"
    # the comparison has masked rows in it: a masked row differs from its unmasked copy
    um = _embed(0, F.embed_layout(row0=0) | {"meta": lay["meta"] | {"mask_pos": F.i32([-1] * 12), "mask_end": F.i32([-1] * 12)}},
                tok_d, typ_d, tab, H, kx)
    n_masked = int((_bits(um["x32"][own.cuda()]) != _bits(got["x32"][own.cuda()])).any(dim=1).sum())
    assert n_masked == int(lay["meta"]["first"][lay["s1"]] - lay["meta"]["first"][lay["s0"]]), n_masked


UGRID = [(H, kx, types) for H in F.HIDDEN for kx in (1, 2) for types in (True, False)]


@pytest.mark.parametrize("case", UGRID, ids=_gid)
def test_embed_unique_rows_are_embed_ln_rows(case):
    H, kx, types = case
    ch = F.dedup_chunk(F.RUNS[130])
    urows = ch["urows"]
    alloc = F.pad_to(urows, 256) + 8
    tok_d, typ_d, _, _ = _tokens(ch["n_tok"], types, seed=2)
    tab = F.embed_tables("plain", H, seed=3 * H + kx, device="cuda")
    h16u = _embed(2, ch, tok_d, typ_d, tab, H, kx, want=("h16",), urows=urows, h16_rows=alloc)["h16"]
    assert (_bits(h16u[urows:]) == SENT16).all(), "a row at or past urows was written"
    assert not (_bits(h16u[:urows]) == SENT16).all(dim=1).any(), "a unique row was not written"
    # every (hypothesis, position, masked?) once, by embed_ln
    lay, row_of = F.triple_layout(ch)
    ref = _embed(0, lay, tok_d, typ_d, tab, H, kx, want=("h16",))["h16"]
    a, b = _bits(h16u[:urows]), _bits(ref[row_of(F.unique_triples(ch)).cuda()])
    assert torch.equal(a, b), f"{int((a != b).any(dim=1).sum())} unique rows differ from embed_ln's row of their triple"
    # the chunk's own copies through SeqRows' addressing
    urow, _, _ = F.unique_map(ch)
    own, _, _ = F.launch_rows(ch["meta"], ch["s0"], ch["s1"], 0)
    full = _embed(0, ch, tok_d, typ_d, tab, H, kx, want=("h16",))["h16"]
    a, b = _bits(h16u[urow.cuda()]), _bits(full[own.cuda()])
    assert torch.equal(a, b), f"{int((a != b).any(dim=1).sum())} copy rows differ from their unique row"
    again = _embed(2, ch, tok_d, typ_d, tab, H, kx, want=("h16",), urows=urows, h16_rows=alloc)["h16"]
    assert torch.equal(_bits(h16u), _bits(again)), "run-to-run"


def test_embed_entry_rejects_bad_arguments():
    lay = F.embed_layout()
    tok_d, typ_d, _, _ = _tokens(lay["n_tok"], True)
    tab = F.embed_tables("plain", 256, device="cuda")
    own, _, _ = F.launch_rows(lay["meta"], lay["s0"], lay["s1"], lay["row0"])
    bad = [dict(lay, s1=lay["s0"]), dict(lay, meta=dict(lay["meta"], len=None)), dict(lay, meta=dict(lay["meta"], row=None))]
    for b in bad:
        _untouched(_embed(0, b, tok_d, typ_d, tab, 256, 1, expect=-1), torch.tensor([], dtype=torch.long))
    _untouched(_embed(0, lay, tok_d, typ_d, tab, 320, 1, expect=-1), torch.tensor([], dtype=torch.long))   # no such H
    _untouched(_embed(0, lay, tok_d, typ_d, tab, 256, 4, expect=-1), torch.tensor([], dtype=torch.long))   # no such kx
    _embed(0, lay, tok_d, typ_d, tab, 256, 1, want=(), expect=-1)                                          # no output
    _untouched(_embed(1, dict(lay, meta=dict(lay["meta"], first=None)), tok_d, typ_d, tab, 256, 1, expect=-1),
               torch.tensor([], dtype=torch.long))
    _untouched(_embed(2, lay, tok_d, typ_d, tab, 256, 1, urows=8, expect=-1), torch.tensor([], dtype=torch.long))  # no urow_*


# ---- gathers ---------------------------------------------------------------------------------------------

def _gather(op, src, ld, tok, meta, a0, a1, row0, dst, lab, llog):
    dm, keep = F.meta_struct(meta)
    rc = _lib.load().rs_debug_gather(op, _p(src), ld, _p(tok), ctypes.addressof(dm), a0, a1, row0, _p(dst), _p(lab),
                                     _p(llog), _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("ld", [256, 512, 768, 250])
def test_gather_query_rows(ld):
    """dst[s - s0] = src[row[s] - row0 + query[s]] and dst[q - q0] = src[row[seq[q]] + pos[q]], bitwise, ld halfs per
    row (H, 2H, 3H for H = 256); rows past the launch keep the sentinel; an ld that is no multiple of 8 is
    rejected."""
    lay = F.embed_layout()
    m, s0, s1, row0 = dict(lay["meta"]), lay["s0"], lay["s1"], lay["row0"]
    T = m["len"]
    m["query"] = F.i32((0, int(t) - 1, int(t) // 2)[i % 3] for i, t in enumerate(T))
    g = torch.Generator().manual_seed(ld)
    src = torch.randint(-2 ** 15, 2 ** 15, (lay["rows"] + row0, ld), generator=g, dtype=torch.int16).cuda().view(torch.float16)
    n_seq, nq_all = len(T), int(m["first"][-1])
    q0, nq = int(m["first"][s0]), int(m["first"][s1] - m["first"][s0])
    assert q0 != 0
    dst = _sent((n_seq, ld), torch.float16)
    dstq = _sent((nq_all, ld), torch.float16)
    rc0 = _gather(0, src[row0:], ld, None, m, s0, s1, row0, dst, None, None)
    m0 = dict(m, row=m["row"] - row0)
    rc1 = _gather(1, src[row0:], ld, None, m0, q0, nq, 0, dstq, None, None)
    if ld % 8:
        assert rc0 != 0 and rc1 != 0
        assert (_bits(dst) == SENT16).all() and (_bits(dstq) == SENT16).all()
        return
    assert rc0 == 0 and rc1 == 0
    want = src[(m["row"][s0:s1] + m["query"][s0:s1]).long().cuda()]
    assert torch.equal(_bits(dst[:s1 - s0]), _bits(want)) and (_bits(dst[s1 - s0:]) == SENT16).all()
    rq = (m["row"][m["seq"][q0:q0 + nq].long()] + m["pos"][q0:q0 + nq]).long().cuda()
    assert torch.equal(_bits(dstq[:nq]), _bits(src[rq])) and (_bits(dstq[nq:]) == SENT16).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("with_tok", [True, False])
def test_gather_labels(n, with_tok):
    """lab[i] = the label of sequence s0 + i / query q0 + i: -1 takes the token at the position (tok null: -1
    passes through), any other value is kept as it is (-7 and vocab + 9 included); label_logit = -inf over
    [0, n) and the sentinel after."""
    n_all, s0 = 300, 5
    g = torch.Generator().manual_seed(n)
    tok = torch.randint(0, F.VOCAB, (3 * n_all + 8,), generator=g, dtype=torch.int32)
    label = torch.randint(0, F.VOCAB, (n_all,), generator=g, dtype=torch.int32)
    label[0::2], label[3::10], label[7::10] = -1, -7, F.VOCAB + 9
    seq_meta = {"tok_off": F.i32(3 * s + 2 for s in range(n_all)), "len": F.i32([3] * n_all),
                "query": F.i32(s % 3 for s in range(n_all)), "label": label}
    # the list form: query q belongs to sequence (7 q) % n_all at position (q + 1) % 3
    list_meta = {"tok_off": seq_meta["tok_off"], "seq": F.i32((7 * q) % n_all for q in range(n_all)),
                 "pos": F.i32((q + 1) % 3 for q in range(n_all)), "qlabel": label.flip(0).contiguous()}
    tok_d = tok.cuda() if with_tok else None
    for op, meta, a1 in ((2, seq_meta, s0 + n), (3, list_meta, n)):
        lab = torch.full((n_all,), SENT32, dtype=torch.int32, device="cuda")
        llog = _sent((n_all,), torch.float32)
        assert _gather(op, None, 0, tok_d, meta, s0, a1, 0, None, lab, llog) == 0
        idx = torch.arange(s0, s0 + n)
        if op == 2:
            l, at = label[idx], tok[(seq_meta["tok_off"][idx] + seq_meta["query"][idx]).long()]
        else:
            l, at = list_meta["qlabel"][idx], tok[(list_meta["tok_off"][list_meta["seq"][idx].long()] + list_meta["pos"][idx]).long()]
        want = torch.where(l == -1, at, l) if with_tok else l
        assert {-7, F.VOCAB + 9} <= set(want.tolist()) or n == 1
        assert torch.equal(lab[:n].cpu(), want) and (lab[n:] == SENT32).all(), op
        assert (llog[:n] == -float("inf")).all() and (_bits(llog[n:]) == SENT32).all(), op


def test_gather_entry_rejects_bad_arguments():
    lay = F.embed_layout()
    m = dict(lay["meta"], query=F.i32([0] * 12))
    src = torch.zeros(lay["rows"], 256, dtype=torch.float16, device="cuda")
    dst = _sent((12, 256), torch.float16)
    assert _gather(0, src, 256, None, m, 5, 5, 0, dst, None, None) != 0          # s1 <= s0
    assert _gather(0, None, 256, None, m, 2, 5, 0, dst, None, None) != 0
    assert _gather(0, src, 256, None, dict(m, query=None), 2, 5, 0, dst, None, None) != 0
    assert _gather(1, src, 256, None, dict(m, seq=None), 2, 5, 0, dst, None, None) != 0
    assert _gather(4, src, 256, None, m, 2, 5, 0, dst, None, None) != 0
    assert _gather(2, None, 0, None, m, 2, 5, 0, None, None, None) != 0           # no lab / llog
    assert (_bits(dst) == SENT16).all()


# ---- heads -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [256, 768])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 9])
def test_cls_linear_vs_float64(rows, H):
    g = torch.Generator(device="cuda").manual_seed(rows + H)
    h = torch.randn(rows + 3, H, device="cuda", generator=g) * 2 + 0.5
    w = 0.05 * torch.randn(H, device="cuda", generator=g)
    b = torch.tensor([0.37], device="cuda")
    out = _sent((rows + 3,), torch.float32)
    assert _lib.load().rs_debug_cls_linear(h.data_ptr(), rows, H, w.data_ptr(), b.data_ptr(), out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert (_bits(out[rows:]) == SENT32).all(), "rows past the launch written"
    ref = h[:rows].double() @ w.double() + b.double()
    e32 = ((h[:rows] @ w + b).double() - ref).abs().max().item()
    err = (out[:rows].double() - ref).abs().max().item()
    bound = 4 * max(e32, 2.0 ** -23 * ref.abs().max().item())
    print(f"CLS rows {rows} H {H}: err {err:.3e} e32 {e32:.3e} err/bound {err / bound:.3f}")
    assert err <= bound, (err, e32, bound)
    assert _lib.load().rs_debug_cls_linear(None, rows, H, w.data_ptr(), b.data_ptr(), out.data_ptr(), _stream()) != 0
    assert _lib.load().rs_debug_cls_linear(h.data_ptr(), 0, H, w.data_ptr(), b.data_ptr(), out.data_ptr(), _stream()) != 0


@pytest.mark.parametrize("n", [1, 256, 257])
def test_segsum_is_the_sequential_float64_sum(n):
    """Segments of 0, 1, 2 and 300 rows in turn (n = 1: the 300-row one): bitwise the float64 sum in row order;
    an empty segment gives exactly 0.0; out past n keeps the sentinel."""
    lens = [300] if n == 1 else [(0, 1, 2, 300)[h % 4] for h in range(n)]
    off = np.concatenate([[4], 4 + np.cumsum(lens)]).astype(np.int32)
    x = (np.random.default_rng(n).standard_normal(int(off[-1]) + 5) * 10).astype(np.float32)
    want = F.segsum_ref(x, off)
    out = torch.full((n + 3,), SENT32, dtype=torch.int64, device="cuda").view(torch.float64)
    d_x, d_off = torch.from_numpy(x).cuda(), torch.from_numpy(off).cuda()
    assert _lib.load().rs_debug_segsum(d_x.data_ptr(), d_off.data_ptr(), n, out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:n].view(np.int64) == want.view(np.int64)).all(), int((got[:n] != want).sum())
    assert (got[n:].view(np.int64) == SENT32).all()
    if n > 1:
        assert got[0] == 0.0 and not np.signbit(got[0])
    assert _lib.load().rs_debug_segsum(d_x.data_ptr(), None, n, out.data_ptr(), _stream()) != 0
