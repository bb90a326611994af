"""GPU: the trainer's non-attention kernels (k_train.hip) through the rs_debug_train_* entries — the
launchers train_api.hip calls, on caller-provided buffers — against the float64 reference of
tests/train_ops_ref.py.

Bound (the rule of tests/test_gpu_attention.py and tests/test_gpu_train_attn.py): for every output
tensor max |out - ref64| <= 4 e32, e32 = max |ref32 - ref64|, ref32 the same expressions in torch
float32 on the same inputs.  For the pointwise ops and the cross-entropy's d-logits the rule is
applied per band of input magnitude (|x| < 1, 1-3, 3-6, > 6), so an error in the tails is not hidden
by the bulk.  An output that is one correctly rounded fp32 operation per step in a fixed order
(tr_bias, the saved pre-LN sums without dropout, the row moves, d score w of the CLS rows) must
equal the float32 reference bit for bit; zeros the kernels promise (a type without rows, dh off the
CLS rows, expanded rows that are not listed) are bitwise +0.  Output buffers are NaN-filled before
each call and must come back finite.

Fast intrinsics: tr_ce (``__expf``, ``__logf``) and tr_gelu_bwd (``__expf``) are compared with the
reference in the same function forms, exp2(x log2 e) and log2(x) ln 2 (train_ops_ref.exp_fast /
log_fast), so e32 carries the argument rounding of the form.

Cross-entropy labels: the kernel clamps a label into [0, V) (the labelled entry never passes an
ignore_index row to it), so the row labelled -100 is scored as label 0 — by the reference too.

MD_MWED: a group whose CER sums to 0 has T = sum c / 0, a division by zero in the reference as
well; the inputs keep every CER >= 0.05 and no such group is tested.

AdamW: ref32 / ref64 are torch.optim.AdamW(foreach=False) on float32 / float64 CPU tensors with
the float32-rounded hyper-parameters the entry receives.

Every output of more than a few elements is held to the rule case by case (each M, each draw,
each input family on its own).  Only outputs of one or a few elements (a loss, a bias gradient, the
means of a few rows) are gathered into one tensor per name before the rule is applied, and only
over the sizes or draws of one input family (_Pool), so that its maxima run over more than a
single rounding.

Where e32 is not torch's: the reasons, each from the kernel's code, are in _colsum_case (the
column sums' interleaved lanes and fmaf: a float32 numpy model of that order) and
test_losses_vs_float64 (the loss total's index-order chain, against which torch.sum gave
err / e32 = 35; MD_MWED's dsc, whose two terms the reference adds one after the other as the
kernel does).

Measured err / e32 on MI355X, the largest over the cases of each op:
  embed_ln       mean 1.68  rstd 1.00  h0 1.83          (x0 bit-equal to float32)
  bias_res_ln    y (dropout) 1.00  mean 1.86  rstd 2.14  h 3.06
  ln_bwd         dx 1.12
  bias_gelu      act |x| < 1: 1.25  1-3: 1.17  3-6: 1.00  > 6: 1.00   (pre bit-equal)
  gelu_bwd       d   |x| < 1: 1.23  1-3: 1.12  3-6: 1.00  > 6: 1.00
  colsum         modes 0 / 1, accumulate, row predicate: 1.00 (order model)
  word / pos     dword 1.00  dpos 1.00
  CLS head       score 0.48  dw 1.71  db 1.00            (dh bit-equal)
  losses         dsc 1.59  uloss 1.71  total 1.00 (order model; torch.sum 35)
  cross-entropy  row 1.82  mean 1.62  d-logits |x| < 1: 1.03  1-3: 1.63  3-6: 2.56  > 6: 1.00
  AdamW          p 1.40  m 1.00  v 1.00
(err 8e-24 .. 0.41, the largest the rstd = 1e6 of the constant rows; e32 8e-24 .. 0.46.)
"""
import functools

import numpy as np
import pytest
import torch

import train_ops_ref as R
from asr_rescoring_amd import _lib

pytestmark = pytest.mark.gpu

RS_EARG, RS_EUNSUP = -1, -5
NAN = float("nan")
EPS = 1e-12
BANDS = [(0.0, 1.0), (1.0, 3.0), (3.0, 6.0), (6.0, float("inf"))]
DROP = dict(seed=1234, step=7, site=2, p=0.1)
NODROP = dict(seed=0, step=0, site=0, p=0.0)


def _dev():
    return torch.device("cuda", 0)


def _g(t):
    return None if t is None else t.contiguous().to(_dev())


def _nan(*shape):
    return torch.full(shape, NAN, device=_dev())


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc):
    assert rc == 0, _lib.load().rs_last_error()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).float()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(tag, parts):
    """parts: (name, got, ref64, ref32[, band_by]).  Prints err, e32 and their ratio of every part
    (per band where band_by, the input magnitudes, is given), then holds each to err <= 4 e32."""
    rows = []
    for part in parts:
        name, got, want, w32 = part[:4]
        got, want, w32 = (torch.as_tensor(t).double().reshape(-1) for t in (got, want, w32))
        assert got.shape == want.shape == w32.shape, (tag, name)
        assert torch.isfinite(got).all(), (tag, name)
        if len(part) == 4:
            rows.append((name, (got - want).abs().max().item(), (w32 - want).abs().max().item()))
            continue
        by = part[4].double().reshape(-1).abs()
        for lo, hi in BANDS:
            sel = (by >= lo) & (by < hi)
            if sel.any():
                rows.append((f"{name}[{lo:g}-{hi:g}]", (got[sel] - want[sel]).abs().max().item(),
                             (w32[sel] - want[sel]).abs().max().item()))
    print(f"TRAIN-OPS {tag}: " + "  ".join(
        f"{n} err {e:.2e} e32 {b:.2e} ratio {(e / b if b > 0 else (0.0 if e == 0 else float('inf'))):.2f}"
        for n, e, b in rows))
    for n, err, e32 in rows:
        assert err <= 4 * e32, (tag, n, err, e32)


class _Pool:
    """Outputs of one or a few elements (a loss, a bias gradient, the statistics of a few rows)
    gathered into one tensor per name over the sizes or draws of ONE input family, so that the
    rule's maxima run over more than a single rounding.  Every larger output is held to the rule
    case by case."""

    def __init__(self):
        self.d = {}

    def add(self, name, *tensors):
        cols = self.d.setdefault(name, [[] for _ in tensors])
        for col, t in zip(cols, tensors):
            col.append(torch.as_tensor(t).double().reshape(-1))

    def parts(self):
        return [(name,) + tuple(torch.cat(col) for col in cols) for name, cols in self.d.items()]


def _keep_mult(M, H):
    from asr_rescoring_amd.train import dropout_keep
    return R.keep_to_mult(dropout_keep(DROP["seed"], DROP["step"], DROP["site"], DROP["p"], M * H), M, H, DROP["p"])


# ---- row ops -------------------------------------------------------------------------------------

VOCAB, TYPES, MAXPOS = 37, 2, 16
TOK = [0, VOCAB - 1, VOCAB + 5, -2, 9, 7, 7, 11, 1]
POS = [0, 1, 2, 3, 6, 15, 4, 0, 1]
TYP = [0, 1, 5, -1, 1, 0, 1, 1, 0]
ROW_M = [1, 3, 4, 5, 9]


@functools.lru_cache(maxsize=None)
def _row_inputs(H, M, family):
    """normal; bigmean (row mean 100, spread ~1e-2); const (the last row constant: variance 0,
    rstd = 1e6; dyadic values, so every sum is exact); gamma (zeros and negative entries)."""
    s = 1000 * H + 10 * M
    word, pos, typ = _randn(VOCAB, H, seed=s + 1), _randn(MAXPOS, H, seed=s + 2, scale=0.5), _randn(TYPES, H, seed=s + 3, scale=0.5)
    g, b = 1.0 + _randn(H, seed=s + 4, scale=0.3), _randn(H, seed=s + 5, scale=0.3)
    y, res, bias = _randn(M, H, seed=s + 6), _randn(M, H, seed=s + 7), _randn(H, seed=s + 8, scale=0.5)
    dy = _randn(M, H, seed=s + 9)
    tok, pidx, ty = torch.tensor(TOK[:M]), torch.tensor(POS[:M]), torch.tensor(TYP[:M])
    if family == "bigmean":
        word, pos, typ = 100.0 + 1e-2 * word, 1e-2 * pos, 1e-2 * typ
        y, res, bias = 100.0 + 1e-2 * y, 1e-2 * res, 1e-2 * bias
    elif family == "const":
        word[3], pos[5], typ[0], typ[1] = 0.5, 0.125, 0.25, -0.5
        tok[M - 1], pidx[M - 1], ty[M - 1] = 3, 5, 1
        bias = torch.randint(-64, 65, (H,), generator=_gen(s)).float() / 64
        y[M - 1], res[M - 1] = 0.5 - bias, 0.25
    elif family == "gamma":
        g = _randn(H, seed=s + 4)
        g[::7] = 0.0
    return dict(word=word, pos=pos, typ=typ, g=g, b=b, y=y, res=res, bias=bias, dy=dy, tok=tok.int(), pidx=pidx.int(),
                ty=ty.int(), mult=_keep_mult(M, H))


def _run_embed(c, M, H, with_type, drop):
    x0, st, h0 = _nan(M, H), _nan(M, 2), _nan(M, H)
    d = DROP if drop else NODROP
    keep = [_g(c[k]) for k in ("tok", "pidx", "ty", "word", "pos", "typ", "g", "b")]
    _ok(_lib.load().rs_debug_train_embed_ln(_p(keep[0]), _p(keep[1]), _p(keep[2]) if with_type else None, M, VOCAB,
                                            TYPES, MAXPOS, _p(keep[3]), _p(keep[4]), _p(keep[5]), _p(keep[6]),
                                            _p(keep[7]), EPS, H, d["seed"], d["step"], d["site"], d["p"], _p(x0),
                                            _p(st), _p(h0), _stream()))
    return x0.cpu(), st.cpu(), h0.cpu()


def _run_bias_res_ln(c, M, H, form):
    """form: "plain" (bias null), "bias", "drop" """
    y, st, h = _g(c["y"]).clone(), _nan(M, 2), _nan(M, H)
    d = DROP if form == "drop" else NODROP
    keep = [_g(c[k]) for k in ("bias", "res", "g", "b")]
    plain = form == "plain"
    _ok(_lib.load().rs_debug_train_bias_res_ln(_p(y), None if plain else _p(keep[0]), None if plain else _p(keep[1]),
                                               M, _p(keep[2]), _p(keep[3]), EPS, H, d["seed"], d["step"], d["site"],
                                               d["p"], _p(st), _p(h), _stream()))
    return y.cpu(), st.cpu(), h.cpu()


def _run_ln_bwd(dy, x, st, g, M, H, alias):
    dyd, keep = _g(dy).clone(), [_g(x), _g(st), _g(g)]
    dx = dyd if alias else _nan(M, H)
    _ok(_lib.load().rs_debug_train_ln_bwd(_p(dyd), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(dx), M, H, _stream()))
    return dx.cpu()


@pytest.mark.parametrize("family", ["normal", "bigmean", "const", "gamma"])
@pytest.mark.parametrize("H", [256, 512, 768, 1024])
def test_row_ops_vs_float64(H, family):
    """Every form of the three row kernels at M = 1, 3, 4, 5, 9 (four rows share a block).  h0, h, y
    and dx are held to the rule at every M; the M means and M rstds of a form are gathered over M."""
    pool, parts = _Pool(), []
    for M in ROW_M:
        c = _row_inputs(H, M, family)
        tag = f"H{H}-M{M}-{family}"
        for with_type, drop in ((True, False), (False, False), (True, True)):
            a = (c["tok"], c["pidx"], c["ty"] if with_type else None, c["word"], c["pos"], c["typ"], c["g"], c["b"], EPS,
                 c["mult"] if drop else None)
            r64, r32 = R.embed_ln(*a, dt=torch.float64), R.embed_ln(*a, dt=torch.float32)
            x0, st, h0 = _run_embed(c, M, H, with_type, drop)
            assert _bits(x0, r32[0]), tag                      # two ordered fp32 adds
            form = f"emb-t{int(with_type)}d{int(drop)}"
            pool.add(f"{form}.mean", st[:, 0], r64[1][:, 0], r32[1][:, 0])
            pool.add(f"{form}.rstd", st[:, 1], r64[1][:, 1], r32[1][:, 1])
            parts.append((f"{form}.h0 M{M}", h0, r64[2], r32[2]))
            if family == "const" and not drop:                 # the constant row: LN gives beta exactly
                assert torch.equal(h0[M - 1], c["b"]) and st[M - 1, 0].item() == (0.125 if with_type else 0.875), tag
        for form in ("plain", "bias", "drop"):
            a = (c["y"], None if form == "plain" else c["bias"], c["res"], c["g"], c["b"], EPS,
                 c["mult"] if form == "drop" else None)
            r64, r32 = R.bias_res_ln(*a, dt=torch.float64), R.bias_res_ln(*a, dt=torch.float32)
            y, st, h = _run_bias_res_ln(c, M, H, form)
            if form == "drop":                                 # (y + bias) * scale + res may contract to an fma
                parts.append((f"ln-drop.y M{M}", y, r64[0], r32[0]))
            else:
                assert _bits(y, r32[0]), (tag, form)
            pool.add(f"ln-{form}.mean", st[:, 0], r64[1][:, 0], r32[1][:, 0])
            pool.add(f"ln-{form}.rstd", st[:, 1], r64[1][:, 1], r32[1][:, 1])
            parts.append((f"ln-{form}.h M{M}", h, r64[2], r32[2]))
            if family == "const" and form == "bias":
                assert torch.equal(h[M - 1], c["b"]) and st[M - 1, 0].item() == 0.75, tag
                assert abs(st[M - 1, 1].item() - 1e6) < 1.0, tag
        # backward from the saved (x, mean, rstd) of the bias + residual form
        x, st64, _ = R.bias_res_ln(c["y"], c["bias"], c["res"], c["g"], c["b"], EPS)
        x, st = x.float(), st64.float()
        dx = _run_ln_bwd(c["dy"], x, st, c["g"], M, H, alias=False)
        parts.append((f"ln_bwd.dx M{M}", dx, R.ln_bwd(c["dy"], x, st, c["g"]),
                      R.ln_bwd(c["dy"], x, st, c["g"], torch.float32)))
        assert _bits(dx, _run_ln_bwd(c["dy"], x, st, c["g"], M, H, alias=True)), tag
    _check(f"rows H{H}-{family}", parts + pool.parts())


# ---- pointwise ops -------------------------------------------------------------------------------

SPECIAL = [0.0, -0.0, 1e-30, -1e-30, 5.5, -5.5, 5.6, -5.6, 6.0, -6.0, 9.0, -9.0, 12.0, -12.0, 3.0, -3.0, 1.0, -1.0]


@functools.lru_cache(maxsize=None)
def _pointwise_inputs(M, N):
    """v = pre + bias dense over about [-13, 13], the bias distinct in every column: a shuffled
    ramp, except +0 in column 0 and -0 in column 1, under which v is exactly 0, -0, 1e-30 and
    -1e-30 (rows 0 and 1), and dyadic k / 64 in the next columns, under which row 0 hits exact 0
    and the values around which erff saturates.  gelu_bwd reads pre itself: every special exactly."""
    n = M * N
    pre = torch.linspace(-12.0, 12.0, n)[torch.randperm(n, generator=_gen(M + N))].float().view(M, N)
    bias = (torch.linspace(-1.0, 1.0, N) * 0.987 + 0.0123)[torch.randperm(N, generator=_gen(N))].float()
    k = len(SPECIAL)
    bias[0], bias[1] = 0.0, -0.0
    bias[2:2 + k] = torch.arange(1, k + 1).float() / 64
    pre[0, 0], pre[0, 1], pre[1, 0], pre[1, 1] = 0.0, -0.0, 1e-30, -1e-30
    pre[0, 2:2 + k] = torch.tensor(SPECIAL) - bias[2:2 + k]
    assert torch.unique(bias).numel() == N - 1 and (pre[0, 2] + bias[2]).item() == 0.0      # +0 == -0
    d = _randn(M, N, seed=M * 7 + N)
    gpre = pre.clone()
    gpre[0, :k] = torch.tensor(SPECIAL)
    refs = {}
    for dt in (torch.float64, torch.float32):
        refs[dt] = R.bias_gelu(pre, bias, dt) + (R.gelu_bwd(d, gpre, dt),)
    return pre, bias, d, gpre, refs


@pytest.mark.parametrize("M,N", [(3, 256), (5, 1024), (2, 3072), (3, 21128), (2731, 3072)])
def test_pointwise_ops_vs_float64(M, N):
    """2731 x 3072: just past 8192 x 256 quads, the grid-stride loops wrap."""
    pre, bias, d, gpre, refs = _pointwise_inputs(M, N)
    r64, r32 = refs[torch.float64], refs[torch.float32]
    L, tag = _lib.load(), f"{M}x{N}"
    a, v, act = _g(pre).clone(), _g(bias), _nan(M, N)
    _ok(L.rs_debug_train_pointwise(0, _p(a), _p(v), _p(act), M, N, _stream()))
    assert _bits(a.cpu(), r32[0]), tag                         # pre + bias: one fp32 add
    assert a.cpu()[0, 1].item() == 0.0 and np.signbit(a.cpu()[0, 1].item())
    _check(f"bias_gelu {tag}", [("act", act.cpu(), r64[1], r32[1], r64[0])])
    y = _g(pre).clone()
    _ok(L.rs_debug_train_pointwise(2, _p(y), _p(v), None, M, N, _stream()))
    assert _bits(y.cpu(), r32[0]), tag
    dd, pp = _g(d).clone(), _g(gpre)
    _ok(L.rs_debug_train_pointwise(1, _p(dd), _p(pp), None, M, N, _stream()))
    _check(f"gelu_bwd {tag}", [("d", dd.cpu(), r64[2], r32[2], gpre)])


# ---- column sums ---------------------------------------------------------------------------------

COL_M = [1, 7, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 2177, 4101]


def _colsum_inputs(M, N, family, seed):
    """normal; cancel (row r + M // 2 cancels row r in dy, with the same x and statistics: every
    column's exact sum is 0 in both modes); bigrow (one row 1e4 times the rest)."""
    dy, x = _randn(M, N, seed=seed), _randn(M, N, seed=seed + 1)
    st = torch.stack([x.double().mean(1), 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-12)], 1).float() \
        if N > 1 else torch.ones(M, 2)
    if family == "cancel":
        h = M // 2
        dy[h:2 * h], x[h:2 * h], st[h:2 * h] = -dy[:h], x[:h], st[:h]
        if M % 2:
            dy[M - 1] = 0.0
    elif family == "bigrow":
        dy[M // 3] *= 1e4
    rtype = (torch.arange(M) * 7 % 5 < 2).int()          # two types mixed (about 2 rows in 5 of type 1)
    return dy, x, st, rtype


def _seq32(a, axis):
    """float32 sum along an axis in index order"""
    a = np.moveaxis(a, axis, 0)
    t = a[0].copy()
    for k in range(1, a.shape[0]):
        t = t + a[k]
    return t


def _pad0(a, k):
    r = (-a.shape[0]) % k
    return np.concatenate([a, np.zeros((r,) + a.shape[1:], np.float32)]) if r else a


def _acc32(d, xh, axis):
    """Per-lane accumulation along an axis in index order from 0: a += d (mode 0), or the kernels'
    a = fmaf(d, xhat, a) (mode 1; the product of two floats is exact in float64)."""
    d = np.moveaxis(d, axis, 0)
    a = np.zeros(d.shape[1:], np.float32)
    if xh is None:
        for k in range(d.shape[0]):
            a = a + d[k]
        return a
    xh = np.moveaxis(xh, axis, 0)
    for k in range(d.shape[0]):
        a = (d[k].astype(np.float64) * xh[k] + a).astype(np.float32)
    return a


def _colsum_model32(dy, x, st, mode, rows=None, out0=None):
    """The column sums in float32 numpy in the kernels' order (an unwanted row adds nothing: +0):
      N % 4 != 0   64-row blocks, accumulator r & 3 in row order, (a0 + a1) + (a2 + a3); then the
                   blocks into accumulator rb & 3 in block order, combined the same way
      M <= 2048    64 row lanes (rows l, l + 64, ... in order), groups of 8 lanes in order, the 8 groups
      M >  2048    128-row blocks of 16 row lanes, two groups of 8 lanes; then the blocks as above"""
    d = dy.numpy()
    M, N = d.shape
    xh = None
    if mode == 1:
        s = st.numpy()
        xh = (x.numpy() - s[:, 0:1]) * s[:, 1:2]
    if rows is not None:
        d = np.where(rows.numpy()[:, None], d, np.float32(0))

    def lanes(k, shape, axis):
        return _acc32(_pad0(d, k).reshape(shape), None if xh is None else _pad0(xh, k).reshape(shape), axis)

    def tree4(acc, axis):
        a = np.moveaxis(acc, axis, 0)
        return (a[0] + a[1]) + (a[2] + a[3])

    def final(part):
        return tree4(_seq32(_pad0(part, 4).reshape(-1, 4, N), 0), 0)

    if N % 4:
        out = final(tree4(lanes(64, (-1, 16, 4, N), 1), 1))
    elif M <= 2048:
        out = _seq32(_seq32(lanes(64, (-1, 64, N), 0).reshape(8, 8, N), 1), 0)
    else:
        red8 = _seq32(lanes(128, (-1, 8, 16, N), 1).reshape(-1, 2, 8, N), 2)
        out = final(red8[:, 0] + red8[:, 1])
    assert out.dtype == np.float32
    return torch.from_numpy(out if out0 is None else out0.numpy() + out)


def _run_colsum(op, dev, M, N, out0=None, accumulate=0, rtype=None, want=0):
    """dev: (dy, x, st) on the device -> out (op 2: (gamma, beta))"""
    out = _nan(N) if out0 is None else _g(out0).clone()
    out_b = _nan(N) if op == 2 else None
    _ok(_lib.load().rs_debug_train_colsum(op, _p(dev[0]), _p(dev[1]), _p(dev[2]), M, N, _p(out), _p(out_b), accumulate,
                                          _p(rtype), want, _stream()))
    return (out.cpu(), out_b.cpu()) if op == 2 else out.cpu()


def _colsum_case(M, N, family, seed):
    """e32 is the float32 numpy model of the kernels' summation order, not torch.sum: torch adds a
    column's rows in row order, the kernels in interleaved accumulators and a fixed tree, and with
    a handful of rows that partly cancel torch's float32 sum can be exact where the kernel's order
    rounds once (7 x 30, rows 0, 3, 5 of type 1 with dy[3] = -dy[0]: torch gets dy[5] exactly, the
    kernel (dy[0] + dy[5]) - dy[0]; err 1.2e-7 against e32 = 0).  Against torch.sum every other case
    measured err / e32 <= 2.6.  Mode 1 accumulates with the kernels' fmaf(dy, xhat, a): where a
    lane's rows cancel (128 x 768, rows r and r + 64) the fused form leaves the product's rounding,
    7e-7, and an unfused multiply and add exactly 0."""
    dy, x, st, rtype = _colsum_inputs(M, N, family, seed)
    dev, rt = (_g(dy), _g(x), _g(st)), _g(rtype)
    out0 = _randn(N, seed=seed + 2)
    tag, parts = f"{M}x{N}-{family}", []
    plain = {}
    for mode in (0, 1):
        got = plain[mode] = _run_colsum(mode, dev, M, N)
        parts.append((f"m{mode}", got, R.colsum(dy, x, st, mode), _colsum_model32(dy, x, st, mode)))
        assert _bits(got, _run_colsum(mode, dev, M, N)), (tag, "two runs")
        acc = _run_colsum(mode, dev, M, N, out0=out0, accumulate=1)
        parts.append((f"m{mode}+acc", acc, R.colsum(dy, x, st, mode, out0=out0),
                      _colsum_model32(dy, x, st, mode, out0=out0)))
        sel = rtype == 1
        got = _run_colsum(mode, dev, M, N, rtype=rt, want=1)
        parts.append((f"m{mode}+type", got, R.colsum(dy, x, st, mode, rows=sel), _colsum_model32(dy, x, st, mode, rows=sel)))
        one = _g(torch.full((M,), 3, dtype=torch.int32))
        assert _bits(_run_colsum(mode, dev, M, N, rtype=one, want=3), plain[mode]), (tag, "all rows of one type")
        none = _run_colsum(mode, dev, M, N, rtype=one, want=2)
        assert (none.view(torch.int32) == 0).all(), (tag, "a type without rows")
    gam, bet = _run_colsum(2, dev, M, N)
    assert _bits(gam, plain[1]) and _bits(bet, plain[0]), (tag, "tr_colsum_ln == the two tr_colsum calls")
    _check(f"colsum {tag}", parts)


@pytest.mark.parametrize("N", [20, 256, 768, 1000, 3072, 30, 1001])
def test_column_sums_vs_float64(N):
    """Every M around the 64- / 128-row blocks and kOnePass = 2048; N % 4 != 0 (30, 1001): the narrow form."""
    for M in COL_M:
        _colsum_case(M, N, "normal", 100 * N + M)


@pytest.mark.parametrize("M", [2047, 2048, 2049])
def test_column_sums_vocab_wide(M):
    _colsum_case(M, 21128, "normal", M)


@pytest.mark.parametrize("family", ["cancel", "bigrow"])
@pytest.mark.parametrize("N", [768, 30])
def test_column_sums_input_families(N, family):
    for M in COL_M:
        _colsum_case(M, N, family, 7 * N + M)


# ---- embedding gradients -------------------------------------------------------------------------

@pytest.mark.parametrize("H", [256, 768])
def test_embedding_gradients_vs_float64(H):
    lens, vocab = [5, 1, 9, 3], 23                          # position 8: one sequence only
    M, tmax = sum(lens), max(lens)
    tok = torch.tensor([4, 0, 7, 4, 22, 4, 9, 0, 7, 7, 1, 0, 22, 3, 4, 5, 4, 2])
    assert tok.numel() == M
    dx0, dword0, dpos0 = _randn(M, H, seed=H), _randn(vocab, H, seed=H + 1), _randn(tmax, H, seed=H + 2)
    utok = torch.unique(tok)
    rows = [torch.nonzero(tok == u).flatten() for u in utok]
    toff = torch.tensor(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), dtype=torch.int32)
    L = _lib.load()
    keep = [_g(dx0), _g(utok.int()), _g(toff), _g(torch.cat(rows).int())]
    dword = _g(dword0).clone()
    _ok(L.rs_debug_train_word_grad(_p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), len(utok), M, vocab, H,
                                   _p(dword), _stream()))
    dword = dword.cpu()
    untouched = [i for i in range(vocab) if i == 0 or i not in tok.tolist()]
    assert _bits(dword[untouched], dword0[untouched])         # the pad id and the absent ids: left as they were
    off = _g(torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32))
    dpos = _g(dpos0).clone()
    _ok(L.rs_debug_train_pos_grad(_p(keep[0]), _p(off), len(lens), M, tmax, H, _p(dpos), _stream()))
    _check(f"embed_grad H{H}", [
        ("dword", dword, R.word_grad(dx0, tok, dword0), R.word_grad(dx0, tok, dword0, torch.float32)),
        ("dpos", dpos.cpu(), R.pos_grad(dx0, lens, dpos0), R.pos_grad(dx0, lens, dpos0, torch.float32))])


# ---- CLS head ------------------------------------------------------------------------------------

CLS_LENS = [3, 1, 5, 2, 4, 1, 7, 2, 6]


@pytest.mark.parametrize("H", [256, 768])
def test_cls_head_vs_float64(H):
    """S = 1, 3, 4, 5, 9 sequences (four share a block of the forward).  dw is held to the rule at
    every S; the S scores and the one db are gathered over S."""
    L, pool, parts = _lib.load(), _Pool(), []
    for S in (1, 3, 4, 5, 9):
        lens = CLS_LENS[:S]
        M = sum(lens)
        offs = np.concatenate([[0], np.cumsum(lens)])
        rows = torch.tensor(offs[:-1])
        h, w, b = _randn(M, H, seed=H + S), _randn(H, seed=H + S + 1, scale=0.1), _randn(1, seed=S)
        dsc, dw0, db0 = _randn(S, seed=S + 2), _randn(H, seed=S + 3), _randn(1, seed=S + 4)
        keep = [_g(h), _g(torch.tensor(offs, dtype=torch.int32)), _g(w), _g(b), _g(dsc)]
        out = _nan(S)
        _ok(L.rs_debug_train_cls_fwd(_p(keep[0]), _p(keep[1]), S, M, H, _p(keep[2]), _p(keep[3]), _p(out), _stream()))
        dh, dw, db = torch.zeros(M, H, device=_dev()), _g(dw0).clone(), _g(db0).clone()
        _ok(L.rs_debug_train_cls_bwd(_p(keep[4]), _p(keep[0]), _p(keep[1]), S, M, H, _p(keep[2]), _p(dh), _p(dw),
                                     _p(db), _stream()))
        r64, r32 = R.cls_bwd(dsc, h, rows, w, dw0, db0), R.cls_bwd(dsc, h, rows, w, dw0, db0, torch.float32)
        assert _bits(dh.cpu(), r32[0]), (H, S)                  # one product at the CLS rows, +0 elsewhere
        pool.add("score", out.cpu(), R.cls_fwd(h, rows, w, b), R.cls_fwd(h, rows, w, b, torch.float32))
        parts.append((f"dw S{S}", dw.cpu(), r64[1], r32[1]))
        pool.add("db", db.cpu(), r64[2], r32[2])
    _check(f"cls H{H}", parts + pool.parts())


# ---- distillation losses -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loss_inputs(n_utt, family, seed):
    """Group sizes ragged 1..16 with one empty group in the middle.  normal; eqmix (mixed scores
    s + am equal within a group, dyadic so exactly); sharp (AM -200 +- 30); eqcer (CER equal
    within a group).  CER >= 0.05 everywhere."""
    sizes = [1 + (5 * u + 6 + 3 * seed) % 16 for u in range(n_utt)]
    if n_utt >= 3:
        sizes[n_utt // 2] = 0
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n, s = int(off[-1]), 10 * n_utt + 1000 * seed
    sc, tgt = _randn(n, seed=s, scale=2.0), _randn(n, seed=s + 1, scale=2.0)
    am = -20.0 + _randn(n, seed=s + 2, scale=3.0)            # log-likelihoods: sum c stays far from 0 (MWED's T)
    cer = torch.rand(n, generator=_gen(s + 3)).float() * 0.6 + 0.05
    grp = torch.repeat_interleave(torch.arange(n_utt), torch.tensor(sizes))
    if family == "eqmix":
        sc = torch.round(sc * 8) / 8
        am = 1.0 + (grp % 5).float() * 0.5 - sc                # never 0: MWED divides by T = sum c / sum e
    elif family == "sharp":
        am = -200.0 + 30.0 * _randn(n, seed=s + 4)
    elif family == "eqcer":
        cer = cer[torch.tensor(off[:-1]).long().clamp(max=n - 1)][grp]
    return sc, tgt, am, cer, off


def _seq_sum32(v):
    """A float32 sum in index order."""
    v = np.asarray(v, dtype=np.float32)
    return np.cumsum(v, dtype=np.float32)[-1] if v.size else np.float32(0)


@pytest.mark.parametrize("family", ["normal", "eqmix", "sharp", "eqcer"])
@pytest.mark.parametrize("kind", ["MD", "MD_MWER", "MD_MWED"])
@pytest.mark.parametrize("n_utt", [1, 5, 300])
def test_losses_vs_float64(n_utt, kind, family):
    """Several draws of one family.  dsc is held to the rule draw by draw, and so are the 300
    per-utterance losses; the one or five per-utterance losses and the total are gathered over
    the draws: 16 of the one- and five-utterance shapes, 4 of the 300-utterance shape.  (A maximum
    over 4 scalars is not yet the float32 error of the expression: MD_MWED's group loss carries
    log Q of a thrice-rounded Q, about 2e-7, and four draws of the float32 reference happened to
    stay under 5e-8 where the kernel's four reached 2.1e-7.  Over 16 draws the chance that the
    reference's largest error is under a quarter of an equally accurate kernel's is below 1e-6.)

    The total's e32 is a float32 numpy model, not torch's sum: thread 0 of tr_loss_kernel adds the
    n_hyp squared differences, then the n_utt group losses, in index order (a chain as deep as the
    batch), where torch.sum adds pairwise in blocks; the model is those two index-order float32
    sums over the float32 reference's terms.  The figure against torch's sum is printed beside it.

    MD_MWED's dsc: the reference adds dz / T and dT / sum e to 2 w (s - t) one after the other, as
    the kernel does (two roundings at the size of the MD term, up to 4.8e-7 at |dsc| in [4, 8));
    added to each other first they round there once, and err / e32 reached 4.9 with two
    hypotheses (5.6e-7 against 1.1e-7; a float32 model of the kernel's order gave the kernel's
    5.586e-7 to every digit)."""
    md_w, pool, parts, torch_model = 0.5, _Pool(), [], [0.0, 0.0]
    for seed in range(4 if n_utt == 300 else 16):
        sc, tgt, am, cer, off = _loss_inputs(n_utt, family, seed)
        n = sc.numel()
        keep = [_g(t) for t in (sc, tgt, am, cer, torch.from_numpy(off))]
        dsc, ul, loss = _nan(n), _nan(n_utt), _nan(1)
        _ok(_lib.load().rs_debug_train_loss(*(_p(t) for t in keep), n_utt, n, R.LOSS_KINDS[kind], md_w, _p(dsc),
                                            _p(ul), _p(loss), _stream()))
        r64 = R.losses(sc, tgt, am, cer, off, kind, md_w)
        r32 = R.losses(sc, tgt, am, cer, off, kind, md_w, torch.float32)
        md32 = _seq_sum32(((sc - tgt) ** 2).numpy())
        tot32 = md32 if kind == "MD" else np.float32(_seq_sum32(r32[1].numpy()) + np.float32(md_w) * md32)
        parts.append((f"dsc#{seed}", dsc.cpu(), r64[0], r32[0]))
        if kind != "MD":                                       # MD writes no per-utterance losses
            if n_utt == 300:
                parts.append((f"uloss#{seed}", ul.cpu(), r64[1], r32[1]))
            else:
                pool.add("uloss", ul.cpu(), r64[1], r32[1])
        pool.add("loss", loss.cpu(), r64[2], float(tot32))
        torch_model[0] = max(torch_model[0], abs(loss.item() - r64[2].item()))
        torch_model[1] = max(torch_model[1], abs(r32[2].item() - r64[2].item()))
    print(f"TRAIN-OPS loss {kind} n{n_utt} {family}: total against torch.sum err {torch_model[0]:.2e} "
          f"e32 {torch_model[1]:.2e}")
    _check(f"loss {kind} n{n_utt} {family}", parts + pool.parts())


# ---- cross-entropy -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ce_inputs(M, V, family):
    x = _randn(M, V, seed=V + M)
    lab = torch.tensor([V - 1] if M == 1 else [0, V - 1, V // 2, -100, 1])
    used = lab.clamp(0, V - 1)
    if family == "spread":
        x = (torch.rand(M, V, generator=_gen(V)).float() - 0.5) * 60.0
    elif family == "peak-label":
        x[torch.arange(M), used] += 40.0
    elif family == "peak-other":
        x[torch.arange(M), (used + 3) % V] += 40.0
    return x, lab.int(), R.ce(x, lab), R.ce(x, lab, torch.float32)


@pytest.mark.parametrize("family", ["normal", "spread", "peak-label", "peak-other"])
@pytest.mark.parametrize("V", [8, 257, 1000, 21128])
def test_cross_entropy_vs_float64(V, family):
    """M = 1 and 5 rows of one family: normal logits; spread over +-30; one logit 40 above the rest
    at the label (the gradient there is the cancellation p - 1: the absolute rule applies) or
    away from it.  The in-place d-logits are held to the rule at each M in bands of |logit|; the
    six row losses and the two means are gathered over M."""
    pool, parts = _Pool(), []
    for M in (1, 5):
        x, lab, r64, r32 = _ce_inputs(M, V, family)
        logits, labels, rl, loss = _g(x).clone(), _g(lab), _nan(M), _nan(1)
        _ok(_lib.load().rs_debug_train_ce(_p(logits), _p(labels), M, V, _p(rl), _p(loss), _stream()))
        pool.add("row", rl.cpu(), r64[0], r32[0])
        pool.add("mean", loss.cpu(), r64[1], r32[1])
        parts.append((f"dlogits M{M}", logits.cpu(), r64[2], r32[2], x))
    _check(f"ce V{V} {family}", parts + pool.parts())


# ---- AdamW ---------------------------------------------------------------------------------------

ADAM_BIG = 8192 * 256 * 4 + 403          # wraps the quad loop, leaves a 3-element scalar tail
HP = dict(beta1=R.f32(0.9), beta2=R.f32(0.999), eps=R.f32(1e-8))


@functools.lru_cache(maxsize=None)
def _adam_inputs(n, lr, wd):
    p0 = _randn(n, seed=n % 1000 + 1)
    grads = []
    for k in range(3):
        g = _randn(n, seed=n % 1000 + 10 + k) * 10.0 ** torch.randint(-12, 4, (n,), generator=_gen(k)).float()
        g[k::5] = 0.0                                          # exact zeros
        grads.append(g.float())
    hp = dict(lr=R.f32(lr), wd=R.f32(wd), **HP)
    return p0, grads, R.adamw_torch(p0, grads, dt=torch.float64, **hp), R.adamw_torch(p0, grads, dt=torch.float32, **hp)


def _adam_run(p0, grads, lr, wd, offset):
    """Three steps with carried moments; offset 1: every buffer starts one float past a 16-B
    boundary, which takes the scalar kernel."""
    n = p0.numel()
    bufs = [torch.zeros(n + 4, device=_dev()) for _ in range(4)]
    p, g, m, v = (b[offset:offset + n] for b in bufs)
    assert p.data_ptr() % 16 == 4 * offset
    p.copy_(p0)
    out = []
    for k, gk in enumerate(grads):
        g.copy_(gk)
        _ok(_lib.load().rs_debug_train_adamw(_p(p), _p(g), _p(m), _p(v), n, lr, HP["beta1"], HP["beta2"], HP["eps"],
                                             wd, k + 1, _stream()))
        out.append((p.cpu().clone(), m.cpu().clone(), v.cpu().clone()))
    return out


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("lr", [1e-3, 2e-5])
@pytest.mark.parametrize("ns", [(1, 3, 4, 5, 7), (1025,), (ADAM_BIG,)])
def test_adamw_vs_torch(ns, lr, wd):
    """p, m, v after each of three steps, held to the rule per size; only the five sizes around one
    quad (1 to 7 elements, the same hyper-parameters and input family) are gathered.  Then the
    same run on buffers one float off a 16-B boundary (the scalar kernel): bit for bit the same."""
    pool = _Pool()
    for n in ns:
        p0, grads, r64, r32 = _adam_inputs(n, lr, wd)
        got = _adam_run(p0, grads, lr, wd, 0)
        for k in range(3):
            for i, what in enumerate("pmv"):
                pool.add(f"{what}{k + 1}", got[k][i], r64[k][i], r32[k][i])
        scalar = _adam_run(p0, grads, lr, wd, 1)
        for k in range(3):
            for i in range(3):
                assert _bits(got[k][i], scalar[k][i]), ("float4 kernel != scalar kernel", n, k, "pmv"[i])
    _check(f"adamw n{ns[0]} lr{lr:g} wd{wd:g}", pool.parts())


# ---- row moves -----------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [256, 768])
def test_row_moves_are_exact(H):
    M, rows = 11, torch.tensor([10, 0, 4, 7, 2])
    n = rows.numel()
    x = _randn(M, H, seed=H)
    inv = torch.full((M,), -1, dtype=torch.int32)
    inv[rows] = torch.arange(n, dtype=torch.int32)
    L = _lib.load()
    src, idx, dst = _g(x), _g(rows.int()), _nan(n, H)
    _ok(L.rs_debug_train_move_rows(0, _p(src), _p(idx), n, M, H, _p(dst), _stream()))
    assert _bits(dst.cpu(), R.gather_rows(x, rows))
    back, dinv = _nan(M, H), _g(inv)
    _ok(L.rs_debug_train_move_rows(1, _p(dst), _p(dinv), n, M, H, _p(back), _stream()))
    back = back.cpu()
    assert _bits(back, R.expand_rows(R.gather_rows(x, rows), inv, M))
    rest = [r for r in range(M) if r not in rows.tolist()]
    assert _bits(back[rows], x[rows]) and (back[rest].view(torch.int32) == 0).all()


# ---- argument checks -----------------------------------------------------------------------------

def test_entries_refuse_bad_arguments():
    L, s = _lib.load(), _stream()
    a, v, idx = _g(torch.zeros(4, 256)), _g(torch.zeros(256)), _g(torch.tensor([0, 1, 2, 99], dtype=torch.int32))
    st = _g(torch.ones(4, 2))
    assert L.rs_debug_train_ln_bwd(_p(a), _p(a), _p(st), _p(v), _p(a), 4, 300, s) == RS_EUNSUP
    assert L.rs_debug_train_ln_bwd(_p(a), None, _p(st), _p(v), _p(a), 4, 256, s) == RS_EARG
    assert L.rs_debug_train_pointwise(0, _p(a), _p(v), _p(a), 4, 30, s) == RS_EUNSUP
    assert L.rs_debug_train_pointwise(3, _p(a), _p(v), _p(a), 4, 256, s) == RS_EARG
    assert L.rs_debug_train_colsum(2, _p(a), _p(a), _p(st), 4, 256, _p(v), _p(v), 1, None, 0, s) == RS_EARG
    assert L.rs_debug_train_colsum(1, _p(a), None, None, 4, 256, _p(v), None, 0, None, 0, s) == RS_EARG
    # row_pos 99 is outside max_pos = 16: refused on the host, never dereferenced
    assert L.rs_debug_train_embed_ln(_p(idx), _p(idx), None, 4, 37, 2, 16, _p(a), _p(a), _p(a), _p(v), _p(v), EPS, 256,
                                     0, 0, 0, 0.0, _p(a), _p(st), _p(a), s) == RS_EARG
    assert b"row_pos" in L.rs_last_error()
    assert L.rs_debug_train_move_rows(0, _p(a), _p(idx), 4, 4, 256, _p(a), s) == RS_EARG
    assert L.rs_debug_train_adamw(_p(v), _p(v), _p(v), _p(v), 256, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, s) == RS_EARG
    assert L.rs_debug_train_loss(_p(v), _p(v), _p(v), _p(v), _p(idx), 3, 256, 7, 0.5, _p(v), _p(v), _p(v), s) == RS_EARG
