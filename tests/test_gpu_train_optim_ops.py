"""The kernels behind gradient accumulation, clipping and the scaled AdamW step (csrc/k_train.hip:
tr_sumsq, tr_accum, tr_adamw_scaled) through their ``rs_debug_train_*`` entries, which call the
launchers ``train_api.hip`` calls.

Bounds, all derived:
  * norm: each fp32 square is exact in float64, so kernel and numpy differ only in the order of a
    float64 sum of n <= 1e6 non-negative terms, at most n * 2^-53 ~ 1.1e-10 relative: 1e-9.
  * accumulate: ``fmaf(w, g, acc)`` in fp32 is the exact product (exact in float64, 48 bits) plus acc,
    rounded once to fp32.  numpy's float64 ``w * g + acc`` rounds that sum to float64 first, which can
    differ from the single rounding only on a double-rounding tie; such inputs are left out of the
    bitwise comparison (none may be left out at weight 1, where the product is g itself).
  * scaled AdamW: the project's rule, max|out - ref64| <= 4 * e32 (tests/test_gpu_train_ops.py)."""
import functools

import numpy as np
import pytest
import torch

import train_ops_ref as R
from asr_rescoring_amd import _lib

pytestmark = pytest.mark.gpu

RS_EARG = -1
HP = dict(beta1=R.f32(0.9), beta2=R.f32(0.999), eps=R.f32(1e-8))
SUMSQ_GRID = 512 * 256                    # k_train.hip kSumsqBlocks blocks of 256 threads


def _dev():
    return torch.device("cuda", 0)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc):
    assert rc == 0, _lib.load().rs_last_error()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(n, seed, scale=1.0):
    return (torch.randn(n, generator=_gen(seed)) * scale).float()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _i64(v):
    return np.ascontiguousarray(v, np.int64)


def _sumsq(buf, ranges):
    """rs_debug_train_sumsq over (offset, count) ranges of a device buffer -> python float."""
    off, cnt = _i64([r[0] for r in ranges]), _i64([r[1] for r in ranges])
    out = np.full(1, np.nan, np.float64)
    _ok(_lib.load().rs_debug_train_sumsq(_p(buf), off.ctypes.data, cnt.ctypes.data, len(ranges), buf.numel(),
                                         out.ctypes.data, _stream()))
    return float(out[0])


def _norm64(x):
    return float(np.sqrt(np.sum(x.astype(np.float64) ** 2)))


# ---- gradient norm -------------------------------------------------------------------------------

# around one quad and one wave, several blocks, and one element past the grid's one-item-per-thread
# coverage of each form (quads on a 16-B aligned buffer, single floats one float off it)
NORM_SIZES = [1, 3, 4, 5, 63, 64, 65, 1025, 4 * SUMSQ_GRID + 5]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_matches_float64(n, offset):
    if offset and n > SUMSQ_GRID + 1:
        n = SUMSQ_GRID + 1
    g = _randn(n, seed=n % 997 + 3 * offset) * 10.0 ** torch.randint(-6, 4, (n,), generator=_gen(n % 13)).float()
    buf = torch.full((n + 8,), float("inf"), device=_dev())       # anything read outside the range shows
    buf[offset:offset + n].copy_(g)
    assert buf.data_ptr() % 16 == 0
    got = np.sqrt(_sumsq(buf, [(offset, n)]))
    want = _norm64(g.numpy())
    print(f"NORM n{n} off{offset}: got {got!r} want {want!r} rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-9 * want
    assert np.sqrt(_sumsq(buf, [(offset, n)])) == got               # the same bits on a second run


def test_norm_over_two_ranges_skips_the_gap():
    n = 3000
    g = _randn(n, seed=5)
    buf = g.to(_dev())
    a, b = (0, 1024), (1088, n - 1088)
    buf[1024:1088] = torch.tensor([float("nan"), float("inf"), 1e30, -1e30] * 16, device=_dev())   # poison
    got = _sumsq(buf, [a, b])
    x = g.numpy()
    want = _norm64(np.concatenate([x[:1024], x[1088:]]))
    assert np.isfinite(got) and abs(np.sqrt(got) - want) <= 1e-9 * want
    assert _sumsq(buf, [a, b]) == got
    # unaligned ranges with odd counts inside one buffer
    got = _sumsq(buf, [(1, 5), (1091, 63)])
    want = _norm64(np.concatenate([x[1:6], x[1091:1154]]))
    assert abs(np.sqrt(got) - want) <= 1e-9 * want


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("where", [0, 777, 4100])
def test_norm_of_a_non_finite_buffer_is_non_finite(bad, where):
    buf = _randn(4101, seed=2).to(_dev())
    buf[where] = bad
    assert not np.isfinite(_sumsq(buf, [(0, 4101)]))


def test_range_lists_are_checked():
    L = _lib.load()
    buf = torch.zeros(256, device=_dev())
    out = np.zeros(1, np.float64)
    for off, cnt in ([0], [257]), ([200], [57]), ([-1], [4]), ([0], [0]):
        o, c = _i64(off), _i64(cnt)
        assert L.rs_debug_train_sumsq(_p(buf), o.ctypes.data, c.ctypes.data, 1, 256, out.ctypes.data, _stream()) == RS_EARG
        assert L.rs_debug_train_accum(_p(buf), _p(buf), o.ctypes.data, c.ctypes.data, 1, 256, 1.0, _stream()) == RS_EARG
    assert L.rs_debug_train_adamw_scaled(_p(buf), _p(buf), _p(buf), _p(buf), 256, 0.5, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0,
                                         _stream()) == RS_EARG


# ---- accumulate ----------------------------------------------------------------------------------

def _fma32(w, g, acc):
    """fp32 fmaf(w, g, acc) through float64, and where that emulation is exact: the float64 sum of
    the (exact) product and acc was itself exact, or its rounding to fp32 is not a tie."""
    prod = np.float64(np.float32(w)) * g.astype(np.float64)              # exact: 24 x 24 bits
    s = prod + acc.astype(np.float64)
    # the float64 addition was exact iff the two-sum error term is zero
    bb = s - prod
    err = (prod - (s - bb)) + (acc.astype(np.float64) - bb)
    out = s.astype(np.float32)
    up = np.nextafter(out, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(out, np.float32(-np.inf)).astype(np.float64)
    tie = (np.abs(s - out.astype(np.float64)) == np.abs(up - s)) | (np.abs(s - out.astype(np.float64)) == np.abs(s - dn))
    return out, (err == 0.0) | ~tie


@pytest.mark.parametrize("offset", [0, 1])
def test_accumulate_is_the_fp32_fma_chain(offset):
    n = 2500
    a, b = (offset, 1027), (1200 + offset, n - 1200 - offset - 3)
    weights = (1.0, 0.5, 3.0)
    grads = [_randn(n, seed=20 + k) * 10.0 ** torch.randint(-3, 3, (n,), generator=_gen(k)).float() for k in range(3)]
    poison = torch.full((n,), -77.25)
    acc = poison.clone().to(_dev())
    for lo, cnt in (a, b):
        acc[lo:lo + cnt] = 0.0
    off, cnt = _i64([a[0], b[0]]), _i64([a[1], b[1]])
    want = np.zeros(n, np.float32)
    exact = np.ones(n, bool)
    for w, g in zip(weights, grads):
        gd = g.to(_dev())
        _ok(_lib.load().rs_debug_train_accum(_p(acc), _p(gd), off.ctypes.data, cnt.ctypes.data, 2, n, w, _stream()))
        want, ok = _fma32(w, g.numpy(), want)
        if w == 1.0:
            assert ok.all()                    # fmaf(1, g, acc) is a plain add: nothing may be left out
        exact &= ok
    got = acc.cpu().numpy()
    inside = np.zeros(n, bool)
    for lo, c in (a, b):
        inside[lo:lo + c] = True
    print(f"ACCUM off{offset}: compared {int((inside & exact).sum())} of {int(inside.sum())}")
    assert exact.mean() > 0.99
    sel = inside & exact
    assert np.array_equal(got[sel].view(np.int32), want[sel].view(np.int32))
    assert np.array_equal(got[~inside], poison.numpy()[~inside])          # gaps untouched
    # the few left out are still the chain to one ulp
    rest = inside & ~exact
    assert np.all(np.abs(got[rest] - want[rest]) <= np.abs(np.spacing(want[rest])))


# ---- scaled AdamW --------------------------------------------------------------------------------

def _adam_run(p0, grads, gmul, lr, wd, offset, scaled=True):
    n = p0.numel()
    bufs = [torch.zeros(n + 4, device=_dev()) for _ in range(4)]
    p, g, m, v = (b[offset:offset + n] for b in bufs)
    assert p.data_ptr() % 16 == 4 * offset
    p.copy_(p0)
    out = []
    L = _lib.load()
    for k, gk in enumerate(grads):
        g.copy_(gk)
        if scaled:
            _ok(L.rs_debug_train_adamw_scaled(_p(p), _p(g), _p(m), _p(v), n, gmul, lr, HP["beta1"], HP["beta2"],
                                              HP["eps"], wd, k + 1, _stream()))
        else:
            _ok(L.rs_debug_train_adamw(_p(p), _p(g), _p(m), _p(v), n, lr, HP["beta1"], HP["beta2"], HP["eps"], wd,
                                       k + 1, _stream()))
        out.append((p.cpu().clone(), m.cpu().clone(), v.cpu().clone()))
    return out


@functools.lru_cache(maxsize=None)
def _adam_inputs(n):
    p0 = _randn(n, seed=n % 1000 + 1)
    grads = []
    for k in range(3):
        g = _randn(n, seed=n % 1000 + 10 + k) * 10.0 ** torch.randint(-12, 4, (n,), generator=_gen(k)).float()
        g[k::5] = 0.0
        grads.append(g.float())
    return p0, grads


@pytest.mark.parametrize("n", [5, 1025])
def test_scaled_adamw_with_unit_scale_is_the_plain_step(n):
    p0, grads = _adam_inputs(n)
    for offset in (0, 1):
        a = _adam_run(p0, grads, 1.0, 1e-3, 0.01, offset)
        b = _adam_run(p0, grads, 1.0, 1e-3, 0.01, offset, scaled=False)
        assert all(_bits(x, y) for ka, kb in zip(a, b) for x, y in zip(ka, kb))


ADAM_BIG = 8192 * 256 * 4 + 403          # wraps the quad loop, leaves a 3-element scalar tail


@pytest.mark.parametrize("n, gmul", [(1025, 0.25), (1025, 1.0 / 3.0), (1025, 1e-3), (ADAM_BIG, 1.0 / 3.0)])
def test_scaled_adamw_vs_torch(n, gmul):
    """Three steps against torch.optim.AdamW in float64 fed gmul * g formed in float64 from the fp32
    gmul (e32: the same in fp32), and float4 kernel == scalar kernel bit for bit."""
    lr, wd = 1e-3, 0.01
    p0, grads = _adam_inputs(n)
    g32 = np.float32(gmul)
    hp = dict(lr=R.f32(lr), wd=R.f32(wd), **HP)
    r64 = R.adamw_torch(p0, [g.double() * float(g32) for g in grads], dt=torch.float64, **hp)
    r32 = R.adamw_torch(p0, [g * torch.tensor(g32) for g in grads], dt=torch.float32, **hp)
    got = _adam_run(p0, grads, float(g32), lr, wd, 0)
    scalar = _adam_run(p0, grads, float(g32), lr, wd, 1)
    for k in range(3):
        for i, what in enumerate("pmv"):
            err = (got[k][i].double() - r64[k][i].double()).abs().max().item()
            e32 = (r32[k][i].double() - r64[k][i].double()).abs().max().item()
            print(f"ADAMW-SCALED n{n} gmul{gmul:g} {what}{k + 1}: err {err:.2e} e32 {e32:.2e}")
            assert torch.isfinite(got[k][i]).all()
            assert err <= 4 * e32, (what, k, err, e32)
            assert _bits(got[k][i], scalar[k][i]), ("float4 kernel != scalar kernel", what, k)
