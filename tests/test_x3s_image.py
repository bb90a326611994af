"""CPU: the helpers of tests/x3s_image.py — the two-part image round trip, the float64 LayerNorm
reference, and the range of every input family of tests/test_gpu_lnres.py (operands and reference
outputs must stay inside the fp16 range of the images, or the GPU tests would compare overflow)."""
import pytest
import torch

from x3s_image import (FAMILIES, FP16_MAX, LN_EPS, _split2, _unsplit2, ln_ref64, lnres_operands, lnres_ref32,
                       lnres_ref64)


def test_image_round_trip():
    """hi = RNE16(v), lo = RNE16(64 (v - hi)): |v - hi| <= 2^-11 |v| (half an ulp of 11 significant
    bits), and lo keeps that remainder to 2^-11 again, so |v - (hi + lo/64)| <= 2^-22 |v| while
    hi and lo are normal fp16 numbers.  lo = 64 (v - hi) is normal for 64 * 2^-11 |v| >= 2^-14, and
    below that its absolute error is the subnormal half-spacing 2^-25 / 64; v from 2^-6 to 3e4
    (signs mixed) keeps the relative bound."""
    g = torch.Generator().manual_seed(1)
    mag = torch.exp2(torch.rand(64, 1024, generator=g) * 21 - 6)           # 2^-6 .. 2^15
    v = mag * torch.where(torch.rand(64, 1024, generator=g) < 0.5, -1.0, 1.0)
    v[0, :4] = torch.tensor([1.0, -0.333251953125, 30000.0, 2.0 ** -6])
    img = _split2(v)
    assert img.dtype == torch.float16 and img.shape == (64, 2048)
    assert torch.isfinite(img).all()
    back = _unsplit2(img, torch.float64)
    err = (back - v.double()).abs()
    assert (err <= 2.0 ** -22 * v.double().abs()).all(), (err / v.double().abs()).max().item()
    # the fp32 decoding differs from the exact one by at most one fp32 rounding
    assert ((_unsplit2(img).double() - back).abs() <= 2.0 ** -24 * back.abs()).all()


def test_image_layout():
    x = torch.arange(2 * 64, dtype=torch.float32).view(2, 64) + 0.25
    img = _split2(x)
    assert torch.equal(img[0, :32].float(), x[0, :32].half().float())          # hi of columns 0..31
    assert torch.equal(img[0, 32:64].float(), ((x[0, :32] - x[0, :32].half().float()) * 64).half().float())
    assert torch.equal(img[0, 64:96].float(), x[0, 32:].half().float())        # hi of columns 32..63
    assert torch.equal(_unsplit2(img, torch.float64), x.double())


@pytest.mark.parametrize("shape", [(7, 256), (3, 768), (2, 5, 1024)])
def test_ln_ref64_matches_torch(shape):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(*shape, generator=g, dtype=torch.float64) * 3 + 5
    w = torch.randn(shape[-1], generator=g, dtype=torch.float64)
    b = torch.randn(shape[-1], generator=g, dtype=torch.float64)
    for eps in (1e-12, 1e-5):
        got = ln_ref64(x, w.float(), b.float(), eps)          # fp32 parameters, as the GPU tests pass them
        ref = torch.nn.functional.layer_norm(x, (shape[-1],), w.float().double(), b.float().double(), eps)
        assert got.dtype == torch.float64
        assert (got - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())


def test_ln_ref64_constant_row():
    """variance exactly 0: the output is beta, finite (rstd = 1 / sqrt(eps))."""
    x = torch.full((2, 256), 0.5, dtype=torch.float64)
    b = torch.linspace(-1, 1, 256)
    y = ln_ref64(x, torch.ones(256), b, LN_EPS)
    assert torch.equal(y, b.double().expand(2, 256))


@pytest.mark.parametrize("N,K", [(768, 768), (1024, 256)])
@pytest.mark.parametrize("family", FAMILIES)
def test_family_ranges(family, N, K):
    """Every operand image and the float64 reference output of every family: finite and below the
    fp16 range (6e4) in magnitude; the fp32 yardstick finite too."""
    M = 512
    op = lnres_operands(family, M, N, K, seed=3)
    for name in ("A2", "W2", "h2"):
        t = op[name]
        assert t.dtype == torch.float16 and torch.isfinite(t).all(), name
        assert t.abs().max().item() < FP16_MAX, (name, t.abs().max().item())
    for name in ("b", "g", "beta"):
        assert op[name].dtype == torch.float32 and op[name].shape == (N,), name
        assert torch.isfinite(op[name]).all() and op[name].abs().max().item() < FP16_MAX, name
    y = lnres_ref64(op["A2"], op["W2"], op["b"], op["h2"], op["g"], op["beta"])
    assert y.dtype == torch.float64 and y.shape == (M, N)
    assert torch.isfinite(y).all() and y.abs().max().item() < FP16_MAX, y.abs().max().item()
    y32 = lnres_ref32(op["A2"], op["W2"], op["b"], op["h2"], op["g"], op["beta"])
    assert torch.isfinite(y32).all()
    if family == "constant":
        assert torch.equal(y, op["beta"].double().expand(M, N))
    if family == "tile_means":
        # the between-tile term is most of the row's sum of squares
        x = (_unsplit2(op["A2"], torch.float64) @ _unsplit2(op["W2"], torch.float64).t() + op["b"].double()
             + _unsplit2(op["h2"], torch.float64))
        tm = x.view(M, N // 256, 256).mean(dim=2)
        between = 256 * ((tm - x.mean(dim=1, keepdim=True)) ** 2).sum(dim=1)
        total = ((x - x.mean(dim=1, keepdim=True)) ** 2).sum(dim=1)
        assert (between / total).min().item() > 0.9
    if family == "offset":
        x = (_unsplit2(op["A2"], torch.float64) @ _unsplit2(op["W2"], torch.float64).t() + op["b"].double()
             + _unsplit2(op["h2"], torch.float64))
        assert (x.mean(dim=1).abs() / x.std(dim=1)).min().item() > 100
