"""Helpers shared by the split-operand GEMM tests (a plain module, imported by name).

* the interleaved two-part operand image (common.h, kx == 2) and its decoding;
* a float64 LayerNorm and the float64 / float32 evaluations of the fused residual + LayerNorm
  GEMM  y = LN(unsplit(A2) . unsplit(W2)^T + b + unsplit(h2); gamma, beta, eps)  on the values the
  images HOLD (operand quantisation is not part of the error);
* the input families of tests/test_gpu_lnres.py (checked on the CPU in tests/test_x3s_image.py).
"""
import torch

LN_EPS = 1e-12
FP16_MAX = 6.0e4          # the magnitude every image part must stay below


def _split2(x):
    """The split-operand GEMM's two-part image of fp32 x [R, K] (common.h kx == 2): hi and
    lo = (x - hi) * 64 interleaved per 32-column K-step, [hi 0..31 | lo 0..31 | hi 32..63 | ...]."""
    hi = x.half()
    lo = ((x - hi.float()) * 64.0).half()
    R, K = x.shape
    return torch.stack([hi.view(R, K // 32, 32), lo.view(R, K // 32, 32)], dim=2).reshape(R, 2 * K).contiguous()


def _unsplit2(img, dtype=torch.float32):
    """hi + lo / 64 of an interleaved two-part image [R, 2N] -> [R, N] (fp32; float64 is exact)."""
    R, N2 = img.shape
    v = img.to(dtype).view(R, N2 // 64, 2, 32)
    return (v[:, :, 0] + v[:, :, 1] / 64.0).reshape(R, N2 // 2)


def ln_ref64(x64, g, b, eps):
    """LayerNorm over the last dimension in float64 (biased variance, as torch / BERT)."""
    x64 = x64.double()
    mean = x64.mean(dim=-1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(dim=-1, keepdim=True)
    return d / torch.sqrt(var + eps) * g.double() + b.double()


def gemm_ref(A2, W2, b, dtype):
    """unsplit(A2) . unsplit(W2)^T + b evaluated in ``dtype`` on the values the images hold."""
    return _unsplit2(A2, torch.float64).to(dtype) @ _unsplit2(W2, torch.float64).to(dtype).t() + b.to(dtype)


def lnres_ref64(A2, W2, b, h2, g, beta, eps=LN_EPS):
    x = gemm_ref(A2, W2, b, torch.float64) + _unsplit2(h2, torch.float64)
    return ln_ref64(x, g, beta, eps)


def lnres_ref32(A2, W2, b, h2, g, beta, eps=LN_EPS):
    """The yardstick: the same expression in torch fp32 (float() of the unsplit images, fp32 matmul,
    F.layer_norm in fp32)."""
    x = gemm_ref(A2, W2, b, torch.float32) + _unsplit2(h2, torch.float64).float()
    return torch.nn.functional.layer_norm(x, (x.shape[1],), g.float(), beta.float(), eps)


FAMILIES = ("plain", "offset", "tile_means", "constant", "distinct_affine")


def lnres_operands(family, M, N, K, seed=0, device="cpu"):
    """Operands of one fused residual + LayerNorm GEMM: images A2 [M, 2K], W2 [N, 2K], h2 [M, 2N]
    and fp32 b, gamma, beta [N].

    plain            A ~ randn, W ~ 0.05 randn, h ~ randn
    offset           h = 30 + 0.01 randn, A = 0.01 randn: row mean >> row std
    tile_means       b = +20, 0, -20, ... per 256-column tile, h ~ 0.1 randn: the between-tile term
                     256 (mean_c - mean)^2 dominates the row's sum of squares
    constant         A = 0, h = 0, b = 0.5: every partial sum exact, variance exactly 0
    distinct_affine  plain with gamma[c] = 1 + c/N, beta[c] = c/N - 0.5 (a column permutation
                     applied to the wrong vector shows)
    """
    assert family in FAMILIES, family
    gen = torch.Generator(device=device).manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, device=device, generator=gen)

    A, W, h = rn(M, K), 0.05 * rn(N, K), rn(M, N)
    b, g, beta = 0.1 * rn(N), 1.0 + 0.1 * rn(N), 0.1 * rn(N)
    if family == "offset":
        h = 30.0 + 0.01 * h
        A = 0.01 * A
    elif family == "tile_means":
        h = 0.1 * h
        tile = torch.arange(N, device=device) // 256
        b = (20.0 * (1 - tile % 3)).float()               # +20, 0, -20, +20, ...
    elif family == "constant":
        A, h = torch.zeros_like(A), torch.zeros_like(h)
        b = torch.full_like(b, 0.5)
    elif family == "distinct_affine":
        c = torch.arange(N, device=device, dtype=torch.float32)
        g, beta = 1.0 + c / N, c / N - 0.5
    return {"A2": _split2(A), "W2": _split2(W), "h2": _split2(h), "b": b.contiguous(), "g": g.contiguous(),
            "beta": beta.contiguous()}
