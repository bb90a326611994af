"""GPU: the ragged self-attention kernels vs a torch fp32 reference (eager_attention_forward,
transformers modeling_bert.py:111-136, scale 64**-0.5, no padding rows), per sequence.

Kernels (k_attn.hip, through the rs_debug_attention diagnostic entry): kind 0 = attn_tr_kernel
(32x32x16 MFMA, production's fp16 kernel for a chunk with some T > 64), kind 6 = attn16_kernel
(16x16x32 MFMA, production's fp16 kernel while every T <= 64).  Lengths cover
the tile edges of both (1, 15/16/17, 31/32/33, 47/48, 63/64/65) and the online-softmax path
(T > 64, several key blocks).  Inputs and P are fp16, accumulation fp32: |err| <= 2e-3 on
O(1) outputs.

Also: the fp32 online-softmax kernel over every length (production uses it for T > 64 only); the
production router launch_attention_full with the two-part image output (rs_debug_attention_full,
kx = 2: both attn16x3v2_kernel instances through their permlane-swap stores, and the mixed chunk
where two kernels share one ctx); and a peaked-softmax family (logit std ~ 9, one planted key per
sequence, in the last key block for T > 64) next to the nearly flat 0.6 randn inputs, judged against
float64 by e32, the error of the same expression in torch fp32.  Measured err / e32 on MI355X:
flat inputs (asserted: the existing 2e-6; err 2.3e-7 .. 3.1e-7): kind 9 all lengths 1.52; router
H 768 max_len 48 / 64 / 200: 1.45 / 1.65 / 1.58; H 256: 2.08 / 2.27 / 1.89.  Peaked (asserted:
err <= 4 e32): kind 9 0.45, kind 10 0.53, kind 11 0.28, router (max_len 200) 0.55.  Peaked, fp16
kernels 0 and 6 (asserted: 2^-10 max(1, max|v|) per sequence and head): 0.45 of the bound each.
"""
import ctypes

import numpy as np
import pytest
import torch

from asr_rescoring_amd import _lib
from x3s_image import _unsplit2

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 96, 100, 128, 130, 200]


def _run(kind, qkv, T, row, H, heads, kx=1):
    lib = _lib.load()
    fn = lib.rs_debug_attention
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    dev = qkv.device
    d_len = torch.from_numpy(T).to(dev)
    d_row = torch.from_numpy(row).to(dev)
    ctx = torch.full((qkv.shape[0], kx * H), float("nan"), device=dev, dtype=torch.float16)
    assert fn(kind, qkv.data_ptr(), d_len.data_ptr(), d_row.data_ptr(), len(T), H, heads, ctx.data_ptr(),
              torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return ctx


@pytest.mark.parametrize("kind", [0, 6])
def test_attention_kernels_vs_torch(kind):
    H, heads = 768, 12
    rng = np.random.default_rng(3)
    T = np.array(LENGTHS * 2, np.int32)
    rng.shuffle(T)
    row = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int32)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(11)
    qkv = (torch.randn(int(T.sum()), 3 * H, device=dev, generator=g) * 0.6).half()
    ctx = _run(kind, qkv, T, row, H, heads)
    worst = 0.0
    for r0, t in zip(row.tolist(), T.tolist()):
        x = qkv[r0:r0 + t].float().view(t, 3, heads, 64)
        q, k, v = x[:, 0].transpose(0, 1), x[:, 1].transpose(0, 1), x[:, 2].transpose(0, 1)
        p = torch.softmax(q @ k.transpose(1, 2) * 0.125, dim=-1)
        ref = (p @ v).transpose(0, 1).reshape(t, H)
        got = ctx[r0:r0 + t].float()
        assert torch.isfinite(got).all(), t
        worst = max(worst, (got - ref).abs().max().item())
    assert worst < 2e-3, worst


def test_attention_kernels_agree():
    """16x16x32 and 32x32x16 kernels on the same C3-like lengths (T 26..44): same result to
    fp16 rounding of P (different key-tile partition of the fp32 sums)."""
    H, heads = 768, 12
    rng = np.random.default_rng(5)
    T = rng.integers(26, 45, size=256).astype(np.int32)
    row = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int32)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(12)
    qkv = (torch.randn(int(T.sum()), 3 * H, device=dev, generator=g) * 0.6).half()
    a = _run(0, qkv, T, row, H, heads).float()
    b = _run(6, qkv, T, row, H, heads).float()
    assert (a - b).abs().max().item() < 2e-3


@pytest.mark.parametrize("kind,tmax", [(9, 64), (10, 48), (11, 64)])
def test_split_precision_attention_vs_torch(kind, tmax):
    """fp16x3 mode: fp32 Q/K/V, ctx written as the [hi | hi/64 | lo*64] operand image.  10 / 11 =
    attn16x3v2_kernel (three fp16 MFMAs per product) with 48 / 64
    staged key rows (swizzled unpadded V image, Vt fragments read per query tile), 9 = fp32
    VALU kernel; all at fp32-level accuracy: |hi + lo - ref| <= 2e-6 on O(1) outputs.
    T <= tmax (the kernel's range)."""
    H, heads = 768, 12
    rng = np.random.default_rng(4)
    T = np.array([t for t in LENGTHS if t <= tmax] * 2, np.int32)
    rng.shuffle(T)
    row = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int32)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(13)
    qkv = torch.randn(int(T.sum()), 3 * H, device=dev, generator=g) * 0.6
    ctx = _run(kind, qkv, T, row, H, heads, kx=3).float()
    got_all = ctx[:, :H] + ctx[:, 2 * H:] / 64
    assert torch.equal((ctx[:, :H] / 64).half().float(), ctx[:, H:2 * H])     # mid = fp16(hi / 64)
    worst = 0.0
    for r0, t in zip(row.tolist(), T.tolist()):
        x = qkv[r0:r0 + t].double().view(t, 3, heads, 64)
        q, k, v = x[:, 0].transpose(0, 1), x[:, 1].transpose(0, 1), x[:, 2].transpose(0, 1)
        p = torch.softmax(q @ k.transpose(1, 2) * 0.125, dim=-1)
        ref = (p @ v).transpose(0, 1).reshape(t, H)
        worst = max(worst, (got_all[r0:r0 + t].double() - ref).abs().max().item())
    assert worst < 2e-6, worst


# ---- the production router, every length on the fp32 kernel, and peaked softmaxes ----------------

def _layout(lengths, seed, reps=2):
    rng = np.random.default_rng(seed)
    T = np.array(list(lengths) * reps, np.int32)
    rng.shuffle(T)
    row = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int32)
    return T, row


def _ref(qkv, T, row, H, heads, dtype):
    """softmax(Q K^T / 8) V per (sequence, head) evaluated in ``dtype`` -> [rows, H]."""
    out = torch.empty(qkv.shape[0], H, device=qkv.device, dtype=dtype)
    for r0, t in zip(row.tolist(), T.tolist()):
        x = qkv[r0:r0 + t].to(dtype).view(t, 3, heads, 64)
        q, k, v = x[:, 0].transpose(0, 1), x[:, 1].transpose(0, 1), x[:, 2].transpose(0, 1)
        p = torch.softmax(q @ k.transpose(1, 2) * 0.125, dim=-1)
        out[r0:r0 + t] = (p @ v).transpose(0, 1).reshape(t, H)
    return out


def _run_full(qkv, T, row, max_len, H, heads, kx=2):
    """launch_attention_full as a split-operand layer calls it (rs_debug_attention_full); ctx
    pre-filled with NaN: every row must be written."""
    dev = qkv.device
    d_len, d_row = torch.from_numpy(T).to(dev), torch.from_numpy(row).to(dev)
    ctx = torch.full((qkv.shape[0], kx * H), float("nan"), device=dev, dtype=torch.float16)
    assert int(T.max()) <= max_len and int(T.sum()) == qkv.shape[0]
    assert _lib.load().rs_debug_attention_full(qkv.data_ptr(), d_len.data_ptr(), d_row.data_ptr(), len(T), max_len,
                                               H, heads, kx, ctx.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return ctx


def _decode3(ctx, H):
    c = ctx.double()
    return c[:, :H] + c[:, 2 * H:] / 64


def _flat(T, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(int(T.sum()), 3 * H, device="cuda", generator=g) * 0.6


def _peaked(T, row, H, heads, seed):
    """Q, K ~ 3 randn (logit std ~ 9), V ~ 0.6 randn, and one planted key per sequence: every query
    and that key share the component 2.5 u (u = +-1 per head dimension), which adds 2.5^2 64 / 8 = 50
    to its logit.  For T > 64 the planted key lies in the LAST 64-key block, so the online softmax's
    running maximum changes late and everything accumulated before is rescaled by ~e^-20."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    n = int(T.sum())
    qkv = torch.randn(n, 3, H, device="cuda", generator=g) * torch.tensor([3.0, 3.0, 0.6], device="cuda").view(1, 3, 1)
    u = 2.5 * (torch.randint(0, 2, (len(T), H), device="cuda", generator=g).float() * 2 - 1)
    for i, (r0, t) in enumerate(zip(row.tolist(), T.tolist())):
        lo = 64 * ((t - 1) // 64)
        j = int(rng.integers(lo, t))
        qkv[r0:r0 + t, 0] += u[i]
        qkv[r0 + j, 1] += u[i]
    return qkv.view(n, 3 * H).contiguous()


def _yardstick(name, got64, qkv, T, row, H, heads, flat_tol=None):
    """err against float64; e32 = the torch fp32 evaluation's error against float64."""
    ref = _ref(qkv, T, row, H, heads, torch.float64)
    e32 = (_ref(qkv, T, row, H, heads, torch.float32).double() - ref).abs().max().item()
    assert torch.isfinite(got64).all(), name
    err = (got64 - ref).abs().max().item()
    print(f"ATTN {name}: err {err:.3e} e32 {e32:.3e} err/e32 {err / e32:.2f}")
    if flat_tol is not None:
        assert err < flat_tol, (name, err)
    else:
        assert err <= 4 * e32, (name, err, e32)


def test_fp32_attention_every_length():
    """attn_full_kernel<float> (kind 9) over all of LENGTHS: up to four 64-key blocks with a ragged
    last one — the range production uses it for (T > 64) — at the 2e-6 of the T <= 64 test."""
    H, heads = 768, 12
    T, row = _layout(LENGTHS, 6)
    qkv = _flat(T, H, 14)
    ctx = _run(9, qkv, T, row, H, heads, kx=3)
    _yardstick("kind9-flat", _decode3(ctx, H), qkv, T, row, H, heads, flat_tol=2e-6)


@pytest.mark.parametrize("max_len", [48, 64, 200])
@pytest.mark.parametrize("H,heads", [(768, 12), (256, 4)])
def test_attention_router_two_part_image(H, heads, max_len):
    """launch_attention_full with kx = 2, as every split-operand layer launches it: the interleaved
    image through the permlane-swap 16-byte stores of attn16x3v2_kernel (R = 48 for max_len <= 48,
    R = 64 for <= 64) and, for max_len = 200, the mixed chunk — attn16x3v2_kernel<64> and
    attn_full_kernel<float> in one launch pair, each skipping the other's sequences, every ctx row
    written exactly once (NaN pre-fill, all finite after)."""
    T, row = _layout([t for t in LENGTHS if t <= max_len], 7 + max_len)
    qkv = _flat(T, H, 15)
    ctx = _run_full(qkv, T, row, max_len, H, heads)
    assert torch.isfinite(ctx.float()).all()
    _yardstick(f"router-H{H}-L{max_len}-flat", _unsplit2(ctx, torch.float64), qkv, T, row, H, heads, flat_tol=2e-6)


@pytest.mark.parametrize("kind,tmax", [(9, 200), (10, 48), (11, 64), ("router", 200)])
def test_peaked_softmax_split_precision(kind, tmax):
    """Peaked softmaxes (_peaked) on the fp32 and fp16x3 kernels: err <= 4 e32."""
    H, heads = 768, 12
    T, row = _layout([t for t in LENGTHS if t <= tmax], 8)
    qkv = _peaked(T, row, H, heads, 16)
    if kind == "router":
        got = _unsplit2(_run_full(qkv, T, row, tmax, H, heads), torch.float64)
    else:
        got = _decode3(_run(kind, qkv, T, row, H, heads, kx=3), H)
    _yardstick(f"peaked-{kind}", got, qkv, T, row, H, heads)


@pytest.mark.parametrize("kind", [0, 6])
def test_peaked_softmax_fp16_kernels(kind):
    """Peaked softmaxes on the fp16 kernels.  The inputs are exactly fp16 (no operand error); the
    output is a convex combination of the v_j formed with fp16 P (relative rounding 2^-11 per weight:
    at most 2^-11 max|v|) and rounded to fp16 (half an ulp: at most 2^-11 max(1, max|v|)), so per
    (sequence, head)  |err| <= 2^-10 max(1, max_j |v_j|)."""
    H, heads = 768, 12
    T, row = _layout(LENGTHS, 9)
    qkv = _peaked(T, row, H, heads, 17).half()
    ctx = _run(kind, qkv, T, row, H, heads).double()
    assert torch.isfinite(ctx).all()
    ref = _ref(qkv, T, row, H, heads, torch.float64)
    worst = 0.0
    for r0, t in zip(row.tolist(), T.tolist()):
        err = (ctx[r0:r0 + t] - ref[r0:r0 + t]).abs().view(t, heads, 64).amax(dim=(0, 2))
        vmax = qkv[r0:r0 + t, 2 * H:].double().abs().view(t, heads, 64).amax(dim=(0, 2))
        ratio = (err / (2.0 ** -10 * vmax.clamp_min(1.0))).max().item()
        worst = max(worst, ratio)
    print(f"ATTN peaked-fp16-kind{kind}: worst err / bound {worst:.3f}")
    assert worst <= 1.0, (kind, worst)
