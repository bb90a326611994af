// BERT self-attention kernels (gfx950, wave64, head_dim 64).
//
//  attention_full  eager_attention_forward (modeling_bert.py:111-136) over ragged sequences
//                  (no padding rows: equal to the reference's additive pad mask)
//  attention_query the same, last layer, only the scored row of each sequence (masked
//                  position for MLM_PLL, [CLS] for RescoreBert) — the other rows' last-layer
//                  states never reach a score
//
// Every kernel runs one wave per (sequence, head) and writes the fp16 operand image of the
// context (put_split, common.h).  Which kernel serves which launch of attention_full
// (max_len = the longest sequence of the launch, DEDUP = layer-0 unique rows):
//
//  Q/K/V  max_len  kernel
//  fp32   <= 48    attn16x3v2_kernel<DEDUP, 48>   split fp16 hi + lo MFMA, 48 staged key rows
//  fp32   <= 64    attn16x3v2_kernel<DEDUP, 64>   the same, 64 staged key rows
//  fp32   >  64    attn16x3v2_kernel<false, 64> for the launch's T <= 64 sequences, then
//                  attn_full_kernel<float> (fp32 VALU, online softmax) for the longer ones
//  fp16   <= 64    attn16_kernel<DEDUP>           16x16x32 MFMA tiles
//  fp16   >  64    attn_tr_kernel<DEDUP>          32x32x16 MFMA tiles, online softmax
//
// attention_query is attn_query_kernel<float | f16>; attention_mquery (multi-mask rows: several
// scored rows per sequence) is attn_mquery_kernel<float | f16>, four waves per (sequence, head), each
// serving one query at a time in attn_query_kernel's form.  attn_memskel_kernel is a timing
// diagnostic (rs_debug_attention), not part of the scoring path.
//
// rs_debug_attention kinds (AttnKind): 0 attn_tr_kernel, 6 attn16_kernel (fp16 qkv [rows, 3H],
// ctx fp16 [rows, H]); 9 attn_full_kernel<float>, 10 / 11 attn16x3v2_kernel with 48 / 64 staged
// key rows (fp32 qkv [rows, 3H], ctx the three-part fp16 image [rows, 3H]); 3 / 4 the memory
// skeleton of attn_tr_kernel (one / four heads per block).
#include <type_traits>
#include "common.h"

namespace {

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

// ds_read_b64_tr_b16 (gfx950 hardware transpose) of the LDS address p
__device__ __forceinline__ half4 tr_read(const f16* p) {
    const fp16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)p);
    return __builtin_bit_cast(half4, v);
}

// Q/K/V row of position t of sequence s, head hd: rowp(t) points at the head's 64 Q columns
// of a [rows, ld = 3H] buffer (K at + H, V at + 2H).  rs: the sequence's first row.
// DEDUP (layer 0): qkv holds the chunk's unique rows; position t reads row urow_m[s] + (t - lo)
// when it lies in the sequence's masked span [lo, hi) (the [MASK] rows of a hypothesis live apart
// from its unmasked rows), urow_h[s] + t otherwise.  Both are `row origin + t`: the span only
// chooses the origin (urow_m - lo or urow_h).
template <class QT, bool DEDUP>
struct SeqRows {
    const QT* base;
    const QT* mbase;           // origin of the span's rows: row urow_m - lo (only positions >= lo read it)
    int ld, lo, n;
    __device__ __forceinline__ SeqRows(const QT* qkv, const SeqMeta& sm, int s, int rs, int ld_, int hd) : ld(ld_) {
        const int ub = DEDUP ? sm.urow_h[s] : rs;
        lo = DEDUP ? sm.mask_pos[s] : 0;
        n = DEDUP ? sm.mask_end[s] - lo : 0;
        const int um = DEDUP ? sm.urow_m[s] - lo : 0;
        base = qkv + (size_t)ub * ld + hd * 64;
        mbase = qkv + (ptrdiff_t)um * ld + hd * 64;
    }
    __device__ __forceinline__ const QT* operator()(int t) const {
        if constexpr (DEDUP) return ((unsigned)(t - lo) < (unsigned)n ? mbase : base) + (size_t)t * ld;
        else return base + (size_t)t * ld;
    }
};

__device__ __forceinline__ void load8(const f16* p, float (&o)[8]) {
    const half8 v = *(const half8*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)v[e];
}
__device__ __forceinline__ void load8(const float* p, float (&o)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// One wave per (sequence, head), one query row per lane, keys in blocks of 64 staged
// in LDS as fp32; online softmax across key blocks (T > 64).
template <class QT>
__global__ void __launch_bounds__(64)
attn_full_kernel(const QT* __restrict__ qkv, SeqMeta sm, int s0, int row0, int H,
                 f16* __restrict__ ctx, int kx, int skip_le) {
    __shared__ __attribute__((aligned(16))) float sK[64][64];
    __shared__ __attribute__((aligned(16))) float sV[64][64];
    const int s = s0 + blockIdx.x, h = blockIdx.y;
    const int T = sm.len[s], rs = sm.row[s] - row0;
    if (T <= skip_le) return;                     // (mixed chunks: the short ones run on MFMA)
    const int lane = threadIdx.x;
    const int ld = 3 * H;
    const QT* base = qkv + (size_t)rs * ld + h * 64;
    const float scale = 0.125f;   // head_dim ** -0.5 with head_dim = 64

    for (int q0 = 0; q0 < T; q0 += 64) {
        const int t = q0 + lane;
        const bool qv = t < T;
        float q[64];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (qv) load8(base + (size_t)t * ld + c * 8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) q[c * 8 + e] = v[e];
        }
        float acc[64];
#pragma unroll
        for (int d = 0; d < 64; ++d) acc[d] = 0.f;
        float m = -INFINITY, l = 0.f;

        for (int k0 = 0; k0 < T; k0 += 64) {
            const int nk = min(64, T - k0);
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int kr = it * 8 + (lane >> 3), ch = lane & 7;
                float kv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                float vv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (kr < nk) {
                    load8(base + (size_t)(k0 + kr) * ld + H + ch * 8, kv);
                    load8(base + (size_t)(k0 + kr) * ld + 2 * H + ch * 8, vv);
                }
                *(float4*)&sK[kr][ch * 8] = make_float4(kv[0], kv[1], kv[2], kv[3]);
                *(float4*)&sK[kr][ch * 8 + 4] = make_float4(kv[4], kv[5], kv[6], kv[7]);
                *(float4*)&sV[kr][ch * 8] = make_float4(vv[0], vv[1], vv[2], vv[3]);
                *(float4*)&sV[kr][ch * 8 + 4] = make_float4(vv[4], vv[5], vv[6], vv[7]);
            }
            __syncthreads();
            float sc[64];
            float bm = -INFINITY;
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                float d0 = 0.f, d1 = 0.f;
                if (j < nk) {
#pragma unroll
                    for (int c = 0; c < 16; c += 2) {
                        const float4 ka = *(const float4*)&sK[j][c * 4];
                        const float4 kb = *(const float4*)&sK[j][c * 4 + 4];
                        d0 += q[c * 4] * ka.x + q[c * 4 + 1] * ka.y + q[c * 4 + 2] * ka.z + q[c * 4 + 3] * ka.w;
                        d1 += q[c * 4 + 4] * kb.x + q[c * 4 + 5] * kb.y + q[c * 4 + 6] * kb.z + q[c * 4 + 7] * kb.w;
                    }
                    sc[j] = (d0 + d1) * scale;
                    bm = fmaxf(bm, sc[j]);
                } else {
                    sc[j] = -INFINITY;
                }
            }
            const float mn = fmaxf(m, bm);
            const float alpha = __expf(m - mn);   // m = -inf on the first block -> 0
            l *= alpha;
#pragma unroll
            for (int d = 0; d < 64; ++d) acc[d] *= alpha;
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                if (j < nk) {
                    const float p = __expf(sc[j] - mn);
                    l += p;
#pragma unroll
                    for (int c = 0; c < 16; ++c) {
                        const float4 vv = *(const float4*)&sV[j][c * 4];
                        acc[c * 4] += p * vv.x;
                        acc[c * 4 + 1] += p * vv.y;
                        acc[c * 4 + 2] += p * vv.z;
                        acc[c * 4 + 3] += p * vv.w;
                    }
                }
            }
            m = mn;
        }
        if (qv) {
            const float il = 1.0f / l;
            f16* o = ctx + (size_t)(rs + t) * kx * H;
#pragma unroll
            for (int c = 0; c < 16; ++c)
                put_split4(o, h * 64 + c * 4, H, kx,
                           make_float4(acc[c * 4] * il, acc[c * 4 + 1] * il, acc[c * 4 + 2] * il, acc[c * 4 + 3] * il));
        }
    }
}

// One wave per (sequence, head), MFMA, latency-lean variant:
//  * K fragments (A operand of X = K.Q^T) go straight from HBM into registers and stay
//    resident across the query tiles (T <= 64: one key block, loaded once);
//  * V is staged ROW-major in LDS with ds_write_b128 and its transposed fragments (A operand
//    of O^T = V^T.P^T) are read with ds_read_b64_tr_b16 (gfx950 hardware transpose): no
//    scalar transposing writes.  V row stride 96 halfs makes those reads conflict-free
//    (the 8 (row, 16-column) blocks of a 32-lane half land on disjoint 8-bank ranges);
//  * all of a key block's global loads are in flight before the first is consumed.
// Numerics: fp16 P, fp32 accumulation, online softmax across 64-key blocks.
// DEDUP (layer 0): Q, K, V rows come from the chunk's unique rows (SeqRows).
template <bool DEDUP>
__global__ void __launch_bounds__(64, 3)
attn_tr_kernel(const f16* __restrict__ qkv, SeqMeta sm, int s0, int row0, int H,
               f16* __restrict__ ctx, int kx) {
    constexpr int VR = 96;
    __shared__ __attribute__((aligned(16))) f16 sV[64 * VR];
    // grid (sequence, head) (a head-major 1-D grid, the heads of a sequence adjacent, measured
    // 7 % slower, round 1)
    const int s = s0 + (int)blockIdx.x;
    const int hd = (int)blockIdx.y;
    const int T = sm.len[s], rs = sm.row[s] - row0;
    const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
    const SeqRows<f16, DEDUP> rowp(qkv, sm, s, rs, 3 * H, hd);
    const float scale = 0.125f;                   // head_dim ** -0.5
    const int nkb = (T + 63) >> 6;
    // transposed-read role: 16-lane group g reads keys 4(g>>1) + q (+8), dims 16(g&1) + 4p
    const int g4 = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int tr_off = (4 * (g4 >> 1) + tq) * VR + 16 * (g4 & 1) + 4 * tp;

    half8 kf[2][4];
    auto load_kv = [&](int k0) {
        half8 v[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int kr = it * 8 + (lane >> 3), d0 = (lane & 7) * 8;
            v[it] = k0 + kr < T ? *(const half8*)(rowp(k0 + kr) + 2 * H + d0) : (half8){};
        }
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int key = k0 + kt * 32 + r;
                kf[kt][ks] = key < T ? *(const half8*)(rowp(key) + H + ks * 16 + hf * 8) : (half8){};
            }
        __syncthreads();                          // previous block's V reads are done
#pragma unroll
        for (int it = 0; it < 8; ++it)
            *(half8*)(sV + (it * 8 + (lane >> 3)) * VR + (lane & 7) * 8) = v[it];
        __syncthreads();
    };

    half8 qn[4];                                  // Q fragments of the next query tile (prefetch)
    auto load_q = [&](int q0) {
        const int t = q0 + r;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            qn[ks] = t < T ? *(const half8*)(rowp(t) + ks * 16 + hf * 8) : (half8){};
    };
    load_q(0);
    for (int q0 = 0; q0 < T; q0 += 32) {
        const int t = q0 + r;
        half8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = qn[ks];
        if (q0 + 32 < T) load_q(q0 + 32);
        f32x16 o[2] = {(f32x16){}, (f32x16){}};  // O^T[d tile], lane = query
        float m = -INFINITY, l = 0.f;
        for (int kb = 0; kb < nkb; ++kb) {
            const int k0 = kb * 64;
            if (nkb > 1 || q0 == 0) load_kv(k0);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (k0 + kt * 32 >= T) break;
                f32x16 x = {};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) x = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kt][ks], qf[ks], x, 0, 0, 0);
                float bm = -INFINITY;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int kj = k0 + kt * 32 + (j & 3) + 8 * (j >> 2) + 4 * hf;
                    const float v = kj < T ? x[j] * scale : -INFINITY;
                    x[j] = v;
                    bm = fmaxf(bm, v);
                }
                bm = fmaxf(bm, __shfl_xor(bm, 32));
                const float mn = fmaxf(m, bm);
                const float alpha = __expf(m - mn);
                half8 pf[2];
                float ls = 0.f;
#pragma unroll
                for (int sk = 0; sk < 2; ++sk)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const f16 ph = (f16)__expf(x[sk * 8 + e] - mn);
                        pf[sk][e] = ph;
                        ls += (float)ph;
                    }
                ls += __shfl_xor(ls, 32);
                l = l * alpha + ls;
                m = mn;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) o[dt][j] *= alpha;
#pragma unroll
                    for (int sk = 0; sk < 2; ++sk) {
                        // keys kt*32 + 16 sk + 4 hf + {0..3, 8..11}: the P fragment's key order
                        const f16* p = sV + (kt * 32 + 16 * sk) * VR + 32 * dt + tr_off;
                        const half4 lo = tr_read(p), hi = tr_read(p + 8 * VR);
                        const half8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[sk], o[dt], 0, 0, 0);
                    }
                }
            }
        }
        if (t < T) {
            const float il = 1.0f / l;
            f16* orow = ctx + (size_t)(rs + t) * kx * H;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    put_split4(orow, hd * 64 + dt * 32 + 8 * g + 4 * hf, H, kx,
                               make_float4(o[dt][4 * g] * il, o[dt][4 * g + 1] * il,
                                           o[dt][4 * g + 2] * il, o[dt][4 * g + 3] * il));
        }
    }
}

// One wave per (sequence, head) on v_mfma_f32_16x16x32_f16: query tiles of 16 and key tiles
// of 16 (a T = 35 sequence computes 48 x 48 scores instead of 64 x 64 with 32-wide tiles, and
// 12 instead of 16 softmax values per lane and query tile).
//  * Xt = K.Qt per (16-key tile, 16-query tile): lane l holds query l&15, keys 4(l>>4)+e.
//  * softmax over keys: in-lane over the key tiles, then across the 4 lanes of a query
//    (xor 16, 32).
//  * Ot = Vt.Pt per (16-dim tile, 32-key step m): the P fragment is the two key tiles 2m, 2m+1
//    straight from the score registers, so its k index 8(l>>4)+j is key 32m + 4(l>>4) + j
//    (j < 4) or 32m + 16 + 4(l>>4) + j - 4; the Vt fragment follows the same key order with two
//    ds_read_b64_tr_b16 (rows 32m + 4g .. +3 and 32m + 16 + 4g .. +3 of the row-major V image,
//    16 columns).  V row stride 80 halfs: the 8 rows x 16 columns a 32-lane half reads land on
//    disjoint 8-bank ranges.  Vt fragments are read once per key block into registers.
// Online softmax over key blocks of 64 for T > 64.  DEDUP as attn_tr_kernel.
template <bool DEDUP>
__global__ void __launch_bounds__(64, 3)
attn16_kernel(const f16* __restrict__ qkv, SeqMeta sm, int s0, int row0, int H,
              f16* __restrict__ ctx, int kx) {
    constexpr int VR = 80;
    __shared__ __attribute__((aligned(16))) f16 sV[64 * VR];
    const int s = s0 + blockIdx.x, hd = blockIdx.y;
    const int T = sm.len[s], rs = sm.row[s] - row0;
    const int lane = threadIdx.x, r16 = lane & 15, g = lane >> 4;
    const SeqRows<f16, DEDUP> rowp(qkv, sm, s, rs, 3 * H, hd);
    const float scale = 0.125f;                   // head_dim ** -0.5
    const int nkb = (T + 63) >> 6;
    // transposed-read role: lane 4q+p of group g supplies row 4g + q, columns 4p
    const int tr_off = (4 * g + ((lane & 15) >> 2)) * VR + 4 * (lane & 3);
    half8 kf[4][2];                               // [key tile][32-dim step]
    half8 vf[4][2];                               // Vt fragments [16-dim tile][32-key step]
    auto load_kv = [&](int k0) {
        half8 v[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int kr = k0 + it * 8 + (lane >> 3);
            v[it] = kr < T ? *(const half8*)(rowp(kr) + 2 * H + (lane & 7) * 8) : (half8){};
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int key = k0 + kt * 16 + r16;
                kf[kt][ks] = key < T ? *(const half8*)(rowp(key) + H + ks * 32 + g * 8) : (half8){};
            }
        __syncthreads();                          // previous block's V reads are done
#pragma unroll
        for (int it = 0; it < 8; ++it)
            *(half8*)(sV + (it * 8 + (lane >> 3)) * VR + (lane & 7) * 8) = v[it];
        __syncthreads();
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2) {
                const f16* p = sV + (32 * m2) * VR + 16 * dt + tr_off;
                const half4 lo = tr_read(p), hi = tr_read(p + 16 * VR);
                vf[dt][m2] = (half8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
    };
    for (int q0 = 0; q0 < T; q0 += 16) {
        const int t = q0 + r16;
        half8 qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[ks] = t < T ? *(const half8*)(rowp(t) + ks * 32 + g * 8) : (half8){};
        f32x4 o[4] = {(f32x4){}, (f32x4){}, (f32x4){}, (f32x4){}};   // Ot[16-dim tile], lane = query
        float m = -INFINITY, l = 0.f;
        for (int kb = 0; kb < nkb; ++kb) {
            const int k0 = kb * 64;
            if (nkb > 1 || q0 == 0) load_kv(k0);
            const int nkt = min(4, (T - k0 + 15) >> 4);
            f32x4 x[4];
            float bm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                x[kt] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (kt < nkt) {
                    f32x4 a = {};
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][ks], qf[ks], a, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = k0 + kt * 16 + 4 * g + e;
                        const float v = key < T ? a[e] * scale : -INFINITY;
                        x[kt][e] = v;
                        bm = fmaxf(bm, v);
                    }
                }
            }
            bm = fmaxf(bm, __shfl_xor(bm, 16));
            bm = fmaxf(bm, __shfl_xor(bm, 32));
            const float mn = fmaxf(m, bm);
            const float alpha = __expf(m - mn);
            half8 pf[2];
            float ls = 0.f;
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const f16 ph = (f16)__expf(x[2 * m2 + (j >> 2)][j & 3] - mn);
                    pf[m2][j] = ph;
                    ls += (float)ph;
                }
            ls += __shfl_xor(ls, 16);
            ls += __shfl_xor(ls, 32);
            l = l * alpha + ls;
            m = mn;
            const int nm = (nkt + 1) >> 1;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                o[dt] *= alpha;
#pragma unroll
                for (int m2 = 0; m2 < 2; ++m2)
                    if (m2 < nm) o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[dt][m2], pf[m2], o[dt], 0, 0, 0);
            }
        }
        if (t < T) {
            const float il = 1.0f / l;
            f16* orow = ctx + (size_t)(rs + t) * kx * H;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                put_split4(orow, hd * 64 + dt * 16 + 4 * g, H, kx,
                           make_float4(o[dt][0] * il, o[dt][1] * il, o[dt][2] * il, o[dt][3] * il));
        }
    }
}

// fp16x3 precision mode (fp32 Q/K/V from the split-operand QKV GEMM): attn16_kernel's tiling
// with every MFMA operand split into fp16 hi + lo parts and three MFMAs per product
// (hi.hi + hi.lo + lo.hi, the lo.lo term is below fp32 rounding): Xt = K.Qt and Ot = Vt.Pt to
// fp32-level accuracy on the matrix cores instead of the fp32 VALU attention.  The f16 MFMA
// flushes subnormal inputs, and lo = x - hi is subnormal for |x| < 0.25, so lo parts are
// stored scaled by 2^12 (LO_SCALE) and their products go to separate accumulators scaled back
// by 2^-12: 1e-7-level error instead of 3e-5 (tools/diag/attn_split_check.py).  P is split
// after the exponential; the softmax row sum adds the fp32 P.  V is staged as two fp16 images
// (hi, scaled lo).  T <= 64 (one key block; the host routes longer
// sequences to attn_full_kernel<float>).
constexpr float LO_SCALE = 4096.f, LO_UNSCALE = 1.f / 4096.f;
// DEDUP (MLM layer 0): Q, K, V rows come from the chunk's unique rows (SeqRows), as
// attn16_kernel.
//
// Layout: V staged for R = 48 or 64 key rows only (R = 48 when
// every sequence of the chunk has T <= 48: the 16 rows past it are zeros the second 32-key
// block reads from registers), 128-B LDS rows without padding — the 16-B chunks XOR-swizzled
// by (row & 6), which keeps the ds_read_b64_tr_b16 lane groups on distinct banks — and the
// Vt fragments read from LDS per query tile instead of held in registers.  R = 48: 12 KiB of
// LDS and <= 168 VGPRs, so 3 waves per SIMD instead of 2.
template <bool DEDUP, int R>
__global__ void __launch_bounds__(64, R == 48 ? 3 : 2)
attn16x3v2_kernel(const float* __restrict__ qkv, SeqMeta sm, int s0, int row0, int H,
                  f16* __restrict__ ctx, int kx) {
    constexpr int KT = R / 16;                    // 16-key tiles staged
    __shared__ __attribute__((aligned(16))) f16 sVh[R * 64];
    __shared__ __attribute__((aligned(16))) f16 sVl[R * 64];
    const int s = s0 + blockIdx.x, hd = blockIdx.y;
    const int T = sm.len[s], rs = sm.row[s] - row0;
    if (T > R) return;                            // (mixed chunks: the long ones run on attn_full)
    const int lane = threadIdx.x, r16 = lane & 15, g = lane >> 4;
    const SeqRows<float, DEDUP> rowp(qkv, sm, s, rs, 3 * H, hd);
    // V image address (halfs) of (row, col): 16-B chunk col / 8 swizzled by (row & 6)
    auto vaddr = [](int row, int col) { return row * 64 + ((((col >> 3) ^ (row & 6))) << 3) + (col & 7); };
    const float scale = 0.125f;
    float4 vraw[R / 4], kraw[KT][2][2];
#pragma unroll
    for (int it = 0; it < R / 4; ++it) {
        const int kr = it * 4 + (lane >> 4), c4 = (lane & 15) * 4;
        vraw[it] = kr < T ? *(const float4*)(rowp(kr) + 2 * H + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int key = kt * 16 + r16;
            const float* kp = rowp(key) + H + ks * 32 + g * 8;
            kraw[kt][ks][0] = key < T ? *(const float4*)kp : make_float4(0.f, 0.f, 0.f, 0.f);
            kraw[kt][ks][1] = key < T ? *(const float4*)(kp + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    float4 qraw[2][2];
    auto load_q = [&](int q0) {
        const int t = q0 + r16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const float* qp = rowp(t) + ks * 32 + g * 8;
            qraw[ks][0] = t < T ? *(const float4*)qp : make_float4(0.f, 0.f, 0.f, 0.f);
            qraw[ks][1] = t < T ? *(const float4*)(qp + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    load_q(0);
    auto split_raw = [](const float4 (&r)[2], half8& hi, half8& lo) {
        const float v[8] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = (f16)v[e];
            lo[e] = (f16)((v[e] - (float)hi[e]) * LO_SCALE);
        }
    };
#pragma unroll
    for (int it = 0; it < R / 4; ++it) {
        const int kr = it * 4 + (lane >> 4), c4 = (lane & 15) * 4;
        const float4 v = vraw[it];
        const half4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
        const half4 l = {(f16)((v.x - (float)h[0]) * LO_SCALE), (f16)((v.y - (float)h[1]) * LO_SCALE),
                         (f16)((v.z - (float)h[2]) * LO_SCALE), (f16)((v.w - (float)h[3]) * LO_SCALE)};
        const int a = vaddr(kr, c4);
        *(half4*)(sVh + a) = h;
        *(half4*)(sVl + a) = l;
    }
    half8 kfh[KT][2], kfl[KT][2];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) split_raw(kraw[kt][ks], kfh[kt][ks], kfl[kt][ks]);
    __syncthreads();
    // transposed-read role: lane supplies row 4g + (l & 15) / 4 of a 16-row group, columns
    // 16 dt + 4 (l & 3); rows 16 and 32 further keep the same swizzle (row & 6)
    const int trow = 4 * g + ((lane & 15) >> 2);
    int tro[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) tro[dt] = vaddr(trow, 16 * dt + 4 * (lane & 3));
    const int nkt = min(KT, (T + 15) >> 4), nm = (nkt + 1) >> 1;
    for (int q0 = 0; q0 < T; q0 += 16) {
        const int t = q0 + r16;
        half8 qh[2], ql[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) split_raw(qraw[ks], qh[ks], ql[ks]);
        if (q0 + 16 < T) load_q(q0 + 16);
        f32x4 x[4];
        float bm = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            x[kt] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (kt < KT && kt < nkt) {
                f32x4 a = {}, al = {};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    al = __builtin_amdgcn_mfma_f32_16x16x32_f16(kfl[kt < KT ? kt : 0][ks], qh[ks], al, 0, 0, 0);
                    al = __builtin_amdgcn_mfma_f32_16x16x32_f16(kfh[kt < KT ? kt : 0][ks], ql[ks], al, 0, 0, 0);
                    a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kfh[kt < KT ? kt : 0][ks], qh[ks], a, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int key = kt * 16 + 4 * g + e;
                    const float v = key < T ? __builtin_fmaf(al[e], LO_UNSCALE, a[e]) * scale : -INFINITY;
                    x[kt][e] = v;
                    bm = fmaxf(bm, v);
                }
            }
        }
        bm = fmaxf(bm, __shfl_xor(bm, 16));
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        half8 ph[2], pl[2];
        float ls = 0.f;
#pragma unroll
        for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = __expf(x[2 * m2 + (j >> 2)][j & 3] - bm);
                ph[m2][j] = (f16)p;
                pl[m2][j] = (f16)((p - (float)ph[m2][j]) * LO_SCALE);
                ls += p;
            }
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            f32x4 oh = {}, ol = {};
#pragma unroll
            for (int m2 = 0; m2 < 2; ++m2)
                if (m2 < nm) {
                    const int ob = 32 * m2 * 64 + tro[dt];
                    half4 lo = tr_read(sVh + ob), hi = (half4){};
                    if (R == 64 || m2 == 0) hi = tr_read(sVh + ob + 16 * 64);
                    const half8 vh = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    lo = tr_read(sVl + ob);
                    hi = (half4){};
                    if (R == 64 || m2 == 0) hi = tr_read(sVl + ob + 16 * 64);
                    const half8 vl = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    ol = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph[m2], ol, 0, 0, 0);
                    ol = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl[m2], ol, 0, 0, 0);
                    oh = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph[m2], oh, 0, 0, 0);
                }
#pragma unroll
            for (int e = 0; e < 4; ++e) o[dt][e] = __builtin_fmaf(ol[e], LO_UNSCALE, oh[e]);
        }
        const float il = 1.0f / ls;
        f16* orow = ctx + (size_t)(rs + t) * kx * H;
        if (kx == 2) {
            // the interleaved image (common.h): lane (r16, g) holds columns 16 dt + 4 g .. + 3 of its
            // query row; one v_permlane16_swap per dword trades the odd lane group's hi parts for the
            // even group's lo parts (rows of 16 lanes: g <-> g ^ 1, the same query row), so every lane
            // stores 8 consecutive halves with one 16-B store — even g: hi of columns 16 dt + 4 g ..
            // + 7, odd g: lo of 16 dt + 4 (g - 1) .. + 7 — instead of two 8-B stores (T21)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const float4 v = make_float4(o[dt][0] * il, o[dt][1] * il, o[dt][2] * il, o[dt][3] * il);
                const half4 h = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
                const half4 l = {x3_lo(v.x, h[0]), x3_lo(v.y, h[1]), x3_lo(v.z, h[2]), x3_lo(v.w, h[3])};
                const uint2 a = __builtin_bit_cast(uint2, h), b = __builtin_bit_cast(uint2, l);
                const auto r0 = __builtin_amdgcn_permlane16_swap(a.x, b.x, false, false);
                const auto r1 = __builtin_amdgcn_permlane16_swap(a.y, b.y, false, false);
                const int c = hd * 64 + dt * 16 + 4 * (g & ~1);
                if (t < T)
                    *(uint4*)(orow + il_hi(c) + ((g & 1) ? 32 : 0)) = (uint4){r0[0], r1[0], r0[1], r1[1]};
            }
        } else if (t < T) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                put_split4(orow, hd * 64 + dt * 16 + 4 * g, H, kx,
                           make_float4(o[dt][0] * il, o[dt][1] * il, o[dt][2] * il, o[dt][3] * il));
        }
    }
}

// Last layer: one wave per (sequence, head), only the scored query row.  Lanes over keys
// for QK^T, lanes over the 64 head dims for P.V.
template <class QT>
__global__ void __launch_bounds__(64)
attn_query_kernel(const QT* __restrict__ qkv, const QT* __restrict__ qd, const float* __restrict__ x32,
                  const float2* __restrict__ stats, const float* __restrict__ lg,
                  const float* __restrict__ lb, SeqMeta sm, int s0, int row0, int H,
                  f16* __restrict__ ctxq, float* __restrict__ resq, int kx, const f16* __restrict__ himg) {
    __shared__ float sq[64];
    __shared__ float sp[64];
    const int s = s0 + blockIdx.x, h = blockIdx.y;
    const int T = sm.len[s], rs = sm.row[s] - row0, qi = sm.query[s];
    const int lane = threadIdx.x;
    const int ld = 3 * H;
    const QT* base = qkv + (size_t)rs * ld + h * 64;
    // qd: dense [sequence, H] query rows (the last layer projects Q for the scored rows only)
    sq[lane] = (float)(qd ? qd[(size_t)(s - s0) * H + h * 64 + lane] : base[(size_t)qi * ld + lane]) * 0.125f;
    __syncthreads();
    float m = -INFINITY, l = 0.f, acc = 0.f;
    for (int k0 = 0; k0 < T; k0 += 64) {
        const int j = k0 + lane;
        float sc = -INFINITY;
        if (j < T) {
            const QT* kr = base + (size_t)j * ld + H;
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float kv[8];
                load8(kr + c * 8, kv);
#pragma unroll
                for (int e = 0; e < 8; ++e) d += sq[c * 8 + e] * kv[e];
            }
            sc = d;
        }
        const float mn = fmaxf(m, wave_max(sc));
        const float p = (j < T) ? __expf(sc - mn) : 0.f;
        const float alpha = __expf(m - mn);
        l = l * alpha + wave_sum(p);
        acc *= alpha;
        __syncthreads();
        sp[lane] = p;
        __syncthreads();
        const int nk = min(64, T - k0);
        for (int jj = 0; jj < nk; ++jj)
            acc += sp[jj] * (float)base[(size_t)(k0 + jj) * ld + 2 * H + lane];
        m = mn;
    }
    const int s_loc = s - s0;
    put_split(ctxq + (size_t)s_loc * kx * H, h * 64 + lane, H, kx, acc / l);
    {   // residual of the scored row: LN of its pre-LN sum, or the normalised state's image
        const int c = h * 64 + lane;
        const size_t r = (size_t)(rs + qi);
        const float2 hl = himg ? il_parts(himg + r * 2 * H, c) : make_float2(0.f, 0.f);
        resq[(size_t)s_loc * H + c] = himg ? hl.x + hl.y * X3_DOWN : ln_apply(x32[r * H + c], stats[r], lg[c], lb[c]);
    }
}

// Last layer of a multi-mask call: one block of four waves per (sequence, head) serves all of the
// sequence's query rows, wave w the queries w, w + 4, ... of the sequence's list, one at a time and
// each with attn_query_kernel's expression order (lanes over keys for QK^T, lanes over the head
// dims for P.V, 64-key blocks with online softmax), so a query's value does not depend on the
// sequence's other queries.  The four waves re-read the head's K / V rows (T x 128 values, L2
// resident after the first wave); every wave owns one 64-float slice of sq / sp.  The trip counts
// (queries / 4 rounded up, key blocks) are the block's, so every wave reaches every barrier; a
// wave past the list's end recomputes the sequence's first query and stores nothing.
template <class QT>
__global__ void __launch_bounds__(256)
attn_mquery_kernel(const QT* __restrict__ qkv, const QT* __restrict__ qd, const float* __restrict__ x32,
                   const float2* __restrict__ stats, const float* __restrict__ lg, const float* __restrict__ lb,
                   SeqMeta sm, QueryMeta qm, int s0, int H, f16* __restrict__ ctxq, float* __restrict__ resq, int kx,
                   const f16* __restrict__ himg) {
    __shared__ float sq[4][64];
    __shared__ float sp[4][64];
    const int s = s0 + blockIdx.x, h = blockIdx.y;
    const int T = sm.len[s], rs = sm.row[s];
    const int qa = qm.first[s], nqs = qm.first[s + 1] - qa, q0 = qm.first[s0];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ld = 3 * H;
    const QT* base = qkv + (size_t)rs * ld + h * 64;
    for (int i0 = 0; i0 < nqs; i0 += 4) {
        const bool on = i0 + w < nqs;
        const int q = qa + (on ? i0 + w : 0);
        const int qi = qm.pos[q], q_loc = q - q0;
        __syncthreads();
        // qd: dense [query, H] rows (the last layer projects Q for the scored rows only)
        sq[w][lane] = (float)(qd ? qd[(size_t)q_loc * H + h * 64 + lane] : base[(size_t)qi * ld + lane]) * 0.125f;
        __syncthreads();
        float m = -INFINITY, l = 0.f, acc = 0.f;
        for (int k0 = 0; k0 < T; k0 += 64) {
            const int j = k0 + lane;
            float sc = -INFINITY;
            if (j < T) {
                const QT* kr = base + (size_t)j * ld + H;
                float d = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    float kv[8];
                    load8(kr + c * 8, kv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) d += sq[w][c * 8 + e] * kv[e];
                }
                sc = d;
            }
            const float mn = fmaxf(m, wave_max(sc));
            const float p = (j < T) ? __expf(sc - mn) : 0.f;
            const float alpha = __expf(m - mn);
            l = l * alpha + wave_sum(p);
            acc *= alpha;
            __syncthreads();
            sp[w][lane] = p;
            __syncthreads();
            const int nk = min(64, T - k0);
            for (int jj = 0; jj < nk; ++jj)
                acc += sp[w][jj] * (float)base[(size_t)(k0 + jj) * ld + 2 * H + lane];
            m = mn;
        }
        if (on) {
            put_split(ctxq + (size_t)q_loc * kx * H, h * 64 + lane, H, kx, acc / l);
            // residual of the scored row: LN of its pre-LN sum, or the normalised state's image
            const int c = h * 64 + lane;
            const size_t r = (size_t)(rs + qi);
            const float2 hl = himg ? il_parts(himg + r * 2 * H, c) : make_float2(0.f, 0.f);
            resq[(size_t)q_loc * H + c] = himg ? hl.x + hl.y * X3_DOWN : ln_apply(x32[r * H + c], stats[r], lg[c], lb[c]);
        }
    }
}

// ---- folded last layer (RS_LASTFOLD): K / V projections applied to the query side -------------
// K_i = Wk x_i + bk and V_i = Wv x_i + bv are linear in the layer's input rows x_i, and only one
// query row per sequence reads them, so per (sequence, head h)
//   s_i  = q_h . K_i,h / 8 = g_h . x_i + const,   g_h = Wk_h^T q_h / 8   (the constant q_h . bk_h / 8
//                                                  does not depend on i and cancels in the softmax)
//   ctx_h = sum_i p_i V_i,h = Wv_h u_h + bv_h,     u_h = sum_i p_i x_i    (sum_i p_i = 1)
// Three launches: fold_gemm_kernel<false> (G = the g_h of every sequence), attn_fold_kernel
// (softmax and U = the u_h over the two-part image of x), fold_gemm_kernel<true> (ctxq).  No
// K / V row of the chunk is projected.

// Batched fp32 GEMM of the two folds on the f32-input MFMA (exact fp32: every element a fixed-order
// fmaf chain): batch b = blockIdx.z, C_b[M, N] = A_b[M, K] . B_b[K, N], A_b = A + b a_bs rows of lda
// floats (k contiguous), B_b = B + b b_bs rows of ldb floats (n contiguous).  One wave per
// 32 x 64 output tile, four independent waves (row tiles) per workgroup, operands straight from
// global memory into the MFMA fragments: MFMA step kk of a 32-deep K-step takes k = 16 (lane >> 5)
// + kk on both operands, so a lane's 16 A values are 64 contiguous bytes and a half-wave's B values
// of one step 128.  K % 32 == 0, N % 64 == 0 (grid.y = N / 64), rows >= M load row M - 1 and are not
// stored.  IMG: N = 64, C_b + bias[64 b + n] goes to columns 64 b + n of the kx operand image
// img [M, kx Himg] (put_split); else C_b = C + b c_bs, rows of ldc floats.
template <bool IMG>
__global__ void __launch_bounds__(256)
fold_gemm_kernel(const float* __restrict__ A, int lda, int a_bs, const float* __restrict__ B, int ldb, int b_bs,
                 int M, int K, float* __restrict__ C, int ldc, int c_bs, const float* __restrict__ bias,
                 f16* __restrict__ img, int Himg, int kx) {
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    const int m0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32, n0 = blockIdx.y * 64, b = blockIdx.z;
    if (m0 >= M) return;                          // (no barrier in this kernel)
    const float* ap = A + (size_t)b * a_bs + (size_t)min(m0 + c, M - 1) * lda + 16 * h;
    const float* bp = B + (size_t)b * b_bs + (size_t)(16 * h) * ldb + n0 + c;
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 32) {
        float fa[16], fb[2][16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = *(const float4*)(ap + k0 + 4 * q);
            fa[4 * q] = v.x; fa[4 * q + 1] = v.y; fa[4 * q + 2] = v.z; fa[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float* br = bp + (size_t)(k0 + kk) * ldb;
            fb[0][kk] = br[0];
            fb[1][kk] = br[32];
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk], fb[j][kk], acc[j], 0, 0, 0);
    }
    // D map of the 32x32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + 32 * j + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row >= M) continue;
            if constexpr (IMG) put_split(img + (size_t)row * kx * Himg, 64 * b + col, Himg, kx, acc[j][r] + bias[64 * b + col]);
            else C[(size_t)b * c_bs + (size_t)row * ldc + col] = acc[j][r];
        }
    }
}

// Folded last-layer attention of the scored row: one workgroup per sequence, wave h = head h
// (H = 256 NK, 4 NK heads of 64), over the two-part image himg of the layer's input rows.  The
// sequence's rows are staged ONCE for all heads, R at a time, as fp32 hi + lo/64 in LDS; per tile a
// wave forms s_i = g_h . x_i (lane l holds columns 256 k + 4 l .. + 3, k < NK, of g_h, x_i and u_h;
// 4 NK fmaf per lane in a fixed order, then the wave's butterfly sum; lane i keeps s_i), the
// max-shifted probabilities and u_h += p_i x_i, with attn_full_kernel's online rescaling from tile
// to tile (any T; nothing but the trip count depends on it).  No atomics; every sum has one fixed
// order, so the result is the same bits on every run.  U row (s - s0) * heads + h = u_h / l; resq
// as attn_query_kernel forms it from the image.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// Sum over the wave on the DPP network (no LDS traffic, unlike the shuffles of wave_sum): pairs,
// quads, the 16-lane row (rotations by 4 and 8: every lane of a row then holds the row's sum), rows
// 0 + 1 and 2 + 3 (row_bcast:15 into rows 1 and 3), both pairs (row_bcast:31 into rows 2 and 3); the
// total stands in lane 63 and comes back as a scalar.  Masked rows add 0 (old = 0).
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWS, 0xF, false));
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = dpp_add<0xB1, 0xF>(v);      // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E, 0xF>(v);      // quad_perm [2, 3, 0, 1]
    v = dpp_add<0x124, 0xF>(v);     // row_ror:4
    v = dpp_add<0x128, 0xF>(v);     // row_ror:8
    v = dpp_add<0x142, 0xA>(v);     // row_bcast:15
    v = dpp_add<0x143, 0xC>(v);     // row_bcast:31
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
constexpr int FOLD_R = 24;      // staged rows per tile: R H 4 B of LDS (H 768: 72 KiB, two workgroups per CU)
template <int NK>
__global__ void __launch_bounds__(256 * NK, NK <= 3 ? 2 * NK : NK)     // two workgroups per CU where the LDS holds two
attn_fold_kernel(const f16* __restrict__ himg, const float* __restrict__ G, float* __restrict__ U,
                 float* __restrict__ resq, SeqMeta sm, int s0, int row0) {
    constexpr int H = 256 * NK, NT = 256 * NK, R = FOLD_R;
    __shared__ __attribute__((aligned(16))) float sx[R][H];
    const int s = s0 + blockIdx.x, s_loc = blockIdx.x;
    const int T = sm.len[s], rs = sm.row[s] - row0, qi = sm.query[s];
    const int tid = threadIdx.x, lane = tid & 63, hd = tid >> 6;
    const f16* img = himg + (size_t)rs * 2 * H;
    const size_t gu = ((size_t)s_loc * (4 * NK) + hd) * H + 4 * lane;
    f32x4 g[NK], u[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        g[k] = *(const f32x4*)(G + gu + 256 * k);
        u[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float m = -INFINITY, l = 0.f;
    for (int t0 = 0; t0 < T; t0 += R) {
        const int nk = min(R, T - t0);
        // stage rows [t0, t0 + R) (zeros past the sequence's end, so that the row loops below run in
        // whole groups of four): a thread takes 8 columns (one half8 of hi, one of lo) of R / 8 rows
        half8 vh[R / 8], vl[R / 8];
#pragma unroll
        for (int i = 0; i < R / 8; ++i) {
            const int un = tid + i * NT, r = un / (H / 8), c8 = (un % (H / 8)) * 8;
            vh[i] = vl[i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            if (r < nk) {
                const f16* p = img + (size_t)(t0 + r) * 2 * H + il_hi(c8);
                vh[i] = *(const half8*)p;
                vl[i] = *(const half8*)(p + 32);
            }
        }
        __syncthreads();                          // the previous tile's readers are done
#pragma unroll
        for (int i = 0; i < R / 8; ++i) {
            const int un = tid + i * NT, r = un / (H / 8), c8 = (un % (H / 8)) * 8;
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (float)vh[i][e] + (float)vl[i][e] * X3_DOWN;
            *(float4*)&sx[r][c8] = make_float4(x[0], x[1], x[2], x[3]);
            *(float4*)&sx[r][c8 + 4] = make_float4(x[4], x[5], x[6], x[7]);
        }
        __syncthreads();
        // scores, four rows at a time (independent chains): two packed fmaf accumulators per row, then
        // the wave's sum on the DPP network (wave_sum_dpp: one fixed order)
        float sc = -INFINITY;
        for (int r0 = 0; r0 < nk; r0 += 4) {
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x2 a = {0.f, 0.f};
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const f32x4 x = *(const f32x4*)&sx[r0 + j][256 * k + 4 * lane];
                    a = __builtin_elementwise_fma(g[k].xy, x.xy, a);
                    a = __builtin_elementwise_fma(g[k].zw, x.zw, a);
                }
                d[j] = a.x + a.y;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = wave_sum_dpp(d[j]);
                if (lane == r0 + j) sc = t;
            }
        }
        if (lane >= nk) sc = -INFINITY;           // (the zero rows past the end scored 0)
        const float mn = fmaxf(m, wave_max(sc));
        const float p = lane < nk ? __expf(sc - mn) : 0.f;
        const float alpha = __expf(m - mn);       // m = -inf on the first tile -> 0
        l = l * alpha + wave_sum(p);
#pragma unroll
        for (int k = 0; k < NK; ++k) u[k] *= alpha;
        for (int r0 = 0; r0 < nk; r0 += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // p of row r0 + j to every lane (the row index is the wave's: a scalar lane read)
                const float pr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, p), r0 + j));
                const f32x2 pp = {pr, pr};
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const f32x4 x = *(const f32x4*)&sx[r0 + j][256 * k + 4 * lane];
                    u[k].xy = __builtin_elementwise_fma(pp, x.xy, u[k].xy);
                    u[k].zw = __builtin_elementwise_fma(pp, x.zw, u[k].zw);
                }
            }
        }
        m = mn;
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
        *(f32x4*)(U + gu + 256 * k) = f32x4{u[k].x / l, u[k].y / l, u[k].z / l, u[k].w / l};
    {   // residual of the scored row: the normalised state's image
        const int c = hd * 64 + lane;
        const float2 hl = il_parts(img + (size_t)qi * 2 * H, c);
        resq[(size_t)s_loc * H + c] = hl.x + hl.y * X3_DOWN;
    }
}

// Diagnostic: the memory skeleton of attn_tr_kernel (same Q/K/V reads per (sequence, head)
// wave, ctx written) with no math — the access pattern's own cost.
__global__ void __launch_bounds__(256)
attn_memskel_kernel(const f16* __restrict__ qkv, SeqMeta sm, int H, f16* __restrict__ ctx, int heads_per_block) {
    const int s = blockIdx.x;
    const int T = sm.len[s], rs = sm.row[s];
    const int lane = threadIdx.x & 63, hd = blockIdx.y * heads_per_block + (threadIdx.x >> 6);
    const int ld = 3 * H;
    const f16* base = qkv + (size_t)rs * ld + hd * 64;
    for (int r0 = 0; r0 < T; r0 += 8) {
        const int t = r0 + (lane >> 3), d0 = (lane & 7) * 8;
        if (t < T) {
            const half8 q = *(const half8*)(base + (size_t)t * ld + d0);
            const half8 k = *(const half8*)(base + (size_t)t * ld + H + d0);
            const half8 v = *(const half8*)(base + (size_t)t * ld + 2 * H + d0);
            *(half8*)(ctx + (size_t)(rs + t) * H + hd * 64 + d0) = q + k + v;
        }
    }
}

// rs_debug_attention's kernel kinds (the values are the entry's ABI: tests and tools pass integers)
enum AttnKind {
    ATTN_TR = 0,          // attn_tr_kernel<false>
    ATTN_MEMSKEL_1 = 3,   // attn_memskel_kernel, one head per block
    ATTN_MEMSKEL_4 = 4,   //                      four heads per block
    ATTN_16 = 6,          // attn16_kernel<false>
    ATTN_FULL_F32 = 9,    // attn_full_kernel<float>
    ATTN_X3_48 = 10,      // attn16x3v2_kernel<false, 48>
    ATTN_X3_64 = 11,      // attn16x3v2_kernel<false, 64>
};

}  // namespace

hipError_t launch_attention_full(const void* qkv, bool qkv32, SeqMeta sm, int s0, int s1, int row0,
                                 int H, int heads, f16* ctx, int kx, hipStream_t st, bool dedup, int max_len) {
    if (s1 <= s0) return hipSuccess;
    if (H != heads * 64 || max_len <= 0) return hipErrorInvalidValue;
    // dedup (layer 0): fp32 Q/K/V only in the split-operand form (ctx the kx = 2 image) and within
    // one key block; fp16 Q/K/V only with the kx = 1 image (the host gates both)
    if (dedup && (kx != (qkv32 ? 2 : 1) || (qkv32 && max_len > 64))) return hipErrorInvalidValue;
    const dim3 grid(s1 - s0, heads), block(64);
    //  Q/K/V            max_len  kernel(s)                                    D = dedup
    //  fp32             <= 48    attn16x3v2_kernel<D, 48>
    //  fp32             <= 64    attn16x3v2_kernel<D, 64>
    //  fp32, no dedup   >  64    attn16x3v2_kernel<false, 64> (its T <= 64 sequences), then
    //                            attn_full_kernel<float> with skip_le = 64 (the longer ones:
    //                            online softmax over 64-key blocks); each skips the other's
    //  fp32, dedup      >  64    hipErrorInvalidValue (above)
    //  fp16             <= 64    attn16_kernel<D>
    //  fp16             >  64    attn_tr_kernel<D> (16-query tiles re-stage K/V per tile there:
    //                            the 32-query tiles are faster)
    auto route = [&](auto dd) {
        constexpr bool D = decltype(dd)::value;
        if (qkv32) {
            const float* q = (const float*)qkv;
            if (max_len <= 48) hipLaunchKernelGGL((attn16x3v2_kernel<D, 48>), grid, block, 0, st, q, sm, s0, row0, H, ctx, kx);
            else hipLaunchKernelGGL((attn16x3v2_kernel<D, 64>), grid, block, 0, st, q, sm, s0, row0, H, ctx, kx);
            if (max_len > 64) hipLaunchKernelGGL(attn_full_kernel<float>, grid, block, 0, st, q, sm, s0, row0, H, ctx, kx, 64);
        } else {
            const f16* q = (const f16*)qkv;
            if (max_len <= 64) hipLaunchKernelGGL(attn16_kernel<D>, grid, block, 0, st, q, sm, s0, row0, H, ctx, kx);
            else hipLaunchKernelGGL(attn_tr_kernel<D>, grid, block, 0, st, q, sm, s0, row0, H, ctx, kx);
        }
    };
    if (dedup) route(std::true_type{});
    else route(std::false_type{});
    return hipGetLastError();
}

hipError_t launch_attention_query(const void* qkv, bool qkv32, const float* x32, const float2* stats,
                                  const float* g, const float* b, SeqMeta sm, int s0, int s1,
                                  int row0, int H, int heads, f16* ctxq, float* resq, int kx,
                                  hipStream_t st, const void* qd, const f16* himg) {
    if (s1 <= s0) return hipSuccess;
    const dim3 grid(s1 - s0, heads);
    if (qkv32)
        hipLaunchKernelGGL(attn_query_kernel<float>, grid, dim3(64), 0, st, (const float*)qkv, (const float*)qd, x32, stats, g, b, sm, s0, row0, H, ctxq, resq, kx, himg);
    else
        hipLaunchKernelGGL(attn_query_kernel<f16>, grid, dim3(64), 0, st, (const f16*)qkv, (const f16*)qd, x32, stats, g, b, sm, s0, row0, H, ctxq, resq, kx, himg);
    return hipGetLastError();
}

hipError_t launch_attention_mquery(const void* qkv, bool qkv32, const float* x32, const float2* stats, const float* g,
                                   const float* b, SeqMeta sm, QueryMeta qm, int s0, int s1, int H, int heads,
                                   f16* ctxq, float* resq, int kx, hipStream_t st, const void* qd, const f16* himg) {
    if (s1 <= s0) return hipSuccess;
    if (H != heads * 64) return hipErrorInvalidValue;
    const dim3 grid(s1 - s0, heads);
    if (qkv32)
        hipLaunchKernelGGL(attn_mquery_kernel<float>, grid, dim3(256), 0, st, (const float*)qkv, (const float*)qd, x32, stats, g, b, sm, qm, s0, H, ctxq, resq, kx, himg);
    else
        hipLaunchKernelGGL(attn_mquery_kernel<f16>, grid, dim3(256), 0, st, (const f16*)qkv, (const f16*)qd, x32, stats, g, b, sm, qm, s0, H, ctxq, resq, kx, himg);
    return hipGetLastError();
}

namespace {
// dst[s - s0][0, H) = src[row of sequence s's query position][0, H), fp32 rows of ld floats (H % 4 == 0)
__global__ void __launch_bounds__(64)
gather_q32_kernel(const float* __restrict__ src, int ld, SeqMeta sm, int s0, int row0, int H, float* __restrict__ dst) {
    const int s = s0 + blockIdx.x;
    const size_t r = (size_t)(sm.row[s] - row0 + sm.query[s]);
    const float4* a = (const float4*)(src + r * ld);
    float4* o = (float4*)(dst + (size_t)blockIdx.x * H);
    for (int i = threadIdx.x; i < H / 4; i += 64) o[i] = a[i];
}
}  // namespace

hipError_t launch_gather_q32(const float* src, int ld, SeqMeta sm, int s0, int s1, int row0, int H, float* dst,
                             hipStream_t st) {
    if (s1 <= s0) return hipSuccess;
    if (H % 4 || ld % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_q32_kernel, dim3(s1 - s0), dim3(64), 0, st, src, ld, sm, s0, row0, H, dst);
    return hipGetLastError();
}

bool attention_fold_ok(int H, int heads) { return H == heads * 64 && H % 256 == 0 && H <= 1024; }

hipError_t launch_fold_in(const AttnFold& a, int s0, int n, float* G, hipStream_t st) {
    const int H = a.H;
    hipLaunchKernelGGL(fold_gemm_kernel<false>, dim3((n + 127) / 128, H / 64, a.heads), dim3(256), 0, st,
                       a.tq + (size_t)(s0 - a.s0) * H, H, 64, a.wkf, H, 64 * H, n, 64, G, a.heads * H, H, nullptr,
                       nullptr, 0, 0);
    return hipGetLastError();
}

hipError_t launch_fold_query(const AttnFold& a, int s0, int n, const float* G, float* U, hipStream_t st) {
    float* resq = a.resq + (size_t)(s0 - a.s0) * a.H;
    switch (a.H / 256) {
        case 1: hipLaunchKernelGGL(attn_fold_kernel<1>, dim3(n), dim3(256), 0, st, a.himg, G, U, resq, a.sm, s0, a.row0); break;
        case 2: hipLaunchKernelGGL(attn_fold_kernel<2>, dim3(n), dim3(512), 0, st, a.himg, G, U, resq, a.sm, s0, a.row0); break;
        case 3: hipLaunchKernelGGL(attn_fold_kernel<3>, dim3(n), dim3(768), 0, st, a.himg, G, U, resq, a.sm, s0, a.row0); break;
        case 4: hipLaunchKernelGGL(attn_fold_kernel<4>, dim3(n), dim3(1024), 0, st, a.himg, G, U, resq, a.sm, s0, a.row0); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_fold_out(const AttnFold& a, int s0, int n, const float* U, hipStream_t st) {
    const int H = a.H;
    hipLaunchKernelGGL(fold_gemm_kernel<true>, dim3((n + 127) / 128, 1, a.heads), dim3(256), 0, st, U, a.heads * H, H,
                       a.wvt, H, 64, n, H, nullptr, 0, 0, a.bv, a.ctxq + (size_t)(s0 - a.s0) * a.kx * H, H, a.kx);
    return hipGetLastError();
}

// Test entry (not part of the scoring path): the folded last-layer attention through the production
// launcher (launch_attention_fold) over sequences [s0, s1) of the device metadata arrays len / row /
// query.  himg: the two-part image [rows, 2H] of the layer's input, row index = row[s] - row0 + t;
// tq: the dense Q [s1 - s0, H] (bias included); wkf / wvt / bv: the fold's weight images as
// rs_model_finalize builds them (wkf = Wk / 8, wvt = Wv transposed, bv the V bias; fp32); work:
// work_bytes of scratch for G and U (a small one makes the launcher run in several batches); ctxq
// the kx = 1 or 3 image [s1 - s0, kx H], resq fp32 [s1 - s0, H].
extern "C" int rs_debug_attention_fold(const void* himg, const float* tq, const float* wkf, const float* wvt,
                                       const float* bv, const int* len, const int* row, const int* query, int s0,
                                       int s1, int row0, int H, int heads, int kx, void* work, long long work_bytes,
                                       void* ctxq, float* resq, void* stream) {
    if (!himg || !tq || !wkf || !wvt || !bv || !len || !row || !query || !work || !ctxq || !resq) return -1;
    if (s0 < 0 || s1 <= s0 || work_bytes <= 0 || !attention_fold_ok(H, heads) || (kx != 1 && kx != 3)) return -1;
    AttnFold a{};
    a.himg = (const f16*)himg; a.tq = tq; a.wkf = wkf; a.wvt = wvt; a.bv = bv;
    a.sm.len = len; a.sm.row = row; a.sm.query = query;
    a.s0 = s0; a.s1 = s1; a.row0 = row0; a.H = H; a.heads = heads; a.kx = kx;
    a.work = work; a.work_bytes = (size_t)work_bytes; a.ctxq = (f16*)ctxq; a.resq = resq;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = launch_attention_fold(a, st, [](int, double, auto&& launch) { return launch(); });
    return e == hipSuccess ? 0 : -2;
}

// Timing/diagnostic entry (not part of the scoring path): one attention launch over
// sequences [0, n_seq) with an explicit kernel kind (AttnKind; buffer layouts in the file
// comment).  len / row: device int32 arrays.
extern "C" int rs_debug_attention(int kind, const void* qkv, const int* len, const int* row, int n_seq,
                                  int H, int heads, void* ctx, void* stream) {
    SeqMeta sm{};
    sm.len = len;
    sm.row = row;
    const dim3 grid(n_seq, heads), block(64);
    hipStream_t st = (hipStream_t)stream;
    const f16* q16 = (const f16*)qkv;
    const float* q32 = (const float*)qkv;
    f16* c = (f16*)ctx;
    switch (kind) {
        case ATTN_TR: hipLaunchKernelGGL(attn_tr_kernel<false>, grid, block, 0, st, q16, sm, 0, 0, H, c, 1); break;
        case ATTN_16: hipLaunchKernelGGL(attn16_kernel<false>, grid, block, 0, st, q16, sm, 0, 0, H, c, 1); break;
        case ATTN_FULL_F32: hipLaunchKernelGGL(attn_full_kernel<float>, grid, block, 0, st, q32, sm, 0, 0, H, c, 3, 0); break;
        case ATTN_X3_48: hipLaunchKernelGGL((attn16x3v2_kernel<false, 48>), grid, block, 0, st, q32, sm, 0, 0, H, c, 3); break;
        case ATTN_X3_64: hipLaunchKernelGGL((attn16x3v2_kernel<false, 64>), grid, block, 0, st, q32, sm, 0, 0, H, c, 3); break;
        case ATTN_MEMSKEL_1: hipLaunchKernelGGL(attn_memskel_kernel, grid, block, 0, st, q16, sm, H, c, 1); break;
        case ATTN_MEMSKEL_4:
            hipLaunchKernelGGL(attn_memskel_kernel, dim3(n_seq, heads / 4), dim3(256), 0, st, q16, sm, H, c, 4);
            break;
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Test entry (not part of the scoring path): the production attention router on fp32 Q/K/V
// [rows, 3H] over sequences [0, n_seq) — launch_attention_full as rs_api.hip's layer_split calls it for a
// split-operand layer without dedup (kx = 2: ctx the interleaved two-part image [rows, 2H]).
// max_len: the longest sequence of the launch (<= 48 / <= 64: attn16x3v2_kernel with 48 / 64 staged
// key rows; above: the mixed chunk, attn16x3v2_kernel<64> and attn_full_kernel<float> each skipping
// the other's sequences).  len / row: device int32 arrays.
extern "C" int rs_debug_attention_full(const void* qkv32, const int* len, const int* row, int n_seq, int max_len,
                                       int H, int heads, int kx, void* ctx, void* stream) {
    if (!qkv32 || !len || !row || !ctx || n_seq <= 0 || max_len <= 0 || heads <= 0 || H != heads * 64) return -1;
    if (kx != 2 && kx != 3) return -1;
    SeqMeta sm{};
    sm.len = len;
    sm.row = row;
    const hipError_t e = launch_attention_full(qkv32, true, sm, 0, n_seq, 0, H, heads, (f16*)ctx, kx,
                                               (hipStream_t)stream, false, max_len);
    return e == hipSuccess ? 0 : -2;
}

// Test entry (not part of the scoring path): the last layer's scored-row attention through the
// production launcher, over sequences [s0, s1) of the device metadata arrays len / row / query
// (each [>= s1]).  qkv [rows, 3H] fp32 (qkv32 != 0) or fp16, row index = row[s] - row0 + t; qd null or
// the dense Q [s1 - s0, H] of the same type; the residual from (x32 [rows, H], stats [rows], g, b
// [H]) or, himg != null, from the interleaved two-part image [rows, 2H]; ctxq the kx = 1 or 3 image
// [s1 - s0, kx H], resq fp32 [s1 - s0, H].
extern "C" int rs_debug_attention_query(const void* qkv, int qkv32, const int* len, const int* row, const int* query,
                                        int s0, int s1, int row0, int H, int heads, int kx, const void* qd,
                                        const float* x32, const void* stats, const float* g, const float* b,
                                        const void* himg, void* ctxq, float* resq, void* stream) {
    if (!qkv || !len || !row || !query || !ctxq || !resq || s0 < 0 || s1 <= s0 || heads <= 0 || H != heads * 64) return -1;
    if (kx != 1 && kx != 3) return -1;
    if (!himg && (!x32 || !stats || !g || !b)) return -1;
    SeqMeta sm{};
    sm.len = len;
    sm.row = row;
    sm.query = query;
    const hipError_t e = launch_attention_query(qkv, qkv32 != 0, x32, (const float2*)stats, g, b, sm, s0, s1, row0, H, heads,
                                                (f16*)ctxq, resq, kx, (hipStream_t)stream, qd, (const f16*)himg);
    return e == hipSuccess ? 0 : -2;
}

// Test entry (not part of the scoring path): launch_attention_full with every argument given, over
// sequences [s0, s1) of the DebugMeta arrays — dedup != 0: qkv holds the chunk's unique rows (SeqRows:
// urow_h, urow_m, mask_pos, mask_end), else rows row[s] - row0 + t.  ctx: the kx image at rows
// row[s] - row0 + t in both forms.  The launcher's own rejections (dedup with another kx than the
// type's, fp32 dedup past 64 keys) come back as -2.
extern "C" int rs_debug_attention_plan(const void* qkv, int qkv32, const DebugMeta* dm, int s0, int s1, int row0,
                                       int max_len, int H, int heads, int kx, int dedup, void* ctx, void* stream) {
    if (!qkv || !dm || !ctx || !dm->len || !dm->row) return -1;
    if (s0 < 0 || s1 <= s0 || max_len <= 0 || heads <= 0 || H != heads * 64 || kx < 1 || kx > 3) return -1;
    if (dedup && (!dm->urow_h || !dm->urow_m || !dm->mask_pos || !dm->mask_end)) return -1;
    const hipError_t e = launch_attention_full(qkv, qkv32 != 0, debug_seq_meta(*dm), s0, s1, row0, H, heads, (f16*)ctx,
                                               kx, (hipStream_t)stream, dedup != 0, max_len);
    return e == hipSuccess ? 0 : -2;
}

// Test entry (not part of the scoring path): launch_attention_mquery over every query of sequences
// [s0, s1) (DebugMeta: len, row, first, pos).  Arguments as rs_debug_attention_query; qd null or the
// dense Q [queries, H], ctxq / resq row q - first[s0].
extern "C" int rs_debug_attention_mquery(const void* qkv, int qkv32, const DebugMeta* dm, int s0, int s1, int H,
                                         int heads, int kx, const void* qd, const float* x32, const void* stats,
                                         const float* g, const float* b, const void* himg, void* ctxq, float* resq,
                                         void* stream) {
    if (!qkv || !dm || !ctxq || !resq || !dm->len || !dm->row || !dm->first || !dm->pos) return -1;
    if (s0 < 0 || s1 <= s0 || heads <= 0 || H != heads * 64) return -1;
    if (kx != 1 && kx != 3) return -1;
    if (!himg && (!x32 || !stats || !g || !b)) return -1;
    const hipError_t e = launch_attention_mquery(qkv, qkv32 != 0, x32, (const float2*)stats, g, b, debug_seq_meta(*dm),
                                                 debug_query_meta(*dm), s0, s1, H, heads, (f16*)ctxq, resq, kx,
                                                 (hipStream_t)stream, qd, (const f16*)himg);
    return e == hipSuccess ? 0 : -2;
}
