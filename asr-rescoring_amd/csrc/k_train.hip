// Training kernels (RescoreBert distillation training, backward through
// the BERT encoder), with BERT's train-mode dropout (train.h TrDrop).  fp32 throughout — the reference trains in fp32 — with every reduction
// in a fixed order (no float atomics): a training step is bitwise reproducible.
// GEMMs are plain (transposed) fp32 GEMMs on the f32-input MFMA (k_sgemm.hip); everything
// else is here.  One wave per token row for row-wise ops; column reductions in two stages
// (64-row partials, then an ordered sum).
#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "train.h"

namespace {

constexpr float kInvSqrt2= 0.70710678118654752f;
constexpr float kInvSqrt2Pi = 0.39894228040143268f;

template <int NV>
__device__ __forceinline__ void ln_fwd_row(const float4 (&x)[NV], const float* g, const float* b, float eps,
                                           int lane, float2* st, float* h, const TrDrop& dr = TrDrop(),
                                           unsigned long long e0 = 0) {
    constexpr int H = NV * 256;
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) s += (x[v].x + x[v].y) + (x[v].z + x[v].w);
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const float a = x[v].x - mean, bb = x[v].y - mean, c = x[v].z - mean, d = x[v].w - mean;
        q += (a * a + bb * bb) + (c * c + d * d);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
    if (lane == 0) *st = make_float2(mean, rstd);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        const float4 gg = *(const float4*)(g + c), bb = *(const float4*)(b + c);
        float4 o = make_float4((x[v].x - mean) * rstd * gg.x + bb.x, (x[v].y - mean) * rstd * gg.y + bb.y,
                               (x[v].z - mean) * rstd * gg.z + bb.z, (x[v].w - mean) * rstd * gg.w + bb.w);
        if (dr.thresh)
            o = make_float4(tr_drop(dr, e0 + c, o.x), tr_drop(dr, e0 + c + 1, o.y), tr_drop(dr, e0 + c + 2, o.z),
                            tr_drop(dr, e0 + c + 3, o.w));
        *(float4*)(h + c) = o;
    }
}

// x0 = word[tok] + type[row_type, 0 without] + pos[t]; h0 = LN(x0)
template <int NV>
__global__ void __launch_bounds__(256)
tr_embed_ln_kernel(const int* __restrict__ row_tok, const int* __restrict__ row_pos,
                   const int* __restrict__ row_type, int M, int vocab, int type_vocab,
                   const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ typetab,
                   const float* __restrict__ g, const float* __restrict__ b, float eps, float* __restrict__ x0,
                   float2* __restrict__ st, float* __restrict__ h0, TrDrop dr) {
    constexpr int H = NV * 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const int id = min(max(row_tok[row], 0), vocab - 1), t = row_pos[row];
    const float* type0 = typetab + (row_type ? (size_t)min(max(row_type[row], 0), type_vocab - 1) * H : (size_t)0);
    float4 x[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        const float4 w = *(const float4*)(word + (size_t)id * H + c);
        const float4 ty = *(const float4*)(type0 + c);
        const float4 p = *(const float4*)(pos + (size_t)t * H + c);
        x[v] = make_float4((w.x + ty.x) + p.x, (w.y + ty.y) + p.y, (w.z + ty.z) + p.z, (w.w + ty.w) + p.w);
        *(float4*)(x0 + (size_t)row * H + c) = x[v];
    }
    ln_fwd_row<NV>(x, g, b, eps, lane, st + row, h0 + (size_t)row * H, dr, (unsigned long long)row * H);
}

// y <- drop(y + bias) + res (pre-LN, saved), h = LN(y); bias == nullptr: plain LN of y
template <int NV>
__global__ void __launch_bounds__(256)
tr_bias_res_ln_kernel(float* __restrict__ y, const float* bias, const float* res,
                      int M, const float* __restrict__ g, const float* __restrict__ b, float eps,
                      float2* __restrict__ st, float* __restrict__ h, TrDrop dr) {
    constexpr int H = NV * 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    float4 x[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        x[v] = *(const float4*)(y + (size_t)row * H + c);
        if (bias) {
            const float4 bb = *(const float4*)(bias + c);
            const float4 r = *(const float4*)(res + (size_t)row * H + c);
            float4 o = make_float4(x[v].x + bb.x, x[v].y + bb.y, x[v].z + bb.z, x[v].w + bb.w);
            if (dr.thresh) {
                const unsigned long long e = (unsigned long long)row * H + c;
                o = make_float4(tr_drop(dr, e, o.x), tr_drop(dr, e + 1, o.y), tr_drop(dr, e + 2, o.z),
                                tr_drop(dr, e + 3, o.w));
            }
            x[v] = make_float4(o.x + r.x, o.y + r.y, o.z + r.z, o.w + r.w);
            *(float4*)(y + (size_t)row * H + c) = x[v];
        }
    }
    ln_fwd_row<NV>(x, g, b, eps, lane, st + row, h + (size_t)row * H);
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * kInvSqrt2)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
    return 0.5f * (1.0f + erff(x * kInvSqrt2)) + x * kInvSqrt2Pi * __expf(-0.5f * x * x);
}

// pre <- pre + bias; act = gelu(pre)   (N % 4 == 0)
__global__ void tr_bias_gelu_kernel(float* __restrict__ pre, const float* __restrict__ bias, float* __restrict__ act,
                                    long long n4, int N) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)((i * 4) % N);
        float4 v = ((float4*)pre)[i];
        const float4 bb = *(const float4*)(bias + c);
        v = make_float4(v.x + bb.x, v.y + bb.y, v.z + bb.z, v.w + bb.w);
        ((float4*)pre)[i] = v;
        ((float4*)act)[i] = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
    }
}

// dact <- dact * gelu'(pre)
__global__ void tr_gelu_bwd_kernel(float* __restrict__ d, const float* __restrict__ pre, long long n4) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 v = ((float4*)d)[i];
        const float4 p = ((const float4*)pre)[i];
        ((float4*)d)[i] = make_float4(v.x * gelu_erf_grad(p.x), v.y * gelu_erf_grad(p.y), v.z * gelu_erf_grad(p.z),
                                      v.w * gelu_erf_grad(p.w));
    }
}

__global__ void tr_bias_kernel(float* __restrict__ y, const float* __restrict__ bias, long long n4, int N) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)((i * 4) % N);
        float4 v = ((float4*)y)[i];
        const float4 bb = *(const float4*)(bias + c);
        ((float4*)y)[i] = make_float4(v.x + bb.x, v.y + bb.y, v.z + bb.z, v.w + bb.w);
    }
}

// Self-attention forward, one 64-thread block per (sequence, head), thread per query row.
// K and V of the head staged in LDS; P (softmax probabilities) saved for the backward.
// Eager transformers order: scores = (q . k) * scale; softmax = exp(s - max) / sum.
__global__ void __launch_bounds__(64)
tr_attn_fwd_kernel(const float* __restrict__ qkv, const int* __restrict__ seq_off, const int* __restrict__ klen,
                   const long long* __restrict__ pofs, int H, int heads, float* __restrict__ P,
                   float* __restrict__ ctx, TrDrop dr) {
    extern __shared__ __attribute__((aligned(16))) float sm_a[];
    const int s = blockIdx.x, hd = blockIdx.y, tid = threadIdx.x;
    const int r0 = seq_off[s], T = seq_off[s + 1] - r0;
    // keys j >= TK are padding (attention_mask 0): probability exactly 0, as the additive
    // finfo.min mask gives; the backward then carries no gradient to or through them
    const int TK = klen ? min(max(klen[s], 1), T) : T;
    const int ld = 3 * H;
    float* sK = sm_a;                 // [T][64]
    float* sV = sm_a + T * 64;        // [T][64]
    for (int q = tid; q < T * 16; q += 64) {
        const int j = q >> 4, c = (q & 15) * 4;
        const float* rowp = qkv + (size_t)(r0 + j) * ld + hd * 64 + c;
        *(float4*)(sK + j * 64 + c) = *(const float4*)(rowp + H);
        *(float4*)(sV + j * 64 + c) = *(const float4*)(rowp + 2 * H);
    }
    __syncthreads();
    float* Ph = P + pofs[s] + (long long)hd * T * T;
    for (int i = tid; i < T; i += 64) {
        float qv[64];
        const float* qp = qkv + (size_t)(r0 + i) * ld + hd * 64;
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
            const float4 v = *(const float4*)(qp + c);
            qv[c] = v.x; qv[c + 1] = v.y; qv[c + 2] = v.z; qv[c + 3] = v.w;
        }
        float m = -INFINITY;
        for (int j = 0; j < TK; ++j) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < 64; ++c) d += qv[c] * sK[j * 64 + c];
            d *= 0.125f;
            Ph[(long long)i * T + j] = d;
            m = fmaxf(m, d);
        }
        for (int j = TK; j < T; ++j) Ph[(long long)i * T + j] = -INFINITY;
        float sum = 0.f;
        for (int j = 0; j < T; ++j) {
            const float e = j < TK ? __expf(Ph[(long long)i * T + j] - m) : 0.f;
            Ph[(long long)i * T + j] = e;
            sum += e;
        }
        float o[64];
#pragma unroll
        for (int c = 0; c < 64; ++c) o[c] = 0.f;
        const unsigned long long e0 = (unsigned long long)(pofs[s] + (long long)hd * T * T + (long long)i * T);
        for (int j = 0; j < T; ++j) {
            const float p = Ph[(long long)i * T + j] / sum;
            Ph[(long long)i * T + j] = p;          // saved before dropout (the backward's P)
            const float pd = tr_drop(dr, e0 + j, p);
#pragma unroll
            for (int c = 0; c < 64; ++c) o[c] += pd * sV[j * 64 + c];
        }
        float* op = ctx + (size_t)(r0 + i) * H + hd * 64;
#pragma unroll
        for (int c = 0; c < 64; c += 4) *(float4*)(op + c) = make_float4(o[c], o[c + 1], o[c + 2], o[c + 3]);
    }
}

// Attention backward per (sequence, head): dP = dctx V^T, dS = P (dP - rowsum(P dP)),
// dq = scale dS K, dk = scale dS^T Q, dv = P^T dctx.  dS lives in LDS.
__global__ void __launch_bounds__(64)
tr_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ P, const float* __restrict__ dctx,
                   const int* __restrict__ seq_off, const long long* __restrict__ pofs, int H, int heads,
                   float* __restrict__ dqkv, TrDrop dr) {
    extern __shared__ __attribute__((aligned(16))) float sm_a[];
    const int s = blockIdx.x, hd = blockIdx.y, tid = threadIdx.x;
    const int r0 = seq_off[s], T = seq_off[s + 1] - r0;
    const int ld = 3 * H;
    float* sA = sm_a;                 // [T][64]: K (phase 1), Q (phase 2)
    float* sB = sm_a + T * 64;        // [T][64]: V (phase 1), dctx (phase 2)
    float* sS = sm_a + 2 * T * 64;    // [T][T]: dS
    for (int q = tid; q < T * 16; q += 64) {
        const int j = q >> 4, c = (q & 15) * 4;
        const float* rowp = qkv + (size_t)(r0 + j) * ld + hd * 64 + c;
        *(float4*)(sA + j * 64 + c) = *(const float4*)(rowp + H);
        *(float4*)(sB + j * 64 + c) = *(const float4*)(rowp + 2 * H);
    }
    __syncthreads();
    const float* Ph = P + pofs[s] + (long long)hd * T * T;
    for (int i = tid; i < T; i += 64) {
        float g[64];
        const float* gp = dctx + (size_t)(r0 + i) * H + hd * 64;
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
            const float4 v = *(const float4*)(gp + c);
            g[c] = v.x; g[c + 1] = v.y; g[c + 2] = v.z; g[c + 3] = v.w;
        }
        // d(dropped P) = dctx V^T; dP = that * mask * scale
        const unsigned long long e0 = (unsigned long long)(pofs[s] + (long long)hd * T * T + (long long)i * T);
        float rd = 0.f;
        for (int j = 0; j < T; ++j) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < 64; ++c) d += g[c] * sB[j * 64 + c];
            d = tr_drop(dr, e0 + j, d);
            sS[i * T + j] = d;
            rd += Ph[(long long)i * T + j] * d;
        }
        float dq[64];
#pragma unroll
        for (int c = 0; c < 64; ++c) dq[c] = 0.f;
        for (int j = 0; j < T; ++j) {
            const float ds = Ph[(long long)i * T + j] * (sS[i * T + j] - rd);
            sS[i * T + j] = ds;
#pragma unroll
            for (int c = 0; c < 64; ++c) dq[c] += ds * sA[j * 64 + c];
        }
        float* o = dqkv + (size_t)(r0 + i) * ld + hd * 64;
#pragma unroll
        for (int c = 0; c < 64; c += 4)
            *(float4*)(o + c) = make_float4(dq[c] * 0.125f, dq[c + 1] * 0.125f, dq[c + 2] * 0.125f, dq[c + 3] * 0.125f);
    }
    __syncthreads();
    for (int q = tid; q < T * 16; q += 64) {
        const int j = q >> 4, c = (q & 15) * 4;
        *(float4*)(sA + j * 64 + c) = *(const float4*)(qkv + (size_t)(r0 + j) * ld + hd * 64 + c);
        *(float4*)(sB + j * 64 + c) = *(const float4*)(dctx + (size_t)(r0 + j) * H + hd * 64 + c);
    }
    __syncthreads();
    for (int j = tid; j < T; j += 64) {
        float dk[64], dv[64];
#pragma unroll
        for (int c = 0; c < 64; ++c) dk[c] = 0.f, dv[c] = 0.f;
        const unsigned long long eb = (unsigned long long)(pofs[s] + (long long)hd * T * T) + j;
        for (int i = 0; i < T; ++i) {
            // dv uses the dropped probabilities the forward multiplied V by
            const float ds = sS[i * T + j], p = tr_drop(dr, eb + (unsigned long long)i * T, Ph[(long long)i * T + j]);
#pragma unroll
            for (int c = 0; c < 64; ++c) {
                dk[c] += ds * sA[i * 64 + c];
                dv[c] += p * sB[i * 64 + c];
            }
        }
        float* o = dqkv + (size_t)(r0 + j) * ld + hd * 64;
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
            *(float4*)(o + H + c) = make_float4(dk[c] * 0.125f, dk[c + 1] * 0.125f, dk[c + 2] * 0.125f, dk[c + 3] * 0.125f);
            *(float4*)(o + 2 * H + c) = make_float4(dv[c], dv[c + 1], dv[c + 2], dv[c + 3]);
        }
    }
}

// ---- Tiled attention (any T up to max_pos; fixed LDS footprint) ---------------------------------
// The same expressions as the pair above on 64 x 64 tiles and the f32-input MFMA
// (v_mfma_f32_32x32x2_f32: every result an exact k-ordered fp32 fmaf chain).  256 threads, each of
// the four waves owning one 32 x 32 tile of the block's 64 x 64 output: wave w rows 32 (w & 1),
// columns 32 (w >> 1).  Operands are natural row-major [64][kTL] LDS images (rows outside the
// sequence zero-filled), read either with the reduction index contiguous ("KC": a lane's 32
// values of the 64-deep reduction are 8 ds_read_b128; kTL = 68 floats puts the 16 rows of a
// lane group on 16 distinct 16-B slots of the 64 banks) or along it ("MC": ds_read_b32 of 32
// consecutive floats per lane half: conflict-free).  MFMA step kk of lane half h takes reduction
// index 32 h + kk — the same permutation on both operands, so the product is unchanged.
// D map: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
typedef float ta_f32x16 __attribute__((ext_vector_type(16)));
constexpr int kTT = 64, kTL = 68, kTImg = kTT * kTL;

__device__ __forceinline__ void ta_zero(ta_f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// acc[m][n] += sum_k A(m, k) B(n, k) over k = 0..63, m = am0 + (0..31), n = bn0 + (0..31);
// AKC: A(m, k) = a[m][k], else a[k][m]; BKC alike
template <bool AKC, bool BKC>
__device__ __forceinline__ void ta_mma(const float* a, int am0, const float* b, int bn0, int lane, ta_f32x16& acc) {
    const int c = lane & 31, h = lane >> 5;
    float fa[32], fb[32];
    if (AKC) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 v = *(const float4*)(a + (am0 + c) * kTL + 32 * h + 4 * q);
            fa[4 * q] = v.x; fa[4 * q + 1] = v.y; fa[4 * q + 2] = v.z; fa[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) fa[kk] = a[(32 * h + kk) * kTL + am0 + c];
    }
    if (BKC) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 v = *(const float4*)(b + (bn0 + c) * kTL + 32 * h + 4 * q);
            fb[4 * q] = v.x; fb[4 * q + 1] = v.y; fb[4 * q + 2] = v.z; fb[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) fb[kk] = b[(32 * h + kk) * kTL + bn0 + c];
    }
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk], fb[kk], acc, 0, 0, 0);
}

// img[r][0..63] = src[(row0 + r) * ld + 0..63] for row0 + r < rows, else 0 (64 rows; 16-B accesses)
__device__ __forceinline__ void ta_load_rows(float* img, const float* src, size_t ld, int row0, int rows, int tid) {
#pragma unroll
    for (int q = tid; q < kTT * 16; q += 256) {
        const int r = q >> 4, c = (q & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + r < rows) v = *(const float4*)(src + (size_t)(row0 + r) * ld + c);
        *(float4*)(img + r * kTL + c) = v;
    }
}

// img[r][c] = (drop of) src[(i0 + r) * T + j0 + c] inside the T x T matrix, else 0.  e0: the
// dropout element index of src[0] (its place in the saved-P layout).
template <bool DROP>
__device__ __forceinline__ void ta_load_pp(float* img, const float* src, int T, int i0, int j0, int tid,
                                           const TrDrop& dr, unsigned long long e0) {
    const int c = tid & 63;
#pragma unroll 4
    for (int r = tid >> 6; r < kTT; r += 4) {
        float v = 0.f;
        if (i0 + r < T && j0 + c < T) {
            const long long o = (long long)(i0 + r) * T + j0 + c;
            v = src[o];
            if (DROP) v = tr_drop(dr, e0 + (unsigned long long)o, v);
        }
        img[r * kTL + c] = v;
    }
}

// Forward of one (64-query tile, head, sequence): scores of the whole row block into P (pass 1,
// MFMA), a two-pass softmax over the stored row (wave per row), then ctx = drop(P) V (MFMA).
__global__ void __launch_bounds__(256)
tr_attn_fwd_tiled_kernel(const float* __restrict__ qkv, const int* __restrict__ seq_off, const int* __restrict__ klen,
                         const long long* __restrict__ pofs, int H, int heads, float* P, float* __restrict__ ctx,
                         TrDrop dr) {
    __shared__ __attribute__((aligned(16))) float sm[3 * kTImg];
    float *sQ = sm, *sB = sm + kTImg, *sP = sm + 2 * kTImg;
    const int s = blockIdx.z, hd = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = seq_off[s], T = seq_off[s + 1] - r0, q0 = blockIdx.x * kTT;
    if (q0 >= T) return;
    const int TK = klen ? min(max(klen[s], 1), T) : T;
    const size_t ld = 3 * (size_t)H;
    const float* base = qkv + (size_t)r0 * ld + hd * 64;
    const long long pbase = pofs[s] + (long long)hd * T * T;
    float* Ph = P + pbase;
    const int wm = 32 * (wave & 1), wn = 32 * (wave >> 1), c = lane & 31, h = lane >> 5;
    const int nkt = (TK + kTT - 1) / kTT;

    ta_load_rows(sQ, base, ld, q0, T, tid);
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kt * kTT;
        __syncthreads();
        ta_load_rows(sB, base + H, ld, j0, T, tid);
        __syncthreads();
        ta_f32x16 acc;
        ta_zero(acc);
        ta_mma<true, true>(sQ, wm, sB, wn, lane, acc);
        const int j = j0 + wn + c;
        if (j < TK) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = q0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (i < T) Ph[(long long)i * T + j] = acc[r] * 0.125f;
            }
        }
    }
    __syncthreads();
    // softmax of rows q0 + wave, + 4, ...: keys j >= TK are padding, probability exactly 0
    for (int rr = wave; rr < kTT && q0 + rr < T; rr += 4) {
        float* row = Ph + (long long)(q0 + rr) * T;
        float m = -INFINITY;
        for (int j = lane; j < TK; j += 64) m = fmaxf(m, row[j]);
        m = wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < TK; j += 64) {
            const float e = __expf(row[j] - m);
            row[j] = e;
            sum += e;
        }
        sum = wave_sum(sum);
        for (int j = lane; j < T; j += 64) row[j] = j < TK ? row[j] / sum : 0.f;
    }
    ta_f32x16 o;
    ta_zero(o);
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kt * kTT;
        __syncthreads();
        ta_load_rows(sB, base + 2 * H, ld, j0, T, tid);
        ta_load_pp<true>(sP, Ph, T, q0, j0, tid, dr, (unsigned long long)pbase);
        __syncthreads();
        ta_mma<true, false>(sP, wm, sB, wn, lane, o);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = q0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (i < T) ctx[(size_t)(r0 + i) * H + hd * 64 + wn + c] = o[r];
    }
}

// Backward, query side, of one (64-query tile, head, sequence): rd = rowsum(P * drop(dctx V^T))
// (pass 1), then per key tile dS = P (drop(dctx V^T) - rd), stored to dS (the saved-P layout of
// one layer) for the key side, and dQ = 0.125 dS K.  dctx V^T is recomputed in pass 2.
__global__ void __launch_bounds__(256)
tr_attn_bwd_q_tiled_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                           const float* __restrict__ dctx, const int* __restrict__ seq_off,
                           const long long* __restrict__ pofs, int H, int heads, float* __restrict__ dS,
                           float* __restrict__ dqkv, TrDrop dr) {
    __shared__ __attribute__((aligned(16))) float sm[4 * kTImg];
    __shared__ float s_rd[2][kTT];
    float *sG = sm, *sV = sm + kTImg, *sK = sm + 2 * kTImg, *sS = sm + 3 * kTImg;
    const int s = blockIdx.z, hd = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = seq_off[s], T = seq_off[s + 1] - r0, q0 = blockIdx.x * kTT;
    if (q0 >= T) return;
    const size_t ld = 3 * (size_t)H;
    const float* base = qkv + (size_t)r0 * ld + hd * 64;
    const long long pbase = pofs[s] + (long long)hd * T * T;
    const float* Ph = P + pbase;
    float* Sh = dS + pbase;
    const int wm = 32 * (wave & 1), wn = 32 * (wave >> 1), c = lane & 31, h = lane >> 5;
    const int nkt = (T + kTT - 1) / kTT;

    ta_load_rows(sG, dctx + (size_t)r0 * H + hd * 64, (size_t)H, q0, T, tid);
    float rd[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rd[r] = 0.f;
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kt * kTT;
        __syncthreads();
        ta_load_rows(sV, base + 2 * H, ld, j0, T, tid);
        __syncthreads();
        ta_f32x16 acc;
        ta_zero(acc);
        ta_mma<true, true>(sG, wm, sV, wn, lane, acc);
        const int j = j0 + wn + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = q0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (i < T && j < T) {
                const long long o = (long long)i * T + j;
                rd[r] += Ph[o] * tr_drop(dr, (unsigned long long)(pbase + o), acc[r]);
            }
        }
    }
    // a row's sum: the 32 lanes of a half (butterfly), then the two column waves in order
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = rd[r];
#pragma unroll
        for (int d = 16; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        if (c == 0) s_rd[wave >> 1][wm + (r & 3) + 8 * (r >> 2) + 4 * h] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int il = wm + (r & 3) + 8 * (r >> 2) + 4 * h;
        rd[r] = s_rd[0][il] + s_rd[1][il];
    }
    ta_f32x16 dq;
    ta_zero(dq);
    for (int kt = 0; kt < nkt; ++kt) {
        const int j0 = kt * kTT;
        __syncthreads();
        ta_load_rows(sV, base + 2 * H, ld, j0, T, tid);
        ta_load_rows(sK, base + H, ld, j0, T, tid);
        __syncthreads();
        ta_f32x16 acc;
        ta_zero(acc);
        ta_mma<true, true>(sG, wm, sV, wn, lane, acc);
        const int j = j0 + wn + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int il = wm + (r & 3) + 8 * (r >> 2) + 4 * h, i = q0 + il;
            float ds = 0.f;
            if (i < T && j < T) {
                const long long o = (long long)i * T + j;
                ds = Ph[o] * (tr_drop(dr, (unsigned long long)(pbase + o), acc[r]) - rd[r]);
                Sh[o] = ds;
            }
            sS[il * kTL + wn + c] = ds;
        }
        __syncthreads();
        ta_mma<true, false>(sS, wm, sK, wn, lane, dq);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = q0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (i < T) dqkv[(size_t)(r0 + i) * ld + hd * 64 + wn + c] = dq[r] * 0.125f;
    }
}

// Backward, key side, of one (64-key tile, head, sequence): dK = 0.125 dS^T Q and
// dV = drop(P)^T dctx, summed over the query tiles in ascending order in the accumulators
// (no atomics: bitwise reproducible).  A padding key's column of P and dS is 0: its rows are 0.
__global__ void __launch_bounds__(256)
tr_attn_bwd_kv_tiled_kernel(const float* __restrict__ qkv, const float* __restrict__ P,
                            const float* __restrict__ dS, const float* __restrict__ dctx,
                            const int* __restrict__ seq_off, const long long* __restrict__ pofs, int H, int heads,
                            float* __restrict__ dqkv, TrDrop dr) {
    __shared__ __attribute__((aligned(16))) float sm[4 * kTImg];
    float *sQ = sm, *sG = sm + kTImg, *sS = sm + 2 * kTImg, *sP = sm + 3 * kTImg;
    const int s = blockIdx.z, hd = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = seq_off[s], T = seq_off[s + 1] - r0, j0 = blockIdx.x * kTT;
    if (j0 >= T) return;
    const size_t ld = 3 * (size_t)H;
    const float* base = qkv + (size_t)r0 * ld + hd * 64;
    const long long pbase = pofs[s] + (long long)hd * T * T;
    const int wm = 32 * (wave & 1), wn = 32 * (wave >> 1), c = lane & 31, h = lane >> 5;
    const int nqt = (T + kTT - 1) / kTT;
    ta_f32x16 dk, dv;
    ta_zero(dk);
    ta_zero(dv);
    for (int qt = 0; qt < nqt; ++qt) {
        const int i0 = qt * kTT;
        __syncthreads();
        ta_load_rows(sQ, base, ld, i0, T, tid);
        ta_load_rows(sG, dctx + (size_t)r0 * H + hd * 64, (size_t)H, i0, T, tid);
        ta_load_pp<false>(sS, dS + pbase, T, i0, j0, tid, dr, 0);
        ta_load_pp<true>(sP, P + pbase, T, i0, j0, tid, dr, (unsigned long long)pbase);
        __syncthreads();
        ta_mma<false, false>(sS, wm, sQ, wn, lane, dk);
        ta_mma<false, false>(sP, wm, sG, wn, lane, dv);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = j0 + wm + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (j < T) {
            float* o = dqkv + (size_t)(r0 + j) * ld + hd * 64 + wn + c;
            o[H] = dk[r] * 0.125f;
            o[2 * H] = dv[r];
        }
    }
}

// LayerNorm backward for one row: dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)).
// dx may alias dy.
template <int NV>
__global__ void __launch_bounds__(256)
tr_ln_bwd_kernel(const float* dy, const float* __restrict__ x, const float2* __restrict__ st,
                 const float* __restrict__ g, float* dx, int M) {
    constexpr int H = NV * 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float2 s = st[row];
    float4 gd[NV], xh[NV];
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        const float4 d = *(const float4*)(dy + (size_t)row * H + c);
        const float4 xx = *(const float4*)(x + (size_t)row * H + c);
        const float4 gg = *(const float4*)(g + c);
        gd[v] = make_float4(gg.x * d.x, gg.y * d.y, gg.z * d.z, gg.w * d.w);
        xh[v] = make_float4((xx.x - s.x) * s.y, (xx.y - s.x) * s.y, (xx.z - s.x) * s.y, (xx.w - s.x) * s.y);
        a += (gd[v].x + gd[v].y) + (gd[v].z + gd[v].w);
        b += (gd[v].x * xh[v].x + gd[v].y * xh[v].y) + (gd[v].z * xh[v].z + gd[v].w * xh[v].w);
    }
    const float c1 = wave_sum(a) / (float)H, c2 = wave_sum(b) / (float)H;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        *(float4*)(dx + (size_t)row * H + c) =
            make_float4(s.y * (gd[v].x - c1 - xh[v].x * c2), s.y * (gd[v].y - c1 - xh[v].y * c2),
                        s.y * (gd[v].z - c1 - xh[v].z * c2), s.y * (gd[v].w - c1 - xh[v].w * c2));
    }
}

// Column reductions, stage 1: partial[rb][c] over rows [64 rb, 64 rb + 64) in row order.
//   mode 0: sum dy            (bias grads)
//   mode 1: sum dy * xhat     (LN gamma; xhat from x and (mean, rstd)), accumulated as fmaf(dy, xhat, acc),
//           written out in both forms: the contraction the compiler made anyway, now not left to it
// rtype (nullable): row predicate, only rows with rtype[r] == want are summed (the rows are skipped,
// so the order among the rest is the unpredicated one and a type without rows sums to exactly 0).
constexpr int kRB = 64;
__global__ void tr_colsum_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                         const float2* __restrict__ st, int M, int N, int mode,
                                         float* __restrict__ part, const int* __restrict__ rtype, int want) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, rb = blockIdx.y;
    if (c >= N) return;
    const int r0 = rb * kRB, r1 = min(M, r0 + kRB);
    // four interleaved accumulators (rows r % 4), combined in a fixed order: independent
    // loads in flight, still deterministic
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (mode == 0) {
#pragma unroll 8
        for (int r = r0; r < r1; ++r) {
            if (rtype && rtype[r] != want) continue;
            acc[r & 3] += dy[(size_t)r * N + c];
        }
    } else {
#pragma unroll 4
        for (int r = r0; r < r1; ++r) {
            if (rtype && rtype[r] != want) continue;
            const float2 s = st[r];
            acc[r & 3] = fmaf(dy[(size_t)r * N + c], (x[(size_t)r * N + c] - s.x) * s.y, acc[r & 3]);
        }
    }
    part[(size_t)rb * N + c] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// Wide form (N % 4 == 0, every training shape): a block of CL column lanes (float4 each, 4 CL
// columns) x 256 / CL row lanes over a row block, row lane l summing rows r0 + l, r0 + l + RL, ...
// in order, the row lanes then combined through LDS in a fixed order (groups of 8 lanes, then the
// groups): 4x the blocks of the form above at a ~1k-token batch, and every lane's loads
// independent.  Rows <= kOnePass: one row block over all rows (CL = 4: 16 columns a block), written
// straight to the output (accumulate: added to it), no second launch; otherwise kRB4-row blocks
// (CL = 16) and the ordered stage 2 below.  MODE 0: part0 = sum dy; 1: part0 = sum dy * xhat; 2:
// both from one read of dy (LayerNorm gamma into part0, beta into part1).
constexpr int kRB4 = 128, kOnePass = 2048;
template <int MODE, bool ONE>
__global__ void __launch_bounds__(256)
tr_colsum4_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float2* __restrict__ st,
                          int M, int N, float* __restrict__ part0, float* __restrict__ part1, int accumulate,
                          const int* __restrict__ rtype, int want) {
    constexpr int CL = ONE ? 4 : 16, RL = 256 / CL, NQ = MODE == 2 ? 2 : 1;
    __shared__ float4 red[NQ][RL][CL];
    __shared__ float4 red8[NQ][RL / 8][CL];
    const int cl = threadIdx.x % CL, rl = threadIdx.x / CL;
    const int c = blockIdx.x * 4 * CL + cl * 4, rb = blockIdx.y;
    const int r0 = ONE ? 0 : rb * kRB4, r1 = ONE ? M : min(M, r0 + kRB4);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (c < N) {
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += RL) {
            if (rtype && rtype[r] != want) continue;          // row predicate (tr_colsum_partial_kernel)
            const float4 d = *(const float4*)(dy + (size_t)r * N + c);
            if (MODE != 1) {
                b.x += d.x; b.y += d.y; b.z += d.z; b.w += d.w;
            }
            if (MODE != 0) {
                const float2 sr = st[r];
                const float4 xv = *(const float4*)(x + (size_t)r * N + c);
                a.x = fmaf(d.x, (xv.x - sr.x) * sr.y, a.x);
                a.y = fmaf(d.y, (xv.y - sr.x) * sr.y, a.y);
                a.z = fmaf(d.z, (xv.z - sr.x) * sr.y, a.z);
                a.w = fmaf(d.w, (xv.w - sr.x) * sr.y, a.w);
            }
        }
    }
    red[0][rl][cl] = MODE == 0 ? b : a;
    if (MODE == 2) red[NQ - 1][rl][cl] = b;
    __syncthreads();
    auto add8 = [](const float4* v, int stride) {
        float4 t = v[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            const float4 u = v[k * stride];
            t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        return t;
    };
    if (rl < RL / 8)
#pragma unroll
        for (int q = 0; q < NQ; ++q) red8[q][rl][cl] = add8(&red[q][8 * rl][cl], CL);
    __syncthreads();
    if (rl == 0 && c < N) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float4 t = red8[q][0][cl];
#pragma unroll
            for (int k = 1; k < RL / 8; ++k) {
                const float4 v = red8[q][k][cl];
                t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
            }
            float4* o = (float4*)((q == 0 ? part0 : part1) + (size_t)rb * N + c);
            if (ONE && accumulate) {
                const float4 v = *o;
                t.x = v.x + t.x; t.y = v.y + t.y; t.z = v.z + t.z; t.w = v.w + t.w;
            }
            *o = t;
        }
    }
}

// stage 2: out[c] (+)= sum over row blocks in order
__global__ void tr_colsum_final_kernel(const float* __restrict__ part, int nrb, int N, float* __restrict__ out,
                                       int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int rb = 0; rb < nrb; ++rb) acc[rb & 3] += part[(size_t)rb * N + c];
    const float a = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    out[c] = accumulate ? out[c] + a : a;
}

// word-embedding gradient: block per distinct token, its rows summed in row order
__global__ void tr_word_grad_kernel(const float* __restrict__ dx0, const int* __restrict__ utok,
                                    const int* __restrict__ toff, const int* __restrict__ rows, int H,
                                    float* __restrict__ dword) {
    const int u = blockIdx.x;
    const int tk = utok[u], a = toff[u], b = toff[u + 1];
    // nn.Embedding(padding_idx = pad_token_id = 0) in BertEmbeddings: the pad id's lookups
    // pass no gradient to its row (the tied MLM decoder's part is added elsewhere)
    if (tk == 0) return;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        float acc = 0.f;
        for (int k = a; k < b; ++k) acc += dx0[(size_t)rows[k] * H + c];
        dword[(size_t)tk * H + c] += acc;
    }
}

// position-embedding gradient: block per position, sequences in order
__global__ void tr_pos_grad_kernel(const float* __restrict__ dx0, const int* __restrict__ seq_off, int S, int H,
                                   float* __restrict__ dpos) {
    const int p = blockIdx.x;
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        float acc = 0.f;
        for (int s = 0; s < S; ++s)
            if (seq_off[s + 1] - seq_off[s] > p) acc += dx0[(size_t)(seq_off[s] + p) * H + c];
        dpos[(size_t)p * H + c] += acc;
    }
}

// RescoreBert head (RescoreBert/model.py:19-20): score_s = h[CLS_s] . w + b
__global__ void tr_cls_fwd_kernel(const float* __restrict__ h, const int* __restrict__ seq_off, int S, int H,
                                  const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ out) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= S) return;
    const float* hr = h + (size_t)seq_off[s] * H;
    float acc = 0.f;
    for (int c = lane; c < H; c += 64) acc += hr[c] * w[c];
    acc = wave_sum(acc);
    if (lane == 0) out[s] = acc + b[0];
}

// head backward: dh[CLS_s] = dscore_s w (dh zeroed by the caller); dw = sum_s dscore_s h[CLS_s]
// (block per 256 columns, sequences in order); db = sum_s dscore_s
__global__ void tr_cls_bwd_kernel(const float* __restrict__ dsc, const float* __restrict__ h,
                                  const int* __restrict__ seq_off, int S, int H, const float* __restrict__ w,
                                  float* __restrict__ dh, float* __restrict__ dw, float* __restrict__ db) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < H) {
        float acc = 0.f;
        for (int s = 0; s < S; ++s) {
            const float d = dsc[s];
            acc += d * h[(size_t)seq_off[s] * H + c];
            dh[(size_t)seq_off[s] * H + c] = d * w[c];
        }
        dw[c] += acc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float acc = 0.f;
        for (int s = 0; s < S; ++s) acc += dsc[s];
        db[0] += acc;
    }
}

// Distillation losses (single block; groups strided over threads, totals summed by thread 0
// in order).  See train.h for the definitions; every step follows the torch forward /
// autograd sequence of RescoreBert/main.py:104-147 in fp32 (softmax = exp(x - max) / sum,
// log of the softmax OUTPUT for MWED as torch.log(score_distribution) does).
// dsc and uloss are written by one thread and read by another across __syncthreads(): no
// __restrict__ on them, so the compiler cannot move those accesses over the barriers (see
// tr_ce_kernel).
__global__ void tr_loss_kernel(const float* __restrict__ sc, const float* __restrict__ tgt,
                               const float* __restrict__ am, const float* __restrict__ cer,
                               const int* __restrict__ utt_off, int n_utt, int n_hyp, int kind, float md_w,
                               float* dsc, float* uloss, float* __restrict__ loss) {
    const float wmd = kind == RS_LOSS_MD ? 1.0f : md_w;
    for (int h = threadIdx.x; h < n_hyp; h += blockDim.x) dsc[h] = wmd * (2.0f * (sc[h] - tgt[h]));
    __syncthreads();
    if (kind != RS_LOSS_MD) {
        for (int u = threadIdx.x; u < n_utt; u += blockDim.x) {
            const int a = utt_off[u], b = utt_off[u + 1];
            float l = 0.f;
            if (b > a) {
                if (kind == RS_LOSS_MWER) {
                    // P = softmax(mix); MWER_g = sum P (e - sum e / n); d mix = P (d - sum P d)
                    float m = -INFINITY, es = 0.f;
                    for (int i = a; i < b; ++i) { m = fmaxf(m, sc[i] + am[i]); es += cer[i]; }
                    const float avg = es / (float)(b - a);
                    float z = 0.f;
                    for (int i = a; i < b; ++i) z += expf(sc[i] + am[i] - m);
                    for (int i = a; i < b; ++i) l += expf(sc[i] + am[i] - m) / z * (cer[i] - avg);
                    for (int i = a; i < b; ++i) {
                        const float p = expf(sc[i] + am[i] - m) / z;
                        dsc[i] += p * ((cer[i] - avg) - l);
                    }
                } else {
                    // E = softmax(e); T = sum mix / sum e; Q = softmax(mix / T);
                    // KL = sum E (log E - log Q); d z = Q sum E - E; d T = sum d z (-mix / T^2);
                    // d mix = d z / T + d T / sum e
                    float me = -INFINITY, ze = 0.f, smix = 0.f, se = 0.f;
                    for (int i = a; i < b; ++i) { me = fmaxf(me, cer[i]); smix += sc[i] + am[i]; se += cer[i]; }
                    for (int i = a; i < b; ++i) ze += expf(cer[i] - me);
                    const float T = smix / se;
                    float mz = -INFINITY, zq = 0.f;
                    for (int i = a; i < b; ++i) mz = fmaxf(mz, (sc[i] + am[i]) / T);
                    for (int i = a; i < b; ++i) zq += expf((sc[i] + am[i]) / T - mz);
                    float sE = 0.f;
                    for (int i = a; i < b; ++i) sE += expf(cer[i] - me) / ze;
                    float gT = 0.f;
                    for (int i = a; i < b; ++i) {
                        const float mix = sc[i] + am[i];
                        const float E = expf(cer[i] - me) / ze;
                        const float Q = expf(mix / T - mz) / zq;
                        if (E > 0.f) l += E * (logf(E) - logf(Q));
                        const float gz = Q * sE - E;
                        gT += gz * (-mix / (T * T));
                        dsc[i] += gz / T;
                    }
                    for (int i = a; i < b; ++i) dsc[i] += gT / se;
                }
            }
            uloss[u] = l;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float md = 0.f;
        for (int h = 0; h < n_hyp; ++h) md += (sc[h] - tgt[h]) * (sc[h] - tgt[h]);
        float x = 0.f;
        if (kind != RS_LOSS_MD)
            for (int u = 0; u < n_utt; ++u) x += uloss[u];
        loss[0] = kind == RS_LOSS_MD ? md : x + md_w * md;
    }
}

// fixed-tree block reductions (256 threads)
__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] = is_max ? fmaxf(sh[tid], sh[tid + w]) : sh[tid] + sh[tid + w];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// BertForMaskedLM CE (modeling_bert.py:972-975, mean over rows): per row lse - logit[label];
// logits are replaced by d loss / d logits = (softmax - onehot) / M
// The label logit goes through LDS before the first barrier: read from global after the
// reductions (as before), the compiler was free to sink that load past the __syncthreads() that
// precedes the in-place gradient writes (logits was __restrict__), so the row's CE sometimes
// used the thread-(label) gradient instead of the logit — one row's CE off by ~1 in roughly
// one step in four (tools/diag/mlm_first_step.py: 32 of 32 correct after the fix).
__global__ void __launch_bounds__(256)
tr_ce_kernel(float* logits, const int* __restrict__ labels, int M, int V, float* __restrict__ rl) {
    __shared__ float sh[256];
    __shared__ float s_xl;
    const int row = blockIdx.x, tid = threadIdx.x;
    float* x = logits + (size_t)row * V;
    const int lab = min(max(labels[row], 0), V - 1);
    if (tid == 0) s_xl = x[lab];
    float m = -INFINITY;
    for (int j = tid; j < V; j += 256) m = fmaxf(m, x[j]);
    m = block_reduce(m, sh, true);
    float sum = 0.f;
    for (int j = tid; j < V; j += 256) sum += __expf(x[j] - m);
    sum = block_reduce(sum, sh, false);
    const float lse = m + __logf(sum);
    if (tid == 0) rl[row] = lse - s_xl;       // s_xl written before block_reduce's barriers
    __syncthreads();
    const float inv = 1.0f / (float)M;
    for (int j = tid; j < V; j += 256) x[j] = (__expf(x[j] - lse) - (j == lab ? 1.0f : 0.0f)) * inv;
}

__global__ void __launch_bounds__(256) tr_mean_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
    __shared__ float sh[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
    acc = block_reduce(acc, sh, false);
    if (threadIdx.x == 0) out[0] = acc / (float)n;
}

// torch.optim.AdamW step (decoupled decay, bias-corrected, exp_avg via lerp) of one element.  The
// fused multiply-adds are written out: left to -ffp-contract the compiler fused them in the float4
// kernel and not in the scalar one (which it vectorised into separate packed multiplies and adds),
// so the two forms differed in the last bit of m, v and p (tests/test_gpu_train_ops.py).  These are
// the contractions the float4 kernel had.
__device__ __forceinline__ void adamw1(float& pi, float gi, float& mi, float& vi, float decay, float b1w, float b2,
                                       float b2w, float step_size, float bc2_sqrt, float eps) {
    mi = fmaf(b1w, gi - mi, mi);
    vi = fmaf(b2, vi, (b2w * gi) * gi);
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi = fmaf(decay, pi, -(step_size * (mi / denom)));
}

__global__ void tr_adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, long long n, float decay, float b1w, float b2, float b2w,
                                float step_size, float bc2_sqrt, float eps) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float pi = p[i], mi = m[i], vi = v[i];
        adamw1(pi, g[i], mi, vi, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
}

// The same update on float4 quads (16-B aligned arrays, n4 = n / 4 quads; the host runs the
// scalar kernel over the n % 4 tail): every element's arithmetic is the scalar kernel's, bit for
// bit, at 16-B accesses (the scalar form moved its 28 B per parameter at ≈ 63 % of HBM peak)
__global__ void tr_adamw4_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                 float4* __restrict__ v, long long n4, float decay, float b1w, float b2, float b2w,
                                 float step_size, float bc2_sqrt, float eps) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 pi = p[i], mi = m[i], vi = v[i];
        const float4 gi = g[i];
        adamw1(pi.x, gi.x, mi.x, vi.x, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        adamw1(pi.y, gi.y, mi.y, vi.y, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        adamw1(pi.z, gi.z, mi.z, vi.z, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        adamw1(pi.w, gi.w, mi.w, vi.w, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
}

// The AdamW step on a scaled gradient gmul * g (rs_trainer_apply: gradient accumulation's 1/k and
// the clip_grad_norm_ coefficient, folded into one float on the host).  The product is rounded once
// to fp32 before the update, as torch's in-place g.mul_(c) leaves it (__fmul_rn: never contracted
// into adamw1's g - m, so the float4 and scalar forms agree bit for bit as the unscaled pair does).
__global__ void tr_adamw_scaled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                       float* __restrict__ v, long long n, float gmul, float decay, float b1w,
                                       float b2, float b2w, float step_size, float bc2_sqrt, float eps) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float pi = p[i], mi = m[i], vi = v[i];
        adamw1(pi, __fmul_rn(gmul, g[i]), mi, vi, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
}

__global__ void tr_adamw4_scaled_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                        float4* __restrict__ v, long long n4, float gmul, float decay, float b1w,
                                        float b2, float b2w, float step_size, float bc2_sqrt, float eps) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 pi = p[i], mi = m[i], vi = v[i];
        const float4 gi = g[i];
        adamw1(pi.x, __fmul_rn(gmul, gi.x), mi.x, vi.x, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        adamw1(pi.y, __fmul_rn(gmul, gi.y), mi.y, vi.y, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        adamw1(pi.z, __fmul_rn(gmul, gi.z), mi.z, vi.z, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        adamw1(pi.w, __fmul_rn(gmul, gi.w), mi.w, vi.w, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
}

// Gradient accumulation (rs_trainer_accumulate): acc = fmaf(w, g, acc), one rounding per element
// per micro-batch, in the order of the calls.  Scalar and float4 forms, the same arithmetic.
__global__ void tr_accum_kernel(float* __restrict__ acc, const float* __restrict__ g, long long n, float w) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        acc[i] = fmaf(w, g[i], acc[i]);
}

__global__ void tr_accum4_kernel(float4* __restrict__ acc, const float4* __restrict__ g, long long n4, float w) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 a = acc[i];
        const float4 gi = g[i];
        a.x = fmaf(w, gi.x, a.x);
        a.y = fmaf(w, gi.y, a.y);
        a.z = fmaf(w, gi.z, a.z);
        a.w = fmaf(w, gi.w, a.w);
        acc[i] = a;
    }
}

// Sum of squares in float64 (the gradient norm of rs_trainer_grad_norm / rs_trainer_apply), ordered:
// the grid is a function of n alone (at most kSumsqBlocks blocks of 256 threads), thread t of the
// grid sums the squares of its strided share in index order (an fp32 square is exact in float64),
// a wave adds its 64 lanes by a fixed xor butterfly, thread 0 adds the block's 4 waves in wave
// order and writes the block's partial; tr_sumsq_final_kernel adds the partials of all ranges in
// index order.  No atomics: the same buffer gives the same bits on every run and every device.
constexpr int kSumsqBlocks = 512;

template <bool VEC>
__global__ void __launch_bounds__(256)
tr_sumsq_kernel(const float* __restrict__ g, long long n, double* __restrict__ part) {
    __shared__ double sh[4];
    const long long gt = blockIdx.x * 256LL + threadIdx.x, stride = gridDim.x * 256LL;
    double acc = 0.0;
    long long i0 = gt;
    if (VEC) {
        const long long n4 = n / 4;
        const float4* g4 = (const float4*)g;
        for (long long i = gt; i < n4; i += stride) {
            const float4 x = g4[i];
            acc += (double)x.x * (double)x.x;
            acc += (double)x.y * (double)x.y;
            acc += (double)x.z * (double)x.z;
            acc += (double)x.w * (double)x.w;
        }
        i0 = n4 * 4 + gt;                       // the n % 4 tail
    }
    for (long long i = i0; i < n; i += stride) acc += (double)g[i] * (double)g[i];
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ void tr_sumsq_final_kernel(const double* __restrict__ part, int n_part, double* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < n_part; ++i) s += part[i];
        out[0] = s;
    }
}

__global__ void tr_dropout_kernel(float* dst, const float* src, long long n, TrDrop dr) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] = tr_drop(dr, (unsigned long long)i, src[i]);
}

__global__ void tr_dropout_keep_kernel(uint8_t* __restrict__ keep, long long n, TrDrop dr) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        keep[i] = dr.thresh == 0 ? 1 : (uint8_t)tr_keep(dr, (unsigned long long)i);
}

// Labelled-row MLM head (rs_train_step_mlm_labeled): rows of H floats moved as float4 quads (h4 = H / 4
// per row), a flat grid-stride over the quads of the written side, so consecutive lanes move
// consecutive 16 B of one row and every quad of dst has exactly one writer.
// dst[k] = src[rows[k]], k < n (rows validated by the host: in [0, M))
__global__ void __launch_bounds__(256)
tr_gather_rows_kernel(const float4* __restrict__ src, const int* __restrict__ rows, long long n4, int h4,
                      float4* __restrict__ dst) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long k = i / h4;
        const int c = (int)(i - k * h4);
        dst[i] = src[(long long)rows[k] * h4 + c];
    }
}

// dst[r] = inv[r] >= 0 ? src[inv[r]] : 0, r < M: the whole of dst in one pass (no memset + scatter)
__global__ void __launch_bounds__(256)
tr_expand_rows_kernel(const float4* __restrict__ src, const int* __restrict__ inv, long long m4, int h4,
                      float4* __restrict__ dst) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < m4; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / h4;
        const int c = (int)(i - r * h4);
        const int k = inv[r];
        dst[i] = k >= 0 ? src[(long long)k * h4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

int grid_for(long long n, int bs) { return (int)std::min<long long>((n + bs - 1) / bs, 8192); }

}  // namespace

#define RS_NV_SWITCH(H, CALL)                \
    switch (H) {                             \
        case 256: { constexpr int NV = 1; CALL; } break;  \
        case 512: { constexpr int NV = 2; CALL; } break;  \
        case 768: { constexpr int NV = 3; CALL; } break;  \
        case 1024: { constexpr int NV = 4; CALL; } break; \
        default: return hipErrorInvalidValue; \
    }

hipError_t tr_embed_ln(const int* row_tok, const int* row_pos, const int* row_type, int M, int vocab, int type_vocab,
                       const float* word, const float* pos, const float* typetab, const float* g, const float* b,
                       float eps, int H, float* x0, float2* st, float* h0, hipStream_t s, const TrDrop& d) {
    if (M <= 0) return hipSuccess;
    RS_NV_SWITCH(H, hipLaunchKernelGGL(tr_embed_ln_kernel<NV>, dim3((M + 3) / 4), dim3(256), 0, s, row_tok, row_pos,
                                       row_type, M, vocab, type_vocab, word, pos, typetab, g, b, eps, x0, st, h0, d));
    return hipGetLastError();
}

hipError_t tr_bias_res_ln(float* y, const float* bias, const float* res, int M, const float* g, const float* b,
                          float eps, int H, float2* st, float* h, hipStream_t s, const TrDrop& d) {
    if (M <= 0) return hipSuccess;
    RS_NV_SWITCH(H, hipLaunchKernelGGL(tr_bias_res_ln_kernel<NV>, dim3((M + 3) / 4), dim3(256), 0, s, y, bias, res,
                                       M, g, b, eps, st, h, bias ? d : TrDrop()));
    return hipGetLastError();
}

hipError_t tr_bias_gelu(float* pre, const float* bias, float* act, int M, int N, hipStream_t s) {
    const long long n4 = (long long)M * N / 4;
    if (n4 <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_bias_gelu_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, s, pre, bias, act, n4, N);
    return hipGetLastError();
}

hipError_t tr_gelu_bwd(float* d, const float* pre, long long n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_gelu_bwd_kernel, dim3(grid_for(n / 4, 256)), dim3(256), 0, s, d, pre, n / 4);
    return hipGetLastError();
}

hipError_t tr_bias(float* y, const float* bias, int M, int N, hipStream_t s) {
    const long long n4 = (long long)M * N / 4;
    if (n4 <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_bias_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, s, y, bias, n4, N);
    return hipGetLastError();
}

static size_t attn_smem(int tmax, bool bwd) { return (size_t)(2 * tmax * 64 + (bwd ? tmax * tmax : 0)) * 4; }

hipError_t tr_attn_fwd(const float* qkv, const int* seq_off, const int* klen, const long long* pofs, int S,
                       int tmax, int H, int heads, float* P, float* ctx, hipStream_t s, const TrDrop& d) {
    if (S <= 0) return hipSuccess;
    const size_t sm = attn_smem(tmax, false);
    hipError_t e = hipFuncSetAttribute((const void*)tr_attn_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tr_attn_fwd_kernel, dim3(S, heads), dim3(64), sm, s, qkv, seq_off, klen, pofs, H, heads, P, ctx, d);
    return hipGetLastError();
}

hipError_t tr_attn_bwd(const float* qkv, const float* P, const float* dctx, const int* seq_off, const long long* pofs,
                       int S, int tmax, int H, int heads, float* dqkv, hipStream_t s, const TrDrop& d) {
    if (S <= 0) return hipSuccess;
    const size_t sm = attn_smem(tmax, true);
    hipError_t e = hipFuncSetAttribute((const void*)tr_attn_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tr_attn_bwd_kernel, dim3(S, heads), dim3(64), sm, s, qkv, P, dctx, seq_off, pofs, H, heads, dqkv, d);
    return hipGetLastError();
}

// Tiled forms: any tmax, one launch for the whole (mixed-length) batch; blocks past a sequence's
// end exit at once.  The backward's dS scratch has the saved-P layout of one layer (pofs[S] floats).
hipError_t tr_attn_fwd_tiled(const float* qkv, const int* seq_off, const int* klen, const long long* pofs, int S,
                             int tmax, int H, int heads, float* P, float* ctx, hipStream_t s, const TrDrop& d) {
    if (S <= 0 || tmax <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_attn_fwd_tiled_kernel, dim3((tmax + kTT - 1) / kTT, heads, S), dim3(256), 0, s, qkv, seq_off,
                       klen, pofs, H, heads, P, ctx, d);
    return hipGetLastError();
}

hipError_t tr_attn_bwd_tiled(const float* qkv, const float* P, const float* dctx, const int* seq_off,
                             const long long* pofs, int S, int tmax, int H, int heads, float* dS, float* dqkv,
                             hipStream_t s, const TrDrop& d) {
    if (S <= 0 || tmax <= 0) return hipSuccess;
    const dim3 grid((tmax + kTT - 1) / kTT, heads, S);
    hipLaunchKernelGGL(tr_attn_bwd_q_tiled_kernel, grid, dim3(256), 0, s, qkv, P, dctx, seq_off, pofs, H, heads, dS,
                       dqkv, d);
    hipLaunchKernelGGL(tr_attn_bwd_kv_tiled_kernel, grid, dim3(256), 0, s, qkv, P, dS, dctx, seq_off, pofs, H, heads,
                       dqkv, d);
    return hipGetLastError();
}

int rs_fail(int code, const std::string& msg);

// the test entries' dropout key (p = 0: off)
static TrDrop debug_drop(unsigned seed, unsigned long long step, unsigned site, float p) {
    TrDrop d;
    d.seed = seed;
    d.step = (uint32_t)step;
    d.step_hi = (uint32_t)(step >> 32);
    d.site = site;
    d.thresh = p <= 0.f ? 0u : (uint32_t)std::min(4294967295.0, (double)p * 4294967296.0);
    d.scale = (float)(1.0 / (1.0 - (double)p));
    return d;
}

// Test entry: attention forward then backward on caller-provided fp32 qkv [M, 3H] and dctx [M, H]
// (device), seq_off [n_seq + 1] and the nullable klen [n_seq] device int32.  form 0: the
// whole-head kernels (T <= 128); 1: the tiled kernels.  Dropout (seed, step, site, p), p = 0: off.
extern "C" int rs_debug_train_attn(int form, const float* qkv, const int* seq_off, const int* klen, int n_seq, int H,
                                   int heads, const float* dctx, unsigned seed, unsigned long long step, unsigned site,
                                   float p, float* ctx, float* dqkv, void* stream) {
    if (!qkv || !seq_off || !dctx || !ctx || !dqkv || n_seq <= 0) return rs_fail(RS_EARG, "null argument / empty batch");
    if (form < 0 || form > 1) return rs_fail(RS_EARG, "form must be 0 or 1");
    if (heads <= 0 || H != heads * 64) return rs_fail(RS_EUNSUP, "head_dim must be 64");
    if (!(p >= 0.f && p < 1.f)) return rs_fail(RS_EARG, "p must be in [0, 1)");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> off(n_seq + 1);
    if (hipMemcpyAsync(off.data(), seq_off, off.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return rs_fail(RS_EHIP, "rs_debug_train_attn: reading seq_off");
    std::vector<long long> pofs(n_seq + 1, 0);
    int tmax = 0;
    for (int s = 0; s < n_seq; ++s) {
        const long long T = off[s + 1] - off[s];
        if (off[0] != 0 || T < 1) return rs_fail(RS_EARG, "offsets must start at 0 and ascend");
        tmax = std::max(tmax, (int)T);
        pofs[s + 1] = pofs[s] + (long long)heads * T * T;
    }
    if (form == 0 && tmax > 128) return rs_fail(RS_EUNSUP, "form 0 is limited to 128 tokens");
    const TrDrop d = debug_drop(seed, step, site, p);
    // scratch (pofs | P | dS): kept and grown between calls, so a timing loop over this entry
    // (tools/train_attn_bench.py) measures the kernels and not hipMalloc / hipFree
    static void* buf = nullptr;
    static size_t buf_bytes = 0;
    const size_t np = (size_t)pofs[n_seq], meta = ((size_t)(n_seq + 1) * 8 + 255) & ~(size_t)255;
    const size_t need = meta + np * 4 * (form == 1 ? 2 : 1);
    if (need > buf_bytes) {
        if (buf) (void)hipFree(buf);
        buf = nullptr;
        buf_bytes = 0;
        if (hipMalloc(&buf, need) != hipSuccess) {
            (void)hipGetLastError();
            return rs_fail(RS_ENOMEM, "rs_debug_train_attn: scratch");
        }
        buf_bytes = need;
    }
    long long* d_pofs = (long long*)buf;
    float* P = (float*)((char*)buf + meta);
    hipError_t e = hipMemcpyAsync(d_pofs, pofs.data(), pofs.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = form == 1 ? tr_attn_fwd_tiled(qkv, seq_off, klen, d_pofs, n_seq, tmax, H, heads, P, ctx, st, d)
                      : tr_attn_fwd(qkv, seq_off, klen, d_pofs, n_seq, tmax, H, heads, P, ctx, st, d);
    if (e == hipSuccess)
        e = form == 1 ? tr_attn_bwd_tiled(qkv, P, dctx, seq_off, d_pofs, n_seq, tmax, H, heads, P + np, dqkv, st, d)
                      : tr_attn_bwd(qkv, P, dctx, seq_off, d_pofs, n_seq, tmax, H, heads, dqkv, st, d);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return rs_fail(RS_EHIP, std::string("rs_debug_train_attn: ") + hipGetErrorString(e));
    return RS_OK;
}

hipError_t tr_ln_bwd(const float* dy, const float* x, const float2* st, const float* g, float* dx, int M, int H,
                     hipStream_t s) {
    if (M <= 0) return hipSuccess;
    RS_NV_SWITCH(H, hipLaunchKernelGGL(tr_ln_bwd_kernel<NV>, dim3((M + 3) / 4), dim3(256), 0, s, dy, x, st, g, dx, M));
    return hipGetLastError();
}

// floats: the kRB-row partials of tr_colsum's narrow form, or two arrays of kRB4-row partials
size_t tr_colsum_scratch(int M, int N) {
    return std::max((size_t)((M + kRB - 1) / kRB), (size_t)2 * ((M + kRB4 - 1) / kRB4)) * N * 4;
}

hipError_t tr_colsum(const float* dy, const float* x, const float2* st, int M, int N, int mode, float* part,
                     float* out, int accumulate, hipStream_t s, const int* rtype, int want) {
    if (M <= 0 || N <= 0) return hipSuccess;
    if (N % 4 == 0) {
        const dim3 g1((N + 63) / 64), g16((N + 15) / 16);
        if (M <= kOnePass) {
            if (mode == 0)
                hipLaunchKernelGGL((tr_colsum4_partial_kernel<0, true>), g16, dim3(256), 0, s, dy, x, st, M, N, out, out, accumulate, rtype, want);
            else
                hipLaunchKernelGGL((tr_colsum4_partial_kernel<1, true>), g16, dim3(256), 0, s, dy, x, st, M, N, out, out, accumulate, rtype, want);
            return hipGetLastError();
        }
        const int nrb = (M + kRB4 - 1) / kRB4;
        if (mode == 0)
            hipLaunchKernelGGL((tr_colsum4_partial_kernel<0, false>), dim3(g1.x, nrb), dim3(256), 0, s, dy, x, st, M, N, part, part, 0, rtype, want);
        else
            hipLaunchKernelGGL((tr_colsum4_partial_kernel<1, false>), dim3(g1.x, nrb), dim3(256), 0, s, dy, x, st, M, N, part, part, 0, rtype, want);
        hipLaunchKernelGGL(tr_colsum_final_kernel, g1, dim3(64), 0, s, part, nrb, N, out, accumulate);
        return hipGetLastError();
    }
    const int nrb = (M + kRB - 1) / kRB;
    hipLaunchKernelGGL(tr_colsum_partial_kernel, dim3((N + 255) / 256, nrb), dim3(256), 0, s, dy, x, st, M, N, mode, part, rtype, want);
    hipLaunchKernelGGL(tr_colsum_final_kernel, dim3((N + 63) / 64), dim3(64), 0, s, part, nrb, N, out, accumulate);
    return hipGetLastError();
}

// LayerNorm gamma (sum dy * xhat) and beta (sum dy) gradients from one read of dy: the two
// tr_colsum calls' results bit for bit (the same per-column order), half the dy reads and launches
hipError_t tr_colsum_ln(const float* dy, const float* x, const float2* st, int M, int N, float* part, float* out_g,
                        float* out_b, hipStream_t s) {
    if (M <= 0 || N <= 0) return hipSuccess;
    if (N % 4) {
        if (hipError_t e = tr_colsum(dy, x, st, M, N, 1, part, out_g, 0, s)) return e;
        return tr_colsum(dy, nullptr, nullptr, M, N, 0, part, out_b, 0, s);
    }
    if (M <= kOnePass) {
        hipLaunchKernelGGL((tr_colsum4_partial_kernel<2, true>), dim3((N + 15) / 16), dim3(256), 0, s, dy, x, st, M, N, out_g,
                           out_b, 0, nullptr, 0);
        return hipGetLastError();
    }
    const int nrb = (M + kRB4 - 1) / kRB4;
    float* part_b = part + (size_t)nrb * N;         // tr_colsum_scratch: room for two
    hipLaunchKernelGGL((tr_colsum4_partial_kernel<2, false>), dim3((N + 63) / 64, nrb), dim3(256), 0, s, dy, x, st, M, N, part,
                       part_b, 0, nullptr, 0);
    hipLaunchKernelGGL(tr_colsum_final_kernel, dim3((N + 63) / 64), dim3(64), 0, s, part, nrb, N, out_g, 0);
    hipLaunchKernelGGL(tr_colsum_final_kernel, dim3((N + 63) / 64), dim3(64), 0, s, part_b, nrb, N, out_b, 0);
    return hipGetLastError();
}

hipError_t tr_word_grad(const float* dx0, const int* utok, const int* toff, const int* rows, int n_uniq, int H,
                        float* dword, hipStream_t s) {
    if (n_uniq <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_word_grad_kernel, dim3(n_uniq), dim3(256), 0, s, dx0, utok, toff, rows, H, dword);
    return hipGetLastError();
}

hipError_t tr_pos_grad(const float* dx0, const int* seq_off, int S, int tmax, int H, float* dpos, hipStream_t s) {
    if (S <= 0 || tmax <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_pos_grad_kernel, dim3(tmax), dim3(256), 0, s, dx0, seq_off, S, H, dpos);
    return hipGetLastError();
}

hipError_t tr_cls_fwd(const float* h, const int* seq_off, int S, int H, const float* w, const float* b, float* out,
                      hipStream_t s) {
    if (S <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_cls_fwd_kernel, dim3((S + 3) / 4), dim3(256), 0, s, h, seq_off, S, H, w, b, out);
    return hipGetLastError();
}

hipError_t tr_cls_bwd(const float* dsc, const float* h, const int* seq_off, int S, int H, const float* w, float* dh,
                      float* dw, float* db, hipStream_t s) {
    hipLaunchKernelGGL(tr_cls_bwd_kernel, dim3((H + 255) / 256), dim3(256), 0, s, dsc, h, seq_off, S, H, w, dh, dw, db);
    return hipGetLastError();
}

hipError_t tr_loss(const float* sc, const float* tgt, const float* am, const float* err, const int* utt_off,
                   int n_utt, int n_hyp, int kind, float md_w, float* dsc, float* uloss, float* loss, hipStream_t s) {
    hipLaunchKernelGGL(tr_loss_kernel, dim3(1), dim3(256), 0, s, sc, tgt, am, err, utt_off, n_utt, n_hyp, kind, md_w,
                       dsc, uloss, loss);
    return hipGetLastError();
}

hipError_t tr_ce(float* logits, const int* labels, int M, int V, float* row_loss, float* loss, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_ce_kernel, dim3(M), dim3(256), 0, s, logits, labels, M, V, row_loss);
    hipLaunchKernelGGL(tr_mean_kernel, dim3(1), dim3(256), 0, s, row_loss, M, loss);
    return hipGetLastError();
}

hipError_t tr_adamw(float* p, const float* g, float* m, float* v, long long n, float decay, float b1w, float b2,
                    float b2w, float step_size, float bc2_sqrt, float eps, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && n >= 4) {
        const long long n4 = n / 4, done = n4 * 4;
        hipLaunchKernelGGL(tr_adamw4_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, s, (float4*)p, (const float4*)g,
                           (float4*)m, (float4*)v, n4, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        if (done < n)
            hipLaunchKernelGGL(tr_adamw_kernel, dim3(1), dim3(64), 0, s, p + done, g + done, m + done, v + done, n - done,
                               decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(tr_adamw_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, p, g, m, v, n, decay, b1w, b2, b2w,
                       step_size, bc2_sqrt, eps);
    return hipGetLastError();
}

hipError_t tr_adamw_scaled(float* p, const float* g, float* m, float* v, long long n, float gmul, float decay,
                           float b1w, float b2, float b2w, float step_size, float bc2_sqrt, float eps, hipStream_t s) {
    if (gmul == 1.0f) return tr_adamw(p, g, m, v, n, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps, s);
    if (n <= 0) return hipSuccess;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && n >= 4) {
        const long long n4 = n / 4, done = n4 * 4;
        hipLaunchKernelGGL(tr_adamw4_scaled_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, s, (float4*)p,
                           (const float4*)g, (float4*)m, (float4*)v, n4, gmul, decay, b1w, b2, b2w, step_size,
                           bc2_sqrt, eps);
        if (done < n)
            hipLaunchKernelGGL(tr_adamw_scaled_kernel, dim3(1), dim3(64), 0, s, p + done, g + done, m + done, v + done,
                               n - done, gmul, decay, b1w, b2, b2w, step_size, bc2_sqrt, eps);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(tr_adamw_scaled_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, p, g, m, v, n, gmul, decay, b1w,
                       b2, b2w, step_size, bc2_sqrt, eps);
    return hipGetLastError();
}

hipError_t tr_accum(float* acc, const float* g, long long n, float w, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if ((((uintptr_t)acc | (uintptr_t)g) & 15) == 0 && n >= 4) {
        const long long n4 = n / 4, done = n4 * 4;
        hipLaunchKernelGGL(tr_accum4_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, s, (float4*)acc, (const float4*)g,
                           n4, w);
        if (done < n)
            hipLaunchKernelGGL(tr_accum_kernel, dim3(1), dim3(64), 0, s, acc + done, g + done, n - done, w);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(tr_accum_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, acc, g, n, w);
    return hipGetLastError();
}

size_t tr_sumsq_ws_doubles(int n_ranges) { return 1 + (size_t)std::max(n_ranges, 0) * kSumsqBlocks; }

hipError_t tr_sumsq(const float* base, const TrRange* r, int n_ranges, double* ws, hipStream_t s) {
    int n_part = 0;
    for (int k = 0; k < n_ranges; ++k) {
        if (r[k].n <= 0) continue;
        const float* g = base + r[k].off;
        const bool vec = ((uintptr_t)g & 15) == 0 && r[k].n >= 4;
        const long long items = vec ? r[k].n / 4 : r[k].n;
        const int nb = (int)std::min<long long>((items + 255) / 256, kSumsqBlocks);
        if (vec)
            hipLaunchKernelGGL(tr_sumsq_kernel<true>, dim3(nb), dim3(256), 0, s, g, r[k].n, ws + 1 + n_part);
        else
            hipLaunchKernelGGL(tr_sumsq_kernel<false>, dim3(nb), dim3(256), 0, s, g, r[k].n, ws + 1 + n_part);
        n_part += nb;
    }
    hipLaunchKernelGGL(tr_sumsq_final_kernel, dim3(1), dim3(64), 0, s, ws + 1, n_part, ws);
    return hipGetLastError();
}

hipError_t tr_dropout(float* dst, const float* src, long long n, const TrDrop& d, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_dropout_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, dst, src, n, d);
    return hipGetLastError();
}

hipError_t tr_gather_rows(const float* src, const int* rows, int n, int H, float* dst, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (H <= 0 || H % 4 || ((uintptr_t)src | (uintptr_t)dst) % 16) return hipErrorInvalidValue;
    const long long n4 = (long long)n * (H / 4);
    hipLaunchKernelGGL(tr_gather_rows_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, s, (const float4*)src, rows, n4,
                       H / 4, (float4*)dst);
    return hipGetLastError();
}

hipError_t tr_expand_rows(const float* src, const int* inv, int M, int H, float* dst, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (H <= 0 || H % 4 || ((uintptr_t)src | (uintptr_t)dst) % 16) return hipErrorInvalidValue;
    const long long m4 = (long long)M * (H / 4);
    hipLaunchKernelGGL(tr_expand_rows_kernel, dim3(grid_for(m4, 256)), dim3(256), 0, s, (const float4*)src, inv, m4,
                       H / 4, (float4*)dst);
    return hipGetLastError();
}

hipError_t tr_dropout_keep(uint8_t* keep, long long n, const TrDrop& d, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(tr_dropout_keep_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, keep, n, d);
    return hipGetLastError();
}

// ---- Test entries for the non-attention kernels (tests/test_gpu_train_ops.py) -------------------
// Each runs the launchers above — the functions train_api.hip calls, nothing re-implemented — on
// caller-provided device buffers (fp32 / int32) and synchronises.  The kernels trust the trainer's
// host code for their index arrays, so the entries read those back and range-check them first: a
// bad test input is RS_EARG, not a fault.  Sizes of the float buffers are the caller's promise.
namespace {

bool dbg_h(int H) { return H == 256 || H == 512 || H == 768 || H == 1024; }

int dbg_ints(const int* d, size_t n, std::vector<int>& h, hipStream_t st) {
    h.resize(n);
    if (n == 0) return RS_OK;
    if (hipMemcpyAsync(h.data(), d, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return rs_fail(RS_EHIP, "test entry: reading an index array");
    return RS_OK;
}

// offsets: start at 0, ascend (strict: every segment non-empty), end at `end`
bool dbg_offsets(const std::vector<int>& o, bool strict, long long end) {
    if (o.empty() || o[0] != 0 || o.back() != end) return false;
    for (size_t i = 1; i < o.size(); ++i)
        if (o[i] < o[i - 1] + (strict ? 1 : 0)) return false;
    return true;
}

bool dbg_in_range(const std::vector<int>& v, long long lo, long long hi) {       // every value in [lo, hi)
    for (int x : v)
        if (x < lo || x >= hi) return false;
    return true;
}

int dbg_done(hipError_t e, hipStream_t st, const char* what) {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return rs_fail(RS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    return RS_OK;
}

bool dbg_p(float p) { return p >= 0.f && p < 1.f; }

}  // namespace

// x0 [M, H], st [M, 2] (mean, rstd), h0 [M, H] of tr_embed_ln; word [vocab, H], pos [max_pos, H],
// typetab [type_vocab, H]; row_type nullable.  Dropout (seed, step, site, p), p = 0: off.
extern "C" int rs_debug_train_embed_ln(const int* row_tok, const int* row_pos, const int* row_type, int M, int vocab,
                                       int type_vocab, int max_pos, const float* word, const float* pos,
                                       const float* typetab, const float* g, const float* b, float eps, int H,
                                       unsigned seed, unsigned long long step, unsigned site, float p, float* x0,
                                       float* st, float* h0, void* stream) {
    if (!row_tok || !row_pos || !word || !pos || !typetab || !g || !b || !x0 || !st || !h0)
        return rs_fail(RS_EARG, "null argument");
    if (M <= 0 || vocab <= 0 || type_vocab <= 0 || max_pos <= 0) return rs_fail(RS_EARG, "empty shape");
    if (!dbg_h(H)) return rs_fail(RS_EUNSUP, "hidden must be 256, 512, 768 or 1024");
    if (!dbg_p(p)) return rs_fail(RS_EARG, "p must be in [0, 1)");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> hp;
    if (int r = dbg_ints(row_pos, (size_t)M, hp, s)) return r;
    if (!dbg_in_range(hp, 0, max_pos)) return rs_fail(RS_EARG, "row_pos outside [0, max_pos)");
    return dbg_done(tr_embed_ln(row_tok, row_pos, row_type, M, vocab, type_vocab, word, pos, typetab, g, b, eps, H,
                                x0, (float2*)st, h0, s, debug_drop(seed, step, site, p)),
                    s, "rs_debug_train_embed_ln");
}

// y [M, H] in place, st [M, 2], h [M, H] of tr_bias_res_ln; bias == null: plain LayerNorm of y
// (res unused, no dropout)
extern "C" int rs_debug_train_bias_res_ln(float* y, const float* bias, const float* res, int M, const float* g,
                                          const float* b, float eps, int H, unsigned seed, unsigned long long step,
                                          unsigned site, float p, float* st, float* h, void* stream) {
    if (!y || !g || !b || !st || !h || (bias && !res)) return rs_fail(RS_EARG, "null argument");
    if (M <= 0) return rs_fail(RS_EARG, "empty shape");
    if (!dbg_h(H)) return rs_fail(RS_EUNSUP, "hidden must be 256, 512, 768 or 1024");
    if (!dbg_p(p)) return rs_fail(RS_EARG, "p must be in [0, 1)");
    hipStream_t s = (hipStream_t)stream;
    return dbg_done(tr_bias_res_ln(y, bias, res, M, g, b, eps, H, (float2*)st, h, s, debug_drop(seed, step, site, p)),
                    s, "rs_debug_train_bias_res_ln");
}

// dx [M, H] of tr_ln_bwd (dx may be dy)
extern "C" int rs_debug_train_ln_bwd(const float* dy, const float* x, const float* st, const float* g, float* dx,
                                     int M, int H, void* stream) {
    if (!dy || !x || !st || !g || !dx) return rs_fail(RS_EARG, "null argument");
    if (M <= 0) return rs_fail(RS_EARG, "empty shape");
    if (!dbg_h(H)) return rs_fail(RS_EUNSUP, "hidden must be 256, 512, 768 or 1024");
    hipStream_t s = (hipStream_t)stream;
    return dbg_done(tr_ln_bwd(dy, x, (const float2*)st, g, dx, M, H, s), s, "rs_debug_train_ln_bwd");
}

// op 0: tr_bias_gelu(pre = a, bias = v, act = c); 1: tr_gelu_bwd(d = a, pre = v); 2: tr_bias(y = a,
// bias = v).  a, c [M, N]; v [N] (op 1: [M, N]).
extern "C" int rs_debug_train_pointwise(int op, float* a, const float* v, float* c, int M, int N, void* stream) {
    if (op < 0 || op > 2) return rs_fail(RS_EARG, "op must be 0, 1 or 2");
    if (!a || !v || (op == 0 && !c)) return rs_fail(RS_EARG, "null argument");
    if (M <= 0 || N <= 0) return rs_fail(RS_EARG, "empty shape");
    if (N % 4) return rs_fail(RS_EUNSUP, "N must be a multiple of 4");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = op == 0 ? tr_bias_gelu(a, v, c, M, N, s)
                         : op == 1 ? tr_gelu_bwd(a, v, (long long)M * N, s)
                                   : tr_bias(a, v, M, N, s);
    return dbg_done(e, s, "rs_debug_train_pointwise");
}

// op 0 / 1: tr_colsum of that mode into out [N] (accumulate: added to it), over the rows with
// rtype[r] == want when rtype is given; op 2: tr_colsum_ln into out (gamma) and out_b (beta).
// dy, x [M, N], st [M, 2] (x, st: ops 1 and 2).  The scratch is sized by tr_colsum_scratch.
extern "C" int rs_debug_train_colsum(int op, const float* dy, const float* x, const float* st, int M, int N,
                                     float* out, float* out_b, int accumulate, const int* rtype, int want,
                                     void* stream) {
    if (op < 0 || op > 2) return rs_fail(RS_EARG, "op must be 0, 1 or 2");
    if (!dy || !out || (op != 0 && (!x || !st)) || (op == 2 && !out_b)) return rs_fail(RS_EARG, "null argument");
    if (op == 2 && (rtype || accumulate)) return rs_fail(RS_EARG, "tr_colsum_ln takes no row predicate / accumulate");
    if (M <= 0 || N <= 0) return rs_fail(RS_EARG, "empty shape");
    hipStream_t s = (hipStream_t)stream;
    float* part = nullptr;
    if (hipMalloc((void**)&part, tr_colsum_scratch(M, N)) != hipSuccess) {
        (void)hipGetLastError();
        return rs_fail(RS_ENOMEM, "rs_debug_train_colsum: scratch");
    }
    const hipError_t e = op == 2 ? tr_colsum_ln(dy, x, (const float2*)st, M, N, part, out, out_b, s)
                                 : tr_colsum(dy, x, (const float2*)st, M, N, op, part, out, accumulate, s, rtype, want);
    const int r = dbg_done(e, s, "rs_debug_train_colsum");
    (void)hipFree(part);
    return r;
}

// dword [vocab, H] += tr_word_grad of dx0 [M, H]: utok [n_uniq] distinct token ids, toff
// [n_uniq + 1] offsets into rows (the row indices of each token, in row order)
extern "C" int rs_debug_train_word_grad(const float* dx0, const int* utok, const int* toff, const int* rows,
                                        int n_uniq, int M, int vocab, int H, float* dword, void* stream) {
    if (!dx0 || !utok || !toff || !rows || !dword) return rs_fail(RS_EARG, "null argument");
    if (n_uniq <= 0 || M <= 0 || vocab <= 0 || H <= 0) return rs_fail(RS_EARG, "empty shape");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> hu, ho, hr;
    if (int r = dbg_ints(utok, (size_t)n_uniq, hu, s)) return r;
    if (int r = dbg_ints(toff, (size_t)n_uniq + 1, ho, s)) return r;
    if (!dbg_in_range(hu, 0, vocab) || ho[0] != 0 || !dbg_offsets(ho, false, ho.back()))
        return rs_fail(RS_EARG, "token ids / offsets out of range");
    if (int r = dbg_ints(rows, (size_t)ho.back(), hr, s)) return r;
    if (!dbg_in_range(hr, 0, M)) return rs_fail(RS_EARG, "row index outside [0, M)");
    return dbg_done(tr_word_grad(dx0, utok, toff, rows, n_uniq, H, dword, s), s, "rs_debug_train_word_grad");
}

// dpos [tmax, H] += tr_pos_grad of dx0 [seq_off[S], H]
extern "C" int rs_debug_train_pos_grad(const float* dx0, const int* seq_off, int S, int M, int tmax, int H,
                                       float* dpos, void* stream) {
    if (!dx0 || !seq_off || !dpos) return rs_fail(RS_EARG, "null argument");
    if (S <= 0 || M <= 0 || tmax <= 0 || H <= 0) return rs_fail(RS_EARG, "empty shape");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> ho;
    if (int r = dbg_ints(seq_off, (size_t)S + 1, ho, s)) return r;
    if (!dbg_offsets(ho, true, M)) return rs_fail(RS_EARG, "offsets must start at 0, ascend and end at M");
    return dbg_done(tr_pos_grad(dx0, seq_off, S, tmax, H, dpos, s), s, "rs_debug_train_pos_grad");
}

// out [S] = tr_cls_fwd of h [M, H] (the CLS row of sequence s is seq_off[s])
extern "C" int rs_debug_train_cls_fwd(const float* h, const int* seq_off, int S, int M, int H, const float* w,
                                      const float* b, float* out, void* stream) {
    if (!h || !seq_off || !w || !b || !out) return rs_fail(RS_EARG, "null argument");
    if (S <= 0 || M <= 0 || H <= 0) return rs_fail(RS_EARG, "empty shape");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> ho;
    if (int r = dbg_ints(seq_off, (size_t)S + 1, ho, s)) return r;
    if (!dbg_offsets(ho, true, M)) return rs_fail(RS_EARG, "offsets must start at 0, ascend and end at M");
    return dbg_done(tr_cls_fwd(h, seq_off, S, H, w, b, out, s), s, "rs_debug_train_cls_fwd");
}

// tr_cls_bwd: dh [M, H] (zeroed by the caller) at the CLS rows, dw [H] and db [1] added to
extern "C" int rs_debug_train_cls_bwd(const float* dsc, const float* h, const int* seq_off, int S, int M, int H,
                                      const float* w, float* dh, float* dw, float* db, void* stream) {
    if (!dsc || !h || !seq_off || !w || !dh || !dw || !db) return rs_fail(RS_EARG, "null argument");
    if (S <= 0 || M <= 0 || H <= 0) return rs_fail(RS_EARG, "empty shape");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> ho;
    if (int r = dbg_ints(seq_off, (size_t)S + 1, ho, s)) return r;
    if (!dbg_offsets(ho, true, M)) return rs_fail(RS_EARG, "offsets must start at 0, ascend and end at M");
    return dbg_done(tr_cls_bwd(dsc, h, seq_off, S, H, w, dh, dw, db, s), s, "rs_debug_train_cls_bwd");
}

// tr_loss: sc, tgt, am, cer, dsc [n_hyp]; utt_off [n_utt + 1] (empty groups allowed); uloss [n_utt];
// loss [1].  kind: RS_LOSS_MD / _MWER / _MWED.
extern "C" int rs_debug_train_loss(const float* sc, const float* tgt, const float* am, const float* cer,
                                   const int* utt_off, int n_utt, int n_hyp, int kind, float md_w, float* dsc,
                                   float* uloss, float* loss, void* stream) {
    if (!sc || !tgt || !am || !cer || !utt_off || !dsc || !uloss || !loss) return rs_fail(RS_EARG, "null argument");
    if (n_utt <= 0 || n_hyp <= 0) return rs_fail(RS_EARG, "empty shape");
    if (kind != RS_LOSS_MD && kind != RS_LOSS_MWER && kind != RS_LOSS_MWED) return rs_fail(RS_EARG, "unknown loss");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> ho;
    if (int r = dbg_ints(utt_off, (size_t)n_utt + 1, ho, s)) return r;
    if (!dbg_offsets(ho, false, n_hyp)) return rs_fail(RS_EARG, "offsets must start at 0, not descend and end at n_hyp");
    return dbg_done(tr_loss(sc, tgt, am, cer, utt_off, n_utt, n_hyp, kind, md_w, dsc, uloss, loss, s), s,
                    "rs_debug_train_loss");
}

// tr_ce: logits [M, V] replaced by d loss / d logits, row_loss [M], loss [1] (their mean)
extern "C" int rs_debug_train_ce(float* logits, const int* labels, int M, int V, float* row_loss, float* loss,
                                 void* stream) {
    if (!logits || !labels || !row_loss || !loss) return rs_fail(RS_EARG, "null argument");
    if (M <= 0 || V <= 0) return rs_fail(RS_EARG, "empty shape");
    hipStream_t s = (hipStream_t)stream;
    return dbg_done(tr_ce(logits, labels, M, V, row_loss, loss, s), s, "rs_debug_train_ce");
}

// op 0: tr_gather_rows, dst [n, H] = src [M, H] at idx [n] (rows in [0, M)); 1: tr_expand_rows,
// dst [M, H] = src [n, H] at idx [M] (in [0, n), or negative: a zero row)
extern "C" int rs_debug_train_move_rows(int op, const float* src, const int* idx, int n, int M, int H, float* dst,
                                        void* stream) {
    if (op < 0 || op > 1) return rs_fail(RS_EARG, "op must be 0 or 1");
    if (!src || !idx || !dst) return rs_fail(RS_EARG, "null argument");
    if (n <= 0 || M <= 0 || H <= 0) return rs_fail(RS_EARG, "empty shape");
    if (H % 4) return rs_fail(RS_EUNSUP, "H must be a multiple of 4");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> hi;
    if (int r = dbg_ints(idx, (size_t)(op == 0 ? n : M), hi, s)) return r;
    if (!dbg_in_range(hi, op == 0 ? 0 : -2147483648LL, op == 0 ? M : n)) return rs_fail(RS_EARG, "row index out of range");
    return dbg_done(op == 0 ? tr_gather_rows(src, idx, n, H, dst, s) : tr_expand_rows(src, idx, M, H, dst, s), s,
                    "rs_debug_train_move_rows");
}

// One torch.optim.AdamW step, number `step` (1-based), on p, g, m, v [n]: the optimizer's own
// hyper-parameters, turned into the kernel's scalars by tr_adamw_scalars as the trainer does
extern "C" int rs_debug_train_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, long long step, void* stream) {
    if (!p || !g || !m || !v) return rs_fail(RS_EARG, "null argument");
    if (n <= 0 || step < 1) return rs_fail(RS_EARG, "n and step must be positive");
    hipStream_t s = (hipStream_t)stream;
    const TrAdamW a = tr_adamw_scalars(lr, beta1, beta2, eps, weight_decay, step);
    return dbg_done(tr_adamw(p, g, m, v, n, a.decay, a.b1w, a.b2, a.b2w, a.step_size, a.bc2_sqrt, a.eps, s), s,
                    "rs_debug_train_adamw");
}

// The same step on the scaled gradient gmul * g (tr_adamw_scaled, what rs_trainer_apply launches)
extern "C" int rs_debug_train_adamw_scaled(float* p, const float* g, float* m, float* v, long long n, float gmul,
                                           float lr, float beta1, float beta2, float eps, float weight_decay,
                                           long long step, void* stream) {
    if (!p || !g || !m || !v) return rs_fail(RS_EARG, "null argument");
    if (n <= 0 || step < 1) return rs_fail(RS_EARG, "n and step must be positive");
    hipStream_t s = (hipStream_t)stream;
    const TrAdamW a = tr_adamw_scalars(lr, beta1, beta2, eps, weight_decay, step);
    return dbg_done(tr_adamw_scaled(p, g, m, v, n, gmul, a.decay, a.b1w, a.b2, a.b2w, a.step_size, a.bc2_sqrt, a.eps, s),
                    s, "rs_debug_train_adamw_scaled");
}

namespace {

// a host range list (offset, count) inside a buffer of n_total floats
int dbg_ranges(const long long* h_off, const long long* h_n, int n_ranges, long long n_total, std::vector<TrRange>& r) {
    if (!h_off || !h_n || n_ranges <= 0) return rs_fail(RS_EARG, "null / empty range list");
    for (int k = 0; k < n_ranges; ++k) {
        if (h_off[k] < 0 || h_n[k] <= 0 || h_off[k] > n_total || h_n[k] > n_total - h_off[k])
            return rs_fail(RS_EARG, "range " + std::to_string(k) + " outside the buffer");
        r.push_back({h_off[k], h_n[k]});
    }
    return RS_OK;
}

}  // namespace

// acc[i] = fmaf(w, g[i], acc[i]) over the listed ranges of acc, g [n_total] (tr_accum per range, as
// rs_trainer_accumulate runs it); everything outside the ranges is left alone
extern "C" int rs_debug_train_accum(float* acc, const float* g, const long long* h_off, const long long* h_n,
                                    int n_ranges, long long n_total, float w, void* stream) {
    if (!acc || !g) return rs_fail(RS_EARG, "null argument");
    std::vector<TrRange> r;
    if (int e = dbg_ranges(h_off, h_n, n_ranges, n_total, r)) return e;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    for (const TrRange& x : r)
        if (e == hipSuccess) e = tr_accum(acc + x.off, g + x.off, x.n, w, s);
    return dbg_done(e, s, "rs_debug_train_accum");
}

// h_out[0] = float64 sum of squares of g [n_total] over the listed ranges (tr_sumsq; its square root
// is the norm rs_trainer_grad_norm returns)
extern "C" int rs_debug_train_sumsq(const float* g, const long long* h_off, const long long* h_n, int n_ranges,
                                    long long n_total, double* h_out, void* stream) {
    if (!g || !h_out) return rs_fail(RS_EARG, "null argument");
    std::vector<TrRange> r;
    if (int e = dbg_ranges(h_off, h_n, n_ranges, n_total, r)) return e;
    hipStream_t s = (hipStream_t)stream;
    double* ws = nullptr;
    if (hipMalloc((void**)&ws, tr_sumsq_ws_doubles(n_ranges) * 8) != hipSuccess) {
        (void)hipGetLastError();
        return rs_fail(RS_ENOMEM, "rs_debug_train_sumsq: scratch");
    }
    hipError_t e = tr_sumsq(g, r.data(), n_ranges, ws, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h_out, ws, 8, hipMemcpyDeviceToHost, s);
    const int rc = dbg_done(e, s, "rs_debug_train_sumsq");
    (void)hipFree(ws);
    return rc;
}
