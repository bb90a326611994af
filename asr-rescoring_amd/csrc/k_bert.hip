// BERT encoder kernels other than the GEMMs and attention (k_attn.hip) (gfx950, wave64).
//
//  embed_ln        K1+K2: on-device [MASK] expansion (MLM_PLL/preprocess.py:15-21) fused with
//                  BertEmbeddings (modeling_bert.py:53-108): word + type[segment id, 0 without] + position -> LN
//  embed_ln_set    the same for multi-mask rows: [MASK] at every position of the row's query list
//  ln_rows         LayerNorm of BertSelfOutput / BertOutput / head transform (eps 1e-12)
//  lse_finalize    merges the decoder epilogue's (max, sum exp) slabs: log_softmax gather
//                  (MLM_PLL/main.py:101-105)
//  topk_merge      merges the decoder epilogue's per-slab (logit, column) candidates into a row's
//                  k best tokens and their log-probs (the same row before the label gather)
//  cand_finalize   the candidate form's merge: the log-prob of every column of a row's candidate list
//                  (the same row, the label gather at a caller-chosen set of columns)
//  cls_linear      RescoreBert Linear(H, 1) on the CLS state (RescoreBert/model.py:19-20)
//  segsum_f64      per-hypothesis PLL, float64, in row order (MLM_PLL/main.py:106-107)
//
// Every producer of a GEMM operand writes the fp16 operand image (put_split: [hi],
// [hi | hi/64 | lo*64], or the split-operand form's per-K-step interleaved [hi 32 | lo 32]).  The residual stream stays PRE-LayerNorm in fp32 (x32) with per-row
// (mean, rstd): its consumers (the next residual GEMM's accumulator init, attention_query)
// rebuild LN(x) with ln_apply, so no LN kernel writes an fp32 copy of its output.
#include <type_traits>
#include "common.h"
#include "seq_plan.h"

namespace {

// LayerNorm of one row held as NV float4 per lane (row = 256*NV floats over one wave).
// Writes the row statistics (stats != null), LN(x) in fp32 (y32 != null) and the fp16
// operand image; every output element goes through ln_apply (common.h).
template <int NV>
__device__ __forceinline__ void ln_store(const float4 (&x)[NV], const float* g, const float* b, float eps,
                                         int lane, float* y32, float2* stats, f16* y16, int kx) {
    constexpr int H = NV * 256;
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) s += (x[v].x + x[v].y) + (x[v].z + x[v].w);
    const float mean = __fmul_rn(wave_sum(s), 1.0f / H);
    float q = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const float4 d = make_float4(x[v].x - mean, x[v].y - mean, x[v].z - mean, x[v].w - mean);
        q += __builtin_fmaf(d.x, d.x, __fmul_rn(d.y, d.y)) + __builtin_fmaf(d.z, d.z, __fmul_rn(d.w, d.w));
    }
    const float2 st = make_float2(mean, 1.0f / sqrtf(__builtin_fmaf(wave_sum(q), 1.0f / H, eps)));
    if (stats && lane == 0) *stats = st;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        const float4 gg = *(const float4*)(g + c);
        const float4 bb = *(const float4*)(b + c);
        float4 y;
        y.x = ln_apply(x[v].x, st, gg.x, bb.x);
        y.y = ln_apply(x[v].y, st, gg.y, bb.y);
        y.z = ln_apply(x[v].z, st, gg.z, bb.z);
        y.w = ln_apply(x[v].w, st, gg.w, bb.w);
        if (y32) *(float4*)(y32 + c) = y;
        if (y16) put_split4(y16, c, H, kx, y);
    }
}

// Embedding sum of position t of a sequence (token t, or [MASK] when lo <= t < hi): the one
// expression both the copy-row and the unique-row kernels use (bit-identical rows).
// type (nullable): segment ids parallel to tok; a [MASK] row keeps the type of its position.
// typetab: the whole [type_vocab, H] table; without segment ids every row adds its row 0.
template <int NV>
__device__ __forceinline__ void embed_row(const int* tok, const int* type, int toff, int t, int lo, int hi,
                                          int mask_id, int vocab, int type_vocab, const float* word, const float* pos,
                                          const float* typetab, int lane, float4 (&x)[NV]) {
    constexpr int H = NV * 256;
    int id = (t >= lo && t < hi) ? mask_id : tok[toff + t];
    id = min(max(id, 0), vocab - 1);              // out-of-range ids are clamped, never read OOB
    const float* type0 = typetab + (type ? (size_t)min(max(type[toff + t], 0), type_vocab - 1) * H : (size_t)0);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        const float4 w = *(const float4*)(word + (size_t)id * H + c);
        const float4 ty = *(const float4*)(type0 + c);
        const float4 p = *(const float4*)(pos + (size_t)t * H + c);
        // transformers order: (inputs_embeds + token_type) + position
        x[v] = make_float4((w.x + ty.x) + p.x, (w.y + ty.y) + p.y, (w.z + ty.z) + p.z, (w.w + ty.w) + p.w);
    }
}

// Layer-0 dedup: the unique rows of the chunk's plan (seq_plan.h plan_unique_rows), each written
// by exactly one block (unique_rows_owned): the first copy of a run writes the hypothesis' T
// unmasked rows, the last copy the run's [MASK] rows.  s1 - s0 blocks; urows: the chunk's count.
template <int NV>
__global__ void __launch_bounds__(256)
embed_unique_kernel(const int* __restrict__ tok, const int* __restrict__ type, SeqMeta sm, int s0, int urows,
                    int mask_id, int vocab, int type_vocab, const float* __restrict__ word,
                    const float* __restrict__ pos, const float* __restrict__ typetab, const float* __restrict__ g,
                    const float* __restrict__ b, float eps, f16* __restrict__ h16u, int kx) {
    constexpr int H = NV * 256;
    const int s = s0 + blockIdx.x;
    const int T = sm.len[s], toff = sm.tok_off[s], uh = sm.urow_h[s];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool first = blockIdx.x == 0, last = blockIdx.x == gridDim.x - 1;
    const UniqueOwn w = unique_rows_owned(first, last, first ? 0 : sm.urow_h[s - 1], uh, last ? 0 : sm.urow_h[s + 1],
                                          sm.urow_m[s], T, sm.mask_pos[s], urows);
    for (int k = wave; k < w.n_orig + w.n_mask; k += 4) {
        const bool masked = k >= w.n_orig;
        const int j = k - w.n_orig;
        const int t = masked ? w.mask_pos + j : k;
        const size_t r = masked ? (size_t)(w.mask_row + j) : (size_t)(uh + k);
        float4 x[NV];
        embed_row<NV>(tok, type, toff, t, masked ? t : -1, masked ? t + 1 : -1, mask_id, vocab, type_vocab, word, pos,
                      typetab, lane, x);
        ln_store<NV>(x, g, b, eps, lane, nullptr, nullptr, h16u + r * kx * H, kx);
    }
}

template <int NV>
__global__ void __launch_bounds__(256)
embed_ln_kernel(const int* __restrict__ tok, const int* __restrict__ type, SeqMeta sm, int s0, int row0, int mask_id,
                int vocab, int type_vocab, const float* __restrict__ word, const float* __restrict__ pos,
                const float* __restrict__ typetab, const float* __restrict__ g,
                const float* __restrict__ b, float eps, float* __restrict__ x32,
                float2* __restrict__ stats, f16* __restrict__ h16, int kx) {
    constexpr int H = NV * 256;
    const int s = s0 + blockIdx.x;
    const int T = sm.len[s], toff = sm.tok_off[s], lo = sm.mask_pos[s], hi = sm.mask_end[s];
    const int rs = sm.row[s] - row0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < T; t += 4) {
        float4 x[NV];
        embed_row<NV>(tok, type, toff, t, lo, hi, mask_id, vocab, type_vocab, word, pos, typetab, lane, x);
        const size_t r = (size_t)(rs + t);
#pragma unroll
        for (int v = 0; v < NV; ++v) if (x32) *(float4*)(x32 + r * H + v * 256 + lane * 4) = x[v];
        ln_store<NV>(x, g, b, eps, lane, nullptr, stats ? stats + r : nullptr, h16 ? h16 + r * kx * H : nullptr, kx);
    }
}

// embed_ln for multi-mask rows: position t is [MASK] when it is one of the sequence's query
// positions (qm.pos[qm.first[s] .. qm.first[s + 1]), strictly ascending: binary search).  The row
// goes through embed_row / ln_store as in embed_ln_kernel, so a row masked at one position has the
// bits that kernel gives it.
template <int NV>
__global__ void __launch_bounds__(256)
embed_ln_set_kernel(const int* __restrict__ tok, const int* __restrict__ type, SeqMeta sm, QueryMeta qm, int s0,
                    int mask_id, int vocab, int type_vocab, const float* __restrict__ word,
                    const float* __restrict__ pos, const float* __restrict__ typetab, const float* __restrict__ g,
                    const float* __restrict__ b, float eps, float* __restrict__ x32, float2* __restrict__ stats,
                    f16* __restrict__ h16, int kx) {
    constexpr int H = NV * 256;
    const int s = s0 + blockIdx.x;
    const int T = sm.len[s], toff = sm.tok_off[s], rs = sm.row[s];
    const int qa = qm.first[s], qb = qm.first[s + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < T; t += 4) {
        int lo = qa, hi = qb;                      // first query position >= t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (qm.pos[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        const bool masked = lo < qb && qm.pos[lo] == t;
        float4 x[NV];
        embed_row<NV>(tok, type, toff, t, masked ? t : -1, masked ? t + 1 : -1, mask_id, vocab, type_vocab, word, pos,
                      typetab, lane, x);
        const size_t r = (size_t)(rs + t);
#pragma unroll
        for (int v = 0; v < NV; ++v) if (x32) *(float4*)(x32 + r * H + v * 256 + lane * 4) = x[v];
        ln_store<NV>(x, g, b, eps, lane, nullptr, stats ? stats + r : nullptr, h16 ? h16 + r * kx * H : nullptr, kx);
    }
}

template <int NV>
__global__ void __launch_bounds__(256)
ln_rows_kernel(const float* __restrict__ xin, int rows, const float* __restrict__ g,
               const float* __restrict__ b, float eps, float* __restrict__ y32,
               float2* __restrict__ stats, f16* __restrict__ y16, int kx) {
    constexpr int H = NV * 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float4 x[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) x[v] = *(const float4*)(xin + (size_t)row * H + v * 256 + lane * 4);
    ln_store<NV>(x, g, b, eps, lane, y32 ? y32 + (size_t)row * H : nullptr, stats ? stats + row : nullptr,
                 y16 + (size_t)row * kx * H, kx);
}

// BertSelfOutput (modeling_bert.py:282-293) with the O projection done by the persistent
// fp16-output GEMM (o16 = ctx . Wo^T + bo): the residual add and the LayerNorm happen here,
// so the GEMM neither reads nor writes the fp32 stream.  x32 <- LN_prev(x32) + o16 (LN_prev
// rebuilt from the row statistics in `stats` and (pg, pb)), then its statistics and the fp16
// operand image of LN(x32) with (g, b).  fp16 precision mode (kx == 1) only.
template <int NV, bool WX, bool TWO>
__global__ void __launch_bounds__(256)
ln_res_rows_kernel(float* __restrict__ x32, const float2* stats, float2* stats_out, const float* __restrict__ pg,
                   const float* __restrict__ pb, const f16* __restrict__ o16, int rows,
                   const float* __restrict__ g, const float* __restrict__ b, float eps,
                   f16* __restrict__ y16, const float2* __restrict__ stats1, const float* __restrict__ g1,
                   const float* __restrict__ b1, const f16* __restrict__ o16b) {
    constexpr int H = NV * 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float2 st0 = stats[row];
    float2 st1 = make_float2(0.f, 0.f);
    if constexpr (TWO) st1 = stats1[row];
    float4 x[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        const float4 r = *(const float4*)(x32 + (size_t)row * H + c);
        const float4 gg = *(const float4*)(pg + c);
        const float4 bb = *(const float4*)(pb + c);
        const half4 o = *(const half4*)(o16 + (size_t)row * H + c);
        x[v] = make_float4(ln_apply(r.x, st0, gg.x, bb.x) + (float)o[0], ln_apply(r.y, st0, gg.y, bb.y) + (float)o[1],
                           ln_apply(r.z, st0, gg.z, bb.z) + (float)o[2], ln_apply(r.w, st0, gg.w, bb.w) + (float)o[3]);
        if constexpr (TWO) {
            // second residual block: x <- LN1(x; st1, g1, b1) + o16b (BertOutput after a deferred
            // BertSelfOutput: x is the post-attention stream the first pass did not store)
            const float4 g4 = *(const float4*)(g1 + c);
            const float4 b4 = *(const float4*)(b1 + c);
            const half4 ob = *(const half4*)(o16b + (size_t)row * H + c);
            x[v] = make_float4(ln_apply(x[v].x, st1, g4.x, b4.x) + (float)ob[0], ln_apply(x[v].y, st1, g4.y, b4.y) + (float)ob[1],
                               ln_apply(x[v].z, st1, g4.z, b4.z) + (float)ob[2], ln_apply(x[v].w, st1, g4.w, b4.w) + (float)ob[3]);
        }
        if constexpr (WX) *(float4*)(x32 + (size_t)row * H + c) = x[v];
    }
    ln_store<NV>(x, g, b, eps, lane, nullptr, stats_out + row, y16 + (size_t)row * H, 1);
}

// BertSelfOutput / BertOutput (modeling_bert.py:282-293, 340-351) in the fp16x3 split-operand
// mode: the projection (x3s GEMM) wrote o32 = dense(h) + bias in fp32; here x = LN_prev(x32) +
// o32 (the residual input rebuilt from the pre-LN stream and its statistics, the reference's
// hidden_states + input_tensor order), x written back as the new pre-LN stream, its statistics,
// and the kx-wide operand image of LN(x) for the next projection.
template <int NV>
__global__ void __launch_bounds__(256)
ln_res32_kernel(float* __restrict__ x32, const float2* stats, float2* stats_out, const float* __restrict__ pg,
                const float* __restrict__ pb, const float* __restrict__ o32, int rows, const float* __restrict__ g,
                const float* __restrict__ b, float eps, f16* __restrict__ y16, int kx) {
    constexpr int H = NV * 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float2 st0 = stats[row];
    float4 x[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        const float4 r = *(const float4*)(x32 + (size_t)row * H + c);
        const float4 gg = *(const float4*)(pg + c);
        const float4 bb = *(const float4*)(pb + c);
        const float4 o = *(const float4*)(o32 + (size_t)row * H + c);
        x[v] = make_float4(o.x + ln_apply(r.x, st0, gg.x, bb.x), o.y + ln_apply(r.y, st0, gg.y, bb.y),
                           o.z + ln_apply(r.z, st0, gg.z, bb.z), o.w + ln_apply(r.w, st0, gg.w, bb.w));
        *(float4*)(x32 + (size_t)row * H + c) = x[v];
    }
    ln_store<NV>(x, g, b, eps, lane, nullptr, stats_out + row, y16 + (size_t)row * kx * H, kx);
}

// Residual + LayerNorm of a split-operand layer with the residual stream held ONLY as the
// two-part operand image of the normalised hidden state (h = hi + lo/64, ~22 bits):
//   h16 <- image(LN(o32 + h)), in place (one wave per row reads the whole row first).
// 12 B per element (o32, the image in, the image out) instead of ln_res32's 16 (no fp32
// pre-LN stream, no statistics): the next block's residual is the image itself.
template <int NV>
__global__ void __launch_bounds__(256)
ln_res_img_kernel(f16* __restrict__ h16, const float* __restrict__ o32, int rows, const float* __restrict__ g,
                  const float* __restrict__ b, float eps) {
    constexpr int H = NV * 256;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    f16* hr = h16 + (size_t)row * 2 * H;
    float4 x[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int c = v * 256 + lane * 4;
        const float4 h = il_load4(hr, c);
        const float4 o = *(const float4*)(o32 + (size_t)row * H + c);
        x[v] = make_float4(o.x + h.x, o.y + h.y, o.z + h.z, o.w + h.w);
    }
    ln_store<NV>(x, g, b, eps, lane, nullptr, nullptr, hr, 2);
}

// BERTScore embeddings (bert_score bert_encode + greedy_cos_idf's row normalisation):
// e = LN(x) of the last layer, rebuilt from the pre-LN stream, then e / ||e||_2 in fp32,
// stored at the token's position in the caller's ragged token layout: fp16 [H] (TWO false),
// or the two-part image [hi | lo*64] of 2H halves (TWO, the fp16x3 mode: e = hi + lo/64,
// ~22 significant bits, which the split-operand recall kernel multiplies as three products).
template <int NV, bool TWO>
__global__ void __launch_bounds__(256)
embed_out_kernel(const float* __restrict__ x32, const float2* __restrict__ stats,
                 const float* __restrict__ g, const float* __restrict__ b, SeqMeta sm, int s0,
                 int row0, f16* __restrict__ out, const f16* __restrict__ himg) {
    constexpr int H = NV * 256;
    const int s = s0 + blockIdx.x;
    const int T = sm.len[s], rs = sm.row[s] - row0, toff = sm.tok_off[s];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < T; t += 4) {
        const size_t r = (size_t)(rs + t);
        float4 y[NV];
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = v * 256 + lane * 4;
            if (himg) {                       // the normalised state's (interleaved) two-part image
                y[v] = il_load4(himg + r * 2 * H, c);
            } else {
                const float2 st = stats[r];
                const float4 x = *(const float4*)(x32 + r * H + c);
                const float4 gg = *(const float4*)(g + c), bb = *(const float4*)(b + c);
                y[v] = make_float4(ln_apply(x.x, st, gg.x, bb.x), ln_apply(x.y, st, gg.y, bb.y),
                                   ln_apply(x.z, st, gg.z, bb.z), ln_apply(x.w, st, gg.w, bb.w));
            }
            q += y[v].x * y[v].x + y[v].y * y[v].y + y[v].z * y[v].z + y[v].w * y[v].w;
        }
        const float nrm = sqrtf(wave_sum(q));
        f16* o = out + (size_t)(toff + t) * H * (TWO ? 2 : 1);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int c = v * 256 + lane * 4;
            const float4 e = make_float4(y[v].x / nrm, y[v].y / nrm, y[v].z / nrm, y[v].w / nrm);
            if constexpr (TWO) {              // the caller's planar [hi | lo*64] layout (rs_token_embed)
                const half4 hi = {(f16)e.x, (f16)e.y, (f16)e.z, (f16)e.w};
                *(half4*)(o + c) = hi;
                *(half4*)(o + H + c) = half4{x3_lo(e.x, hi[0]), x3_lo(e.y, hi[1]), x3_lo(e.z, hi[2]), x3_lo(e.w, hi[3])};
            } else *(half4*)(o + c) = half4{(f16)e.x, (f16)e.y, (f16)e.z, (f16)e.w};
        }
    }
}

// Row gather: dst[s - s0] = src[row of sequence s's scored position] (ld halfs per row).
__global__ void __launch_bounds__(64)
gather_query_rows_kernel(const f16* __restrict__ src, int ld, SeqMeta sm, int s0, int row0,
                         f16* __restrict__ dst) {
    const int s = s0 + blockIdx.x;
    const size_t r = (size_t)(sm.row[s] - row0 + sm.query[s]);
    const uint4* a = (const uint4*)(src + r * ld);
    uint4* o = (uint4*)(dst + (size_t)blockIdx.x * ld);
    for (int i = threadIdx.x; i < ld / 8; i += 64) o[i] = a[i];
}

// The label may be any int (a caller's label, or a raw token id: the embedding clamps ids, the
// label is not clamped): the decoder epilogue only compares it with column indices, so one outside
// [0, vocab) matches no column and the row keeps the -inf written here.
__global__ void gather_labels_kernel(const int* __restrict__ tok, SeqMeta sm, int s0, int n,
                                     int* __restrict__ lab, float* __restrict__ label_logit) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = s0 + i;
    const int l = sm.label[s];
    lab[i] = (l == -1 && tok) ? tok[sm.tok_off[s] + sm.query[s]] : l;
    label_logit[i] = -INFINITY;
}

// The two gathers over a query list: block / thread i serves query q0 + i, whose row is
// (sequence qm.seq, position qm.pos).
__global__ void __launch_bounds__(64)
gather_query_rows_list_kernel(const f16* __restrict__ src, int ld, SeqMeta sm, QueryMeta qm, int q0,
                              f16* __restrict__ dst) {
    const int q = q0 + blockIdx.x;
    const size_t r = (size_t)(sm.row[qm.seq[q]] + qm.pos[q]);
    const uint4* a = (const uint4*)(src + r * ld);
    uint4* o = (uint4*)(dst + (size_t)blockIdx.x * ld);
    for (int i = threadIdx.x; i < ld / 8; i += 64) o[i] = a[i];
}
__global__ void gather_labels_list_kernel(const int* __restrict__ tok, SeqMeta sm, QueryMeta qm, int q0, int n,
                                          int* __restrict__ lab, float* __restrict__ label_logit) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int q = q0 + i;
    const int l = qm.label[q];
    lab[i] = (l == -1 && tok) ? tok[sm.tok_off[qm.seq[q]] + qm.pos[q]] : l;
    label_logit[i] = -INFINITY;
}

__global__ void __launch_bounds__(256)
lse_finalize_kernel(const float2* __restrict__ part, int n_parts, const float* __restrict__ ll,
                    int rows, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float2* p = part + (size_t)row * n_parts;
    float mx = -INFINITY;
    for (int k = lane; k < n_parts; k += 64)
        if (p[k].y > 0.f) mx = fmaxf(mx, p[k].x);
    mx = wave_max(mx);
    float sm = 0.f;
    for (int k = lane; k < n_parts; k += 64)
        if (p[k].y > 0.f) sm += p[k].y * __expf(p[k].x - mx);
    sm = wave_sum(sm);
    if (lane == 0) out[row] = ll[row] - (mx + logf(sm));
}

// The candidate form's finalise (EPI_LSE_CAND): out[perm[t]] = cand_logit[t] - logsumexp(row) for the
// entries t of the row's list [c_off[row], c_off[row + 1]).  One wave per row; mx and sm are
// lse_finalize_kernel's loops and the subtraction its expression, statement for statement, so a
// candidate's log-prob equals that kernel's output for the same column as label, bit for bit.  A
// row with an empty list writes nothing.
__global__ void __launch_bounds__(256)
cand_finalize_kernel(const float2* __restrict__ part, int n_parts, const float* __restrict__ cl,
                     const int* __restrict__ c_off, const int* __restrict__ perm, int rows, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int t0 = c_off[row], t1 = c_off[row + 1];
    if (t0 >= t1) return;
    const float2* p = part + (size_t)row * n_parts;
    float mx = -INFINITY;
    for (int k = lane; k < n_parts; k += 64)
        if (p[k].y > 0.f) mx = fmaxf(mx, p[k].x);
    mx = wave_max(mx);
    float sm = 0.f;
    for (int k = lane; k < n_parts; k += 64)
        if (p[k].y > 0.f) sm += p[k].y * __expf(p[k].x - mx);
    sm = wave_sum(sm);
    for (int t = t0 + lane; t < t1; t += 64) out[perm[t]] = cl[t] - (mx + logf(sm));
}

__global__ void fill_f32_kernel(float* __restrict__ p, size_t n, float v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// Merges a row's n_parts x k slab candidates (EPI_LSE_TOPK: (logit, column bits), unused slots
// (-inf, INT_MAX)) into its k best, in the epilogue's total order — larger logit first, the lower
// column among equal logits — so the result does not depend on the slab a column fell in.  One wave
// per row.  The columns are distinct, so the order is strict and round t takes the best candidate
// that comes after round t-1's winner: nothing is marked, the candidates are only read.  An unused
// slot is never better than the start value (-inf, INT_MAX), so it is never returned; a row with
// fewer than k finite logits gets id -1 / log-prob -inf there (the call's range guard reports it).
// mx and sm are lse_finalize_kernel's loops, statement for statement: top_lp of a label equals that
// kernel's output for it bit for bit.
__global__ void __launch_bounds__(256)
topk_merge_kernel(const float2* __restrict__ part, int n_parts, const float2* __restrict__ cand, int k, int rows,
                  int* __restrict__ top_id, float* __restrict__ top_lp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float2* p = part + (size_t)row * n_parts;
    float mx = -INFINITY;
    for (int q = lane; q < n_parts; q += 64)
        if (p[q].y > 0.f) mx = fmaxf(mx, p[q].x);
    mx = wave_max(mx);
    float sm = 0.f;
    for (int q = lane; q < n_parts; q += 64)
        if (p[q].y > 0.f) sm += p[q].y * __expf(p[q].x - mx);
    sm = wave_sum(sm);
    const float lse = mx + logf(sm);
    const float2* c = cand + (size_t)row * n_parts * k;
    const int n = n_parts * k;
    float pv = INFINITY;                       // the previous round's winner
    int pc = -1;
    for (int t = 0; t < k; ++t) {
        float bv = -INFINITY;
        int bc = 0x7fffffff;
        for (int i = lane; i < n; i += 64) {
            const float2 e = c[i];
            const float x = e.x;
            const int col = __float_as_int(e.y);
            const bool after = x < pv || (x == pv && col > pc);
            const bool better = x > bv || (x == bv && col < bc);
            if (after && better) {
                bv = x;
                bc = col;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oc = __shfl_xor(bc, o);
            if (ov > bv || (ov == bv && oc < bc)) {
                bv = ov;
                bc = oc;
            }
        }
        if (lane == 0) {
            top_id[(size_t)row * k + t] = bv == -INFINITY ? -1 : bc;
            top_lp[(size_t)row * k + t] = bv - lse;
        }
        pv = bv;
        pc = bc;
    }
}

__global__ void __launch_bounds__(256)
cls_linear_kernel(const float* __restrict__ h, int rows, int H, const float* __restrict__ w,
                  const float* __restrict__ b, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float d = 0.f;
    for (int c = lane; c < H; c += 64) d += h[(size_t)row * H + c] * w[c];
    d = wave_sum(d);
    if (lane == 0) out[row] = d + b[0];
}

__global__ void segsum_f64_kernel(const float* __restrict__ row_lp, const int* __restrict__ off,
                                  int n, double* __restrict__ out) {
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n) return;
    double acc = 0.0;
    for (int i = off[h]; i < off[h + 1]; ++i) acc += (double)row_lp[i];
    out[h] = acc;
}

// memory skeleton of the two-block ln_res_rows pass: the same loads and stores per row
// (x32 fp32, two fp16 rows, stats; x32 + fp16 image written), no arithmetic beyond a sum
__global__ void __launch_bounds__(256)
lnres_memskel_kernel(float* __restrict__ x32, const f16* __restrict__ o1, const f16* __restrict__ o2, int rows,
                     f16* __restrict__ y16) {
    constexpr int H = 768;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const int c = v * 256 + lane * 4;
        float4 r = *(const float4*)(x32 + (size_t)row * H + c);
        const half4 a = *(const half4*)(o1 + (size_t)row * H + c);
        const half4 b = *(const half4*)(o2 + (size_t)row * H + c);
        r = make_float4(r.x + (float)a[0] + (float)b[0], r.y + (float)a[1] + (float)b[1], r.z + (float)a[2] + (float)b[2],
                        r.w + (float)a[3] + (float)b[3]);
        *(float4*)(x32 + (size_t)row * H + c) = r;
        *(half4*)(y16 + (size_t)row * H + c) = half4{(f16)r.x, (f16)r.y, (f16)r.z, (f16)r.w};
    }
}

// The row kernels hold a row of H = 256 NV floats as NV float4 per lane: runs
// launch(std::integral_constant<int, NV>) for H in {256, 512, 768, 1024} and returns the launch's
// error, hipErrorInvalidValue for any other H.
template <class Launch>
hipError_t launch_for_h(int H, Launch&& launch) {
    switch (H) {
        case 256: launch(std::integral_constant<int, 1>{}); break;
        case 512: launch(std::integral_constant<int, 2>{}); break;
        case 768: launch(std::integral_constant<int, 3>{}); break;
        case 1024: launch(std::integral_constant<int, 4>{}); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_embed_ln(const int* tok, const int* type, SeqMeta sm, int s0, int s1, int row0, int mask_id,
                           int vocab, int type_vocab, const float* word, const float* pos, const float* typetab,
                           const float* g, const float* b, float eps, int H, float* x32,
                           float2* stats, f16* h16, int kx, hipStream_t st) {
    const int n = s1 - s0;
    if (n <= 0) return hipSuccess;
    return launch_for_h(H, [&](auto nv) {
        hipLaunchKernelGGL(embed_ln_kernel<decltype(nv)::value>, dim3(n), dim3(256), 0, st, tok, type, sm, s0, row0,
                           mask_id, vocab, type_vocab, word, pos, typetab, g, b, eps, x32, stats, h16, kx);
    });
}

hipError_t launch_embed_unique(const int* tok, const int* type, SeqMeta sm, int s0, int s1, int urows, int mask_id,
                               int vocab, int type_vocab, const float* word, const float* pos, const float* typetab,
                               const float* g, const float* b, float eps, int H, f16* h16u, int kx, hipStream_t st) {
    const int n = s1 - s0;
    if (n <= 0) return hipSuccess;
    return launch_for_h(H, [&](auto nv) {
        hipLaunchKernelGGL(embed_unique_kernel<decltype(nv)::value>, dim3(n), dim3(256), 0, st, tok, type, sm, s0, urows,
                           mask_id, vocab, type_vocab, word, pos, typetab, g, b, eps, h16u, kx);
    });
}

hipError_t launch_embed_out(const float* x32, const float2* stats, const float* g, const float* b,
                            SeqMeta sm, int s0, int s1, int row0, int H, f16* out, hipStream_t st, const f16* himg,
                            bool two) {
    const int n = s1 - s0;
    if (n <= 0) return hipSuccess;
    return launch_for_h(H, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        auto* k = two ? embed_out_kernel<NV, true> : embed_out_kernel<NV, false>;
        hipLaunchKernelGGL(k, dim3(n), dim3(256), 0, st, x32, stats, g, b, sm, s0, row0, out, himg);
    });
}

hipError_t launch_ln_rows(const float* x, int rows, const float* g, const float* b, float eps,
                          int H, float* y32, float2* stats, f16* y16, int kx, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    const dim3 grid((rows + 3) / 4);
    return launch_for_h(H, [&](auto nv) {
        hipLaunchKernelGGL(ln_rows_kernel<decltype(nv)::value>, grid, dim3(256), 0, st, x, rows, g, b, eps, y32, stats,
                           y16, kx);
    });
}

hipError_t launch_ln_res32(float* x32, const float2* stats, float2* stats_out, const float* pg, const float* pb,
                           const float* o32, int rows, const float* g, const float* b, float eps, int H, f16* y16,
                           int kx, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    const dim3 grid((rows + 3) / 4), block(256);
    return launch_for_h(H, [&](auto nv) {
        hipLaunchKernelGGL(ln_res32_kernel<decltype(nv)::value>, grid, block, 0, st, x32, stats, stats_out, pg, pb, o32,
                           rows, g, b, eps, y16, kx);
    });
}

hipError_t launch_ln_res_img(f16* h16, const float* o32, int rows, const float* g, const float* b, float eps, int H,
                             hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    const dim3 grid((rows + 3) / 4), block(256);
    return launch_for_h(H, [&](auto nv) {
        hipLaunchKernelGGL(ln_res_img_kernel<decltype(nv)::value>, grid, block, 0, st, h16, o32, rows, g, b, eps);
    });
}

hipError_t launch_ln_res_rows(float* x32, const float2* stats, float2* stats_out, const float* pg, const float* pb,
                             const f16* o16, int rows, const float* g, const float* b, float eps, int H,
                             f16* y16, bool write_x, hipStream_t st, const float2* stats1, const float* g1,
                             const float* b1, const f16* o16b) {
    if (rows <= 0) return hipSuccess;
    const dim3 grid((rows + 3) / 4), block(256);
    const bool two = o16b != nullptr;
    if (two && !write_x) return hipErrorInvalidValue;
    return launch_for_h(H, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        auto* k = two ? ln_res_rows_kernel<NV, true, true>
                  : write_x ? ln_res_rows_kernel<NV, true, false> : ln_res_rows_kernel<NV, false, false>;
        hipLaunchKernelGGL(k, grid, block, 0, st, x32, stats, stats_out, pg, pb, o16, rows, g, b, eps, y16, stats1, g1,
                           b1, o16b);
    });
}

hipError_t launch_gather_query_rows(const f16* src, int ld, SeqMeta sm, int s0, int s1, int row0, f16* dst,
                                   hipStream_t st) {
    if (s1 <= s0) return hipSuccess;
    if (ld % 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_query_rows_kernel, dim3(s1 - s0), dim3(64), 0, st, src, ld, sm, s0, row0, dst);
    return hipGetLastError();
}

hipError_t launch_gather_labels(const int* tok, SeqMeta sm, int s0, int s1, int* lab, float* label_logit,
                                hipStream_t st) {
    const int n = s1 - s0;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_labels_kernel, dim3((n + 255) / 256), dim3(256), 0, st, tok, sm, s0, n, lab, label_logit);
    return hipGetLastError();
}

hipError_t launch_embed_ln_set(const int* tok, const int* type, SeqMeta sm, QueryMeta qm, int s0, int s1, int mask_id,
                               int vocab, int type_vocab, const float* word, const float* pos, const float* typetab,
                               const float* g, const float* b, float eps, int H, float* x32, float2* stats, f16* h16,
                               int kx, hipStream_t st) {
    const int n = s1 - s0;
    if (n <= 0) return hipSuccess;
    return launch_for_h(H, [&](auto nv) {
        hipLaunchKernelGGL(embed_ln_set_kernel<decltype(nv)::value>, dim3(n), dim3(256), 0, st, tok, type, sm, qm, s0,
                           mask_id, vocab, type_vocab, word, pos, typetab, g, b, eps, x32, stats, h16, kx);
    });
}

hipError_t launch_gather_query_rows_list(const f16* src, int ld, SeqMeta sm, QueryMeta qm, int q0, int n, f16* dst,
                                        hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (ld % 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_query_rows_list_kernel, dim3(n), dim3(64), 0, st, src, ld, sm, qm, q0, dst);
    return hipGetLastError();
}

hipError_t launch_gather_labels_list(const int* tok, SeqMeta sm, QueryMeta qm, int q0, int n, int* lab,
                                     float* label_logit, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_labels_list_kernel, dim3((n + 255) / 256), dim3(256), 0, st, tok, sm, qm, q0, n, lab,
                       label_logit);
    return hipGetLastError();
}

hipError_t launch_lse_finalize(const float2* part, int n_parts, const float* label_logit, int rows,
                               float* out, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(lse_finalize_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, part, n_parts, label_logit, rows, out);
    return hipGetLastError();
}

hipError_t launch_fill_f32(float* p, size_t n, float v, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n, v);
    return hipGetLastError();
}

hipError_t launch_cand_finalize(const float2* part, int n_parts, const float* cand_logit, const int* c_off,
                                const int* perm, int rows, float* out, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(cand_finalize_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, part, n_parts, cand_logit, c_off,
                       perm, rows, out);
    return hipGetLastError();
}

hipError_t launch_topk_merge(const float2* part, int n_parts, const float2* cand, int k, int rows, int* top_id,
                             float* top_lp, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    if (k < 1 || k > TOPK_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(topk_merge_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, part, n_parts, cand, k, rows, top_id,
                       top_lp);
    return hipGetLastError();
}

hipError_t launch_cls_linear(const float* h, int rows, int H, const float* w, const float* b,
                             float* out, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(cls_linear_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, h, rows, H, w, b, out);
    return hipGetLastError();
}

hipError_t launch_segsum_f64(const float* row_lp, const int* hyp_seq_off, int n_hyp, double* out,
                             hipStream_t st) {
    if (n_hyp <= 0) return hipSuccess;
    hipLaunchKernelGGL(segsum_f64_kernel, dim3((n_hyp + 255) / 256), dim3(256), 0, st, row_lp, hyp_seq_off, n_hyp, out);
    return hipGetLastError();
}

// Test entry (not part of the scoring path): the MLM decoder as rs_api.hip's head_mlm runs it
// (launch_mlm_decoder: labels and label-logit preset, EPI_LSE GEMM, lse_finalize) with device labels
// given as they are (any int: one outside [0, vocab) yields -inf).  A [M_pad, K], W [vpad, K] fp16,
// bias [vpad], label [m_valid]; the caller's lab [m_valid] (int), part [M_pad, vpad / 64] (float2),
// llog [M_pad], out [m_valid].
extern "C" int rs_debug_decoder(const void* A, const void* W, const float* bias, const int* label, int M_pad, int m_valid,
                                int vpad, int vocab, int K, int* lab, void* part, float* llog, float* out, void* stream) {
    if (!A || !W || !bias || !label || !lab || !part || !llog || !out) return -1;
    if (m_valid <= 0 || M_pad != (m_valid + 255) / 256 * 256 || vpad <= 0 || vpad % 128 || vocab <= 0 || vocab > vpad ||
        K <= 0 || K % 64)
        return -1;
    SeqMeta sm{};
    sm.label = label;
    const MlmDecoder d{(const f16*)A, (const f16*)W, bias, m_valid, vpad, vocab, K, nullptr, sm, 0, lab,
                       (float2*)part, llog, out};
    const hipError_t e = launch_mlm_decoder(d, (hipStream_t)stream, [](bool, auto&& launch) { return launch(); });
    return e == hipSuccess ? 0 : -2;
}

// Test entry (not part of the scoring path): the top-k form of the decoder as head_mlm runs it
// (launch_mlm_decoder_topk).  Arguments as rs_debug_decoder, then k (1 .. 16, <= vocab), the
// caller's cand [min(M_pad, 2048), vpad / 64, k] (float2) and the outputs top_id (int) / top_lp
// [m_valid, k].
extern "C" int rs_debug_decoder_topk(const void* A, const void* W, const float* bias, const int* label, int M_pad,
                                     int m_valid, int vpad, int vocab, int K, int* lab, void* part, float* llog, float* out,
                                     int k, void* cand, int* top_id, float* top_lp, void* stream) {
    if (!A || !W || !bias || !label || !lab || !part || !llog || !out || !cand || !top_id || !top_lp) return -1;
    if (m_valid <= 0 || M_pad != (m_valid + 255) / 256 * 256 || vpad <= 0 || vpad % 128 || vocab <= 0 || vocab > vpad ||
        K <= 0 || K % 64 || k < 1 || k > TOPK_MAX || k > vocab)
        return -1;
    SeqMeta sm{};
    sm.label = label;
    const MlmDecoder d{(const f16*)A, (const f16*)W, bias, m_valid, vpad, vocab, K, nullptr, sm, 0, lab,
                       (float2*)part, llog, out};
    const MlmTopk t{k, (float2*)cand, top_id, top_lp};
    const hipError_t e = launch_mlm_decoder_topk(d, t, (hipStream_t)stream, [](bool, auto&& launch) { return launch(); });
    return e == hipSuccess ? 0 : -2;
}

// Test entry (not part of the scoring path): the candidate form of the decoder as head_mlm runs it
// (launch_mlm_decoder_cands).  A / W / bias / M_pad / m_valid / vpad / vocab / K / part as
// rs_debug_decoder; c_off [m_valid + 1], cand_id / perm [n_c] (n_c = c_off[m_valid]) device int32,
// row i's ids ascending and perm a permutation of [0, n_c); the caller's cand_logit [n_c] and the
// output out [n_c].  c_off and perm are read back and checked (ascending from 0; perm inside
// [0, n_c)), so a malformed list is -1 and nothing is launched.  Synchronises the stream first.
extern "C" int rs_debug_decoder_cands(const void* A, const void* W, const float* bias, int M_pad, int m_valid, int vpad,
                                      int vocab, int K, void* part, const int* c_off, const int* cand_id, const int* perm,
                                      float* cand_logit, float* out, void* stream) {
    if (!A || !W || !bias || !part || !c_off) return -1;
    if (m_valid <= 0 || M_pad != (m_valid + 255) / 256 * 256 || vpad <= 0 || vpad % 128 || vocab <= 0 || vocab > vpad ||
        K <= 0 || K % 64)
        return -1;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int> off((size_t)m_valid + 1);
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(off.data(), c_off, off.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return -2;
    if (off[0] != 0) return -1;
    for (int i = 0; i < m_valid; ++i)
        if (off[i + 1] < off[i]) return -1;
    const int n_c = off[m_valid];
    if (n_c > 0) {
        if (!cand_id || !perm || !cand_logit || !out) return -1;
        std::vector<int> pm((size_t)n_c);
        if (hipMemcpy(pm.data(), perm, pm.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -2;
        for (int t = 0; t < n_c; ++t)
            if (pm[t] < 0 || pm[t] >= n_c) return -1;
    }
    const MlmDecoder d{(const f16*)A, (const f16*)W, bias, m_valid, vpad, vocab, K, nullptr, SeqMeta{}, 0, nullptr,
                       (float2*)part, nullptr, nullptr};
    const MlmCands c{c_off, cand_id, perm, 0, n_c, cand_logit, out};
    const hipError_t e = launch_mlm_decoder_cands(d, c, st, [](bool, auto&& launch) { return launch(); });
    return e == hipSuccess ? 0 : -2;
}

// Timing/diagnostic entry (not part of the scoring path): one LayerNorm-family launch over
// `rows` rows of H = 768.  kind 0 ln_rows, 1 ln_res_rows (x written back), 2 ln_res_rows
// (deferred: stats + image only), 3 two-block ln_res_rows, 4 memory skeleton of kind 3.
extern "C" int rs_debug_ln(int kind, int rows, float* x32, float2* stats, float2* stats1, const void* o1,
                           const void* o2, const float* g, const float* b, void* y16, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int H = 768;
    hipError_t e = hipSuccess;
    if (kind == 0) e = launch_ln_rows(x32, rows, g, b, 1e-12f, H, nullptr, stats, (f16*)y16, 1, st);
    else if (kind == 1) e = launch_ln_res_rows(x32, stats, stats, g, b, (const f16*)o1, rows, g, b, 1e-12f, H, (f16*)y16, true, st);
    else if (kind == 2) e = launch_ln_res_rows(x32, stats, stats1, g, b, (const f16*)o1, rows, g, b, 1e-12f, H, (f16*)y16, false, st);
    else if (kind == 3)
        e = launch_ln_res_rows(x32, stats, stats, g, b, (const f16*)o1, rows, g, b, 1e-12f, H, (f16*)y16, true, st, stats1,
                               g, b, (const f16*)o2);
    else {
        hipLaunchKernelGGL(lnres_memskel_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x32, (const f16*)o1,
                           (const f16*)o2, rows, (f16*)y16);
        e = hipGetLastError();
    }
    return e == hipSuccess ? 0 : -2;
}

// Test entry (not part of the scoring path): embed_out_kernel through the production launcher over
// sequences [s0, s1) of the device metadata arrays len / row / tok_off (each [>= s1]).  The row of
// position t of sequence s is row[s] - row0 + t in the source: (x32 [rows, H], stats [rows], g, b
// [H]) or, himg != null, the interleaved two-part image [rows, 2H].  out: fp16 [tokens, H], or
// (two != 0) the planar two-part image [tokens, 2H], written at token tok_off[s] + t.
extern "C" int rs_debug_embed_out(const float* x32, const void* stats, const float* g, const float* b, const void* himg,
                                  const int* len, const int* row, const int* tok_off, int s0, int s1, int row0, int H,
                                  int two, void* d_out, void* stream) {
    if (!len || !row || !tok_off || !d_out || s0 < 0 || s1 <= s0) return -1;
    if (!himg && (!x32 || !stats || !g || !b)) return -1;
    SeqMeta sm{};
    sm.len = len;
    sm.row = row;
    sm.tok_off = tok_off;
    const hipError_t e = launch_embed_out(x32, (const float2*)stats, g, b, sm, s0, s1, row0, H, (f16*)d_out,
                                          (hipStream_t)stream, (const f16*)himg, two != 0);
    return e == hipSuccess ? 0 : -2;
}

// Test entries (not part of the scoring path) for tests/test_gpu_front_ops.py: the layer-0 front end,
// the scored-row gathers and the two small heads, each through its production launcher.  The metadata
// is a DebugMeta of device int32 arrays (common.h); every entry returns -1 without launching on a
// bad argument and -2 when the launcher reports an error.

// form 0 launch_embed_ln (rows row[s] - row0 + t), 1 launch_embed_ln_set ([MASK] at the positions
// pos[first[s] .. first[s + 1]); rows row[s] + t, row0 must be 0), 2 launch_embed_unique (h16 = the
// unique-row image [>= urows, kx H]; x32 / stats unused, row0 must be 0).  tok (and type, nullable) are
// indexed by tok_off[s] + t; word [vocab, H], pos [>= longest T, H], typetab [type_vocab, H], g, b [H].
// Forms 0 / 1: any of x32 [rows, H], stats [rows, 2], h16 [rows, kx H] may be null, not all three.
extern "C" int rs_debug_embed(int form, const int* tok, const int* type, const DebugMeta* dm, int s0, int s1, int row0,
                              int urows, int mask_id, int vocab, int type_vocab, const float* word, const float* pos,
                              const float* typetab, const float* g, const float* b, float eps, int H, float* x32,
                              void* stats, void* h16, int kx, void* stream) {
    if (!tok || !dm || !word || !pos || !typetab || !g || !b) return -1;
    if (form < 0 || form > 2 || s0 < 0 || s1 <= s0 || vocab <= 0 || type_vocab <= 0) return -1;
    if (H <= 0 || H % 256 || H > 1024 || kx < 1 || kx > 3) return -1;
    if (!dm->tok_off || !dm->len) return -1;
    const SeqMeta sm = debug_seq_meta(*dm);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (form == 2) {
        if (!dm->mask_pos || !dm->urow_h || !dm->urow_m || !h16 || urows <= 0 || row0 != 0) return -1;
        e = launch_embed_unique(tok, type, sm, s0, s1, urows, mask_id, vocab, type_vocab, word, pos, typetab, g, b, eps, H,
                                (f16*)h16, kx, st);
    } else {
        if (!dm->row || (!x32 && !stats && !h16)) return -1;
        if (form == 1) {
            if (!dm->first || !dm->pos || row0 != 0) return -1;
            e = launch_embed_ln_set(tok, type, sm, debug_query_meta(*dm), s0, s1, mask_id, vocab, type_vocab, word, pos,
                                    typetab, g, b, eps, H, x32, (float2*)stats, (f16*)h16, kx, st);
        } else {
            if (!dm->mask_pos || !dm->mask_end) return -1;
            e = launch_embed_ln(tok, type, sm, s0, s1, row0, mask_id, vocab, type_vocab, word, pos, typetab, g, b, eps, H,
                                x32, (float2*)stats, (f16*)h16, kx, st);
        }
    }
    return e == hipSuccess ? 0 : -2;
}

// op 0 launch_gather_query_rows over sequences [a0, a1) (source row row[s] - row0 + query[s]),
// 1 launch_gather_query_rows_list over the n = a1 queries from a0 (source row row[seq[q]] + pos[q]),
// 2 launch_gather_labels over sequences [a0, a1), 3 launch_gather_labels_list over a1 queries from a0.
// src / dst: fp16 rows of ld halfs (ops 0, 1); tok (nullable), lab (int) and llog (float) (ops 2, 3).
extern "C" int rs_debug_gather(int op, const void* src, int ld, const int* tok, const DebugMeta* dm, int a0, int a1,
                               int row0, void* dst, int* lab, float* llog, void* stream) {
    if (!dm || op < 0 || op > 3 || a0 < 0) return -1;
    const bool list = op == 1 || op == 3, rows = op <= 1;
    if (list ? a1 <= 0 : a1 <= a0) return -1;
    if (rows ? (!src || !dst || ld <= 0 || !dm->row) : (!lab || !llog)) return -1;
    if (list ? (!dm->seq || !dm->pos || (!rows && !dm->qlabel)) : (!dm->query || (!rows && !dm->label))) return -1;
    if (!rows && tok && !dm->tok_off) return -1;
    if (list && row0 != 0) return -1;
    const SeqMeta sm = debug_seq_meta(*dm);
    const QueryMeta qm = debug_query_meta(*dm);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (op == 0) e = launch_gather_query_rows((const f16*)src, ld, sm, a0, a1, row0, (f16*)dst, st);
    else if (op == 1) e = launch_gather_query_rows_list((const f16*)src, ld, sm, qm, a0, a1, (f16*)dst, st);
    else if (op == 2) e = launch_gather_labels(tok, sm, a0, a1, lab, llog, st);
    else e = launch_gather_labels_list(tok, sm, qm, a0, a1, lab, llog, st);
    return e == hipSuccess ? 0 : -2;
}

// launch_cls_linear: out[r] = h[r] . w + b[0], h [rows, H] fp32.
extern "C" int rs_debug_cls_linear(const float* h, int rows, int H, const float* w, const float* b, float* out,
                                   void* stream) {
    if (!h || !w || !b || !out || rows <= 0 || H <= 0) return -1;
    return launch_cls_linear(h, rows, H, w, b, out, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

// launch_segsum_f64: out[h] = the float64 sum of row_lp[off[h] .. off[h + 1]) in row order, off [n + 1].
extern "C" int rs_debug_segsum(const float* row_lp, const int* off, int n, double* out, void* stream) {
    if (!row_lp || !off || !out || n <= 0) return -1;
    return launch_segsum_f64(row_lp, off, n, out, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}
