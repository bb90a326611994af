// Shared definitions for the gfx950 kernels and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef _Float16 f16;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define RS_WAVE 64

// GEMM epilogues (C = A[M,K] . W[N,K]^T, fp32 accumulate):
enum EpiKind {
    EPI_BIAS_F16 = 0,   // out16 = acc + bias                      (fused QKV projection)
    EPI_GELU_F16 = 1,   // out16 = gelu(acc + bias)                (BertIntermediate)
    EPI_GELU_F32 = 2,   // out32 = gelu(acc + bias)                (MLM transform, pre-LN)
    EPI_RES_F32 = 3,    // out32 = acc + bias + res32              (BertSelfOutput / BertOutput, pre-LN)
    EPI_LSE = 4,        // per-row partial (max, sum exp) over a 64-column slab + label logit
    EPI_BIAS_F32 = 5,   // out32 = acc + bias                      (QKV in the fp16x3 precision mode)
    EPI_RESLN_F32 = 6,  // out32 = acc + bias + LN(res32)          (same, residual kept pre-LN:
                        //   LN rebuilt from res_stats/res_g/res_b; out may alias res)
    EPI_LNRES_IMG = 7,  // h <- image(LN(acc + bias + h)), h the two-part image in out, in place
                        //   (split-operand residual blocks; row statistics exchanged between the
                        //   column tiles of a row panel inside the launch: gemm_x3s_kernel)
    EPI_LSE_TOPK = 8,   // EPI_LSE, and per (row, 64-column slab) its best topk_k (logit, column) pairs
    EPI_LSE_CAND = 9,   // EPI_LSE with, in place of the one label logit, the logit of every column of the
                        //   row's candidate list (cand_off / cand_id / cand_logit)
};

struct EpiArgs {
    const float* bias;     // [N]
    const float* res;      // [M, ldc] fp32 residual (EPI_RES_F32; pre-LN sum for EPI_RESLN_F32)
    const float2* res_stats;  // [M] (mean, 1/sqrt(var + eps)) of res rows (EPI_RESLN_F32)
    const float* res_g;    // [N] LayerNorm weight / bias applied to res (EPI_RESLN_F32)
    const float* res_b;
    void* out;             // [M, ldc]
    int ldc;
    int m_valid;           // rows >= m_valid are not stored
    int n_valid;           // columns >= n_valid are masked (EPI_LSE vocab padding)
    float2* lse_part;      // [M, n_parts] (max, sum exp) (EPI_LSE)
    int n_parts;
    const int* label;      // [M] label column per row (EPI_LSE)
    float* label_logit;    // [M]
    int kx;                // fp16 operand image width factor of the output (EPI_GELU_F16): 1 or 3
    int nlog;              // logical N (column offset of the image sections)
    int group_m;           // tile order: row panels per group (set by launch_gemm)
    // EPI_RESLN_F32 with res_o16 != null (deferred BertSelfOutput residual): the residual is
    // LN(LN0(res) + o16) with LN0 = (res_stats0, res_g0, res_b0) and LN = (res_stats, res_g,
    // res_b), i.e. the post-attention stream ln_res_rows did not write back (WX = false)
    const f16* res_o16;    // [M, ldc] fp16 O-projection output (bias included)
    const float2* res_stats0;
    const float* res_g0;
    const float* res_b0;
    // EPI_LNRES_IMG: LN = (res_g, res_b, ln_eps) over nlog columns; lnx: lnres_granules(M)
    // 8-B granules [M/256][N/256][256][2] {ln_tag, sum | M2}, then [M/256] {ln_tag, panel list}
    // (zeroed once by the owner); lncnt:
    // lnres_counter_bytes() of gang-ticket words and gang-id slots (zeroed once by the owner, left
    // zeroed by every launch); lnerr (sticky, the caller's): set to 1 when a statistics or gang wait
    // timed out; ln_tag: set by the launch
    void* lnx;
    unsigned* lncnt;
    unsigned* lnerr;
    unsigned ln_tag;
    float ln_eps;
    int diag;              // EPI_LNRES_IMG: 8 = every wait times out (RS_LNFUSE_DIAG, tests); 0 in production
    unsigned long long* dbg;  // stamp builds only (rs_debug_stamps): per-workgroup phase cycle sums
    // EPI_LSE_TOPK: topk_cand [M, n_parts, topk_k] (logit, column bits), best first (larger logit,
    // then lower column); slots past a slab's valid columns hold (-inf, INT_MAX)
    float2* topk_cand;
    int topk_k;            // 1 .. TOPK_MAX
    // EPI_LSE_CAND: row i owns cand_id[cand_off[i] .. cand_off[i + 1]), ascending (cand_off
    // [m_valid + 1]); cand_logit[t] = the logit of column cand_id[t], stored where that column is a
    // valid one (< n_valid), so an id outside [0, n_valid) leaves the launcher's preset
    const int* cand_off;
    const int* cand_id;
    float* cand_logit;
};
constexpr int TOPK_MAX = 16;         // == RS_TOPK_MAX (rescore.h)
constexpr int TOPK_SUB_ROWS = 2048;  // rows per decoder launch of the top-k form (bounds topk_cand)
// <= 4 column tiles of 256 rows x 2 statistics granules, then one list-claim granule per row panel
inline size_t lnres_granules(int m_pad) { return (size_t)m_pad * 4 * 2 + (size_t)m_pad / 256 + 1; }

// fp16 operand image of an fp32 activation row with logical width K:
//   kx == 1: [hi]                          (RS_PREC_FP16)
//   kx == 3: [hi | hi/64 | (x - hi)*64]    (RS_PREC_FP16X3, K-concatenated GEMM form)
//   kx == 2: hi and lo = (x - hi)*64 INTERLEAVED per 32-column K-step (RS_PREC_FP16X3,
//            split-operand GEMM form): [hi 0..31 | lo 0..31 | hi 32..63 | lo 32..63 | ...], so
//            one K-step of a row is one 128-B line and the x3s kernel's LDS-DMA requests whole
//            lines (round 6; the planar [hi | lo] form requested two 64-B halves per row and
//            K-step, and that kernel's K loop is request-rate bound: profiles/r5kline_*).
//            Column c's hi part sits at il_hi(c), its lo part 32 halves later.  The x3s kernel
//            forms 64 W_hi in registers; its weights are the same interleaved [W_hi | W_lo*64].
// paired with the weight image [W_hi | W_lo*64 | W_hi/64] the K-concatenated MFMA product is
// A_hi.W_hi + A_hi.W_lo + A_lo.W_hi (the power-of-two factors cancel exactly): fp32-level
// accuracy from fp16 MFMA in one accumulator.  The factors keep the lo parts out of the fp16
// subnormal range, which the f16 MFMA flushes: lo = x - hi is subnormal for |x| < 0.25, and
// weights of |W| ~ 0.05 have W_lo ~ 1e-5 (unscaled, those products were lost).
constexpr float X3_UP = 64.f, X3_DOWN = 1.f / 64.f;
__host__ __device__ __forceinline__ int il_hi(int c) { return ((c & ~31) << 1) | (c & 31); }
__device__ __forceinline__ f16 x3_mid(f16 hi) { return (f16)((float)hi * X3_DOWN); }
// lo = RNE(64 (v - hi)), formed as one fma of the fp16 hi with 64 v (v_fma_mix: 64 (v - hi) is
// exact in fp32, so the single rounding to fp16 gives the same bits as (v - hi) * 64 rounded)
__device__ __forceinline__ f16 x3_lo(float v, f16 hi) { return (f16)__builtin_fmaf((float)hi, -X3_UP, v * X3_UP); }
__device__ __forceinline__ void put_split(f16* row, int c, int K, int kx, float v) {
    const f16 hi = (f16)v;
    if (kx == 2) {
        row[il_hi(c)] = hi;
        row[il_hi(c) + 32] = x3_lo(v, hi);
        return;
    }
    row[c] = hi;
    if (kx == 3) {
        row[K + c] = x3_mid(hi);
        row[2 * K + c] = x3_lo(v, hi);
    }
}
// c % 4 == 0 (the four columns lie in one 32-column K-step)
__device__ __forceinline__ void put_split4(f16* row, int c, int K, int kx, float4 v) {
    const half4 hi = {(f16)v.x, (f16)v.y, (f16)v.z, (f16)v.w};
    const int ch = kx == 2 ? il_hi(c) : c;
    *(half4*)(row + ch) = hi;
    if (kx >= 2) {
        const half4 lo = {x3_lo(v.x, hi[0]), x3_lo(v.y, hi[1]), x3_lo(v.z, hi[2]), x3_lo(v.w, hi[3])};
        *(half4*)(row + (kx == 2 ? ch + 32 : 2 * K + c)) = lo;
    }
    if (kx == 3) {
        const half4 mid = {x3_mid(hi[0]), x3_mid(hi[1]), x3_mid(hi[2]), x3_mid(hi[3])};
        *(half4*)(row + K + c) = mid;
    }
}
// value of column c of a kx == 2 image row: hi + lo/64
__device__ __forceinline__ float2 il_parts(const f16* row, int c) {
    return make_float2((float)row[il_hi(c)], (float)row[il_hi(c) + 32]);
}
// the values of columns c .. c + 3 (c % 4 == 0) of a kx == 2 image row
__device__ __forceinline__ float4 il_load4(const f16* row, int c) {
    const half4 hi = *(const half4*)(row + il_hi(c)), lo = *(const half4*)(row + il_hi(c) + 32);
    return make_float4((float)hi[0] + (float)lo[0] * X3_DOWN, (float)hi[1] + (float)lo[1] * X3_DOWN,
                       (float)hi[2] + (float)lo[2] * X3_DOWN, (float)hi[3] + (float)lo[3] * X3_DOWN);
}

// Per-sequence metadata of a scoring call (structure of arrays, device).  A "sequence"
// is one BERT input: a masked copy of a hypothesis (MLM_PLL), a hypothesis
// (RescoreBert) or a caller-provided row (masked_logprob).
struct SeqMeta {
    const int* tok_off;    // offset of the sequence's [CLS] in the token buffer
    const int* len;        // T
    const int* mask_pos;   // first position replaced by [MASK] on device, -1 = none
    const int* query;      // row whose last-layer state is scored
    const int* label;      // label id at query, -1 = take tokens[tok_off + query]
    const int* row;        // first token row of the sequence (global row index)
    const int* urow_h;     // layer-0 dedup: first unique row of the sequence's hypothesis (chunk-local)
    const int* urow_m;     // layer-0 dedup: the unique row of the sequence's first [MASK] position (chunk-local)
    const int* mask_end;   // end of the [MASK] span [mask_pos, mask_end); -1 = none
};

// Query list of a multi-mask call (device copy of seq_plan.h QueryList, uploaded with SeqMeta):
// sequence s scores positions pos[first[s] .. first[s + 1]), ascending; seq[q] is the sequence of
// query q.  Query q's state row is row q - q0 of its chunk's per-query buffers (q0 = first[s0]).
struct QueryMeta {
    const int* first;      // [S + 1]
    const int* seq;        // [n_q]
    const int* pos;        // [n_q]
    const int* label;      // [n_q] label id, -1 = take tokens[tok_off + pos]
};

// The metadata the test entries rs_debug_embed / _attention_plan / _attention_mquery / _gather take
// (tests only; mirrored as _lib.DebugMeta): device int32 arrays, SeqMeta's then QueryMeta's (qlabel =
// QueryMeta.label).  An entry checks the ones its kernels read and leaves the others null.
struct DebugMeta {
    const int *tok_off, *len, *mask_pos, *mask_end, *query, *label, *row, *urow_h, *urow_m;
    const int *first, *seq, *pos, *qlabel;
};
inline SeqMeta debug_seq_meta(const DebugMeta& d) {
    SeqMeta sm{};
    sm.tok_off = d.tok_off; sm.len = d.len; sm.mask_pos = d.mask_pos; sm.query = d.query; sm.label = d.label;
    sm.row = d.row; sm.urow_h = d.urow_h; sm.urow_m = d.urow_m; sm.mask_end = d.mask_end;
    return sm;
}
inline QueryMeta debug_query_meta(const DebugMeta& d) { return QueryMeta{d.first, d.seq, d.pos, d.qlabel}; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// ---- launchers (defined in k_gemm.hip / k_bert.hip / k_attn.hip / k_rerank.hip) --------
// tag != 0: the same kernel instantiated under a name-tag option (k_gemm.hip P_TAG_OPROJ /
// P_TAG_FFN2; the kernel name only, besides RS_GEMM_GROUP_M_FFN2 for tag 2), so
// rocprofv3 separates the O-projection (tag 1) and BertOutput (tag 2) launches from the QKV
// launches of the same epilogue
hipError_t launch_gemm(int epi, const f16* A, const f16* W, int M_pad, int N_pad, int K,
                       const EpiArgs& ep, hipStream_t st, int tag = 0);
// split-operand fp16x3 GEMM (gemm_x3s_kernel): A the interleaved two-part image [M_pad, 2K]
// (kx == 2 above), W rows of ldw >= 2K halfs starting with the interleaved [W_hi | W_lo*64] image
// (ldw = 2K: the packed split-operand weights); epi EPI_BIAS_F32, EPI_GELU_F16 (interleaved
// two-part image out) or EPI_LNRES_IMG.  N_pad % 256 == 0, K % 32 == 0, K >= 64.
hipError_t launch_gemm_x3s(int epi, const f16* A, const f16* W, int ldw, int M_pad, int N_pad, int K,
                           const EpiArgs& ep, hipStream_t st);
int gemm_row_align();   // M padding granularity required by launch_gemm
int gemm_lnres_workgroups(int N_pad);   // grid of the fused residual + LayerNorm GEMM (whole gangs)
size_t lnres_counter_bytes();           // EpiArgs.lncnt size

// kx: width factor of the fp16 operand images written (1 or 3, see put_split);
// qkv32: the QKV projection is fp32 (fp16x3 mode) instead of fp16.
// LayerNorm output of one element from its row statistics: the single expression every
// kernel uses, so an LN rebuilt downstream (EPI_RESLN_F32, attention_query) is bit-identical
// to the one the LN kernel writes.
// Every multiply-add of the LayerNorm is spelled out (fmaf / __fmul_rn): left to -ffp-contract,
// the same source contracted differently in different kernels (embed_ln vs embed_unique), and
// the rows two kernels must produce bit-identically (layer-0 dedup) differed in the last bit.
__device__ __forceinline__ float ln_apply(float x, float2 st, float g, float b) {
    return __builtin_fmaf(__fmul_rn(x - st.x, st.y), g, b);
}

// embed_ln writes the pre-LN embedding sum (x32), its row statistics and the fp16 operand
// image of LN(x); ln_rows writes the operand image, the statistics and (y32 != null) LN(x).
// type (nullable): segment ids parallel to tok (clamped to [0, type_vocab)); typetab [type_vocab, H].
hipError_t launch_embed_ln(const int* tok, const int* type, SeqMeta sm, int s0, int s1, int row0, int mask_id,
                           int vocab, int type_vocab, const float* word, const float* pos, const float* typetab,
                           const float* g, const float* b, float eps, int H, float* x32,
                           float2* stats, f16* h16, int kx, hipStream_t st);
hipError_t launch_ln_rows(const float* x, int rows, const float* g, const float* b, float eps,
                          int H, float* y32, float2* stats, f16* y16, int kx, hipStream_t st);
// x = LN(x32; stats, pg, pb) + o16, then stats_out / fp16 image of LN(x; g, b) (kx == 1);
// write_x: x written back into x32 (else x32 is left as is and the consumer rebuilds x from
// x32, stats, o16: EpiArgs.res_o16 or a second ln_res_rows).  o16b != null (needs write_x):
// two residual blocks, x = LN(LN(x32; stats, pg, pb) + o16; stats1, g1, b1) + o16b.
// stats_out may alias stats.
hipError_t launch_ln_res_rows(float* x32, const float2* stats, float2* stats_out, const float* pg, const float* pb,
                             const f16* o16, int rows, const float* g, const float* b, float eps, int H,
                             f16* y16, bool write_x, hipStream_t st, const float2* stats1 = nullptr,
                             const float* g1 = nullptr, const float* b1 = nullptr, const f16* o16b = nullptr);
// fp16x3 split-operand mode: x32 <- LN(x32; stats, pg, pb) + o32 (o32 = the projection's fp32
// output, bias included), then its statistics (stats_out, may alias stats) and the operand image
// of LN(x32; g, b) with width factor kx
hipError_t launch_ln_res32(float* x32, const float2* stats, float2* stats_out, const float* pg, const float* pb,
                           const float* o32, int rows, const float* g, const float* b, float eps, int H, f16* y16,
                           int kx, hipStream_t st);
hipError_t launch_ln_res_img(f16* h16, const float* o32, int rows, const float* g, const float* b, float eps, int H,
                             hipStream_t st);
// Unique layer-0 rows (dedup): the urows rows of the chunk's plan (seq_plan.h: per run of copies of
// a hypothesis its T rows, then the [MASK] rows of the run's masked range), as the fp16 operand
// image of LN(embedding) (rows of SeqMeta.urow_*)
hipError_t launch_embed_unique(const int* tok, const int* type, SeqMeta sm, int s0, int s1, int urows, int mask_id,
                               int vocab, int type_vocab, const float* word, const float* pos, const float* typetab,
                               const float* g, const float* b, float eps, int H, f16* h16u, int kx, hipStream_t st);
// BERTScore recall matrix (k_bertscore.hip); items = (utterance, j0, j1, -) ref-column runs of
// at most bertscore_cols(two) columns; two: emb is the two-part image (split-operand cosines)
int bertscore_cols(bool two);
hipError_t launch_bertscore_recall(const f16* emb, int H, const int* hyp_off, const int* utt_off,
                                   const long long* mat_off, const int4* items, int n_items, float* rmat, float* rmat0,
                                   hipStream_t st, bool two = false);
// Last hidden state, L2-normalised per token, at out[(tok_off + t) * H * (two ? 2 : 1)] (BERTScore):
// fp16, or (two) the two-part image [hi | lo*64]
hipError_t launch_embed_out(const float* x32, const float2* stats, const float* g, const float* b,
                            SeqMeta sm, int s0, int s1, int row0, int H, f16* out, hipStream_t st,
                            const f16* himg = nullptr, bool two = false);
// H == 64 heads.  max_len > 0: longest sequence of the launch; it and (qkv32, dedup) choose the
// kernel (table in k_attn.hip): the 16x16x32 kernels serve launches whose sequences all fit one
// 64-key block, the 32x32x16 kernel the others (fewer K/V reloads).
// dedup: qkv holds unique rows; sequence s, position t reads row
// (mask_pos <= t < mask_end ? urow_m + (t - mask_pos) : urow_h + t)
hipError_t launch_attention_full(const void* qkv, bool qkv32, SeqMeta sm, int s0, int s1, int row0,
                                 int H, int heads, f16* ctx, int kx, hipStream_t st, bool dedup, int max_len);
// resq = LN(x32[query row]) (x32 pre-LN, with its row statistics and LN weight / bias)
hipError_t launch_attention_query(const void* qkv, bool qkv32, const float* x32, const float2* stats,
                                  const float* g, const float* b, SeqMeta sm, int s0, int s1,
                                  int row0, int H, int heads, f16* ctxq, float* resq, int kx,
                                  hipStream_t st, const void* qd = nullptr, const f16* himg = nullptr);
// The folded last-layer attention of the scored rows (k_attn.hip, RS_LASTFOLD): the K / V
// projections applied to the query side, so that no K / V row is projected.  Over sequences
// [s0, s1): himg the two-part image [rows, 2H] of the layer's input (row = sm.row[s] - row0 + t), tq
// the dense Q [s1 - s0, H]; weight images (fp32, built once at finalize): wkf [H, H] = Wk / 8 (row
// 64 h + d: head h's key weights, the softmax scale folded in), wvt [H, H] = Wv transposed
// (wvt[j][c] = Wv[c][j]), bv [H].  work: scratch for G and U, 2 * heads * H floats per sequence of a
// batch; the launcher cuts [s0, s1) into as many batches as work_bytes asks for (one, when
// work_bytes >= (s1 - s0) * heads * H * 8).  ctxq: the kx = 1 or 3 operand image, resq = hi + lo/64
// of the scored row's image.  H = 64 heads, H % 256 == 0, H <= 1024 (attention_fold_ok).
struct AttnFold {
    const f16* himg;
    const float *tq, *wkf, *wvt, *bv;
    SeqMeta sm;
    int s0, s1, row0, H, heads, kx;
    void* work;
    size_t work_bytes;
    f16* ctxq;
    float* resq;
};
bool attention_fold_ok(int H, int heads);
// dst[s - s0] = the first H floats of src's row at sequence s's query position (fp32 rows of ld floats):
// the scored rows' Q out of a full Q/K/V GEMM's output (RS_LASTQ=0 with the folded last layer)
hipError_t launch_gather_q32(const float* src, int ld, SeqMeta sm, int s0, int s1, int row0, int H, float* dst,
                             hipStream_t st);
// one batch [s0, s0 + n) of a's sequences: G = tq . Wk_h / 8 per head; softmax and U; ctxq = U . Wv_h^T + bv
hipError_t launch_fold_in(const AttnFold& a, int s0, int n, float* G, hipStream_t st);
hipError_t launch_fold_query(const AttnFold& a, int s0, int n, const float* G, float* U, hipStream_t st);
hipError_t launch_fold_out(const AttnFold& a, int s0, int n, const float* U, hipStream_t st);
// wrap(kind, flops, launch): kind 0 = a fold GEMM (flops = its 2 M N K), 1 = the query kernel; runs
// one launch and returns its error (the scorer's profiler scopes, or a plain call)
template <class Wrap>
hipError_t launch_attention_fold(const AttnFold& a, hipStream_t st, Wrap&& wrap) {
    if (a.s1 <= a.s0) return hipSuccess;
    if (!attention_fold_ok(a.H, a.heads)) return hipErrorInvalidValue;
    const size_t per = (size_t)a.heads * a.H;                 // floats of G (and of U) per sequence
    const size_t cap = a.work_bytes / (2 * per * sizeof(float));
    if (cap == 0) return hipErrorInvalidValue;
    for (int s = a.s0; s < a.s1;) {
        const int n = (int)(cap < (size_t)(a.s1 - s) ? cap : (size_t)(a.s1 - s));
        float *G = (float*)a.work, *U = G + (size_t)n * per;
        const double flops = 2.0 * n * (double)a.H * a.H;
        if (hipError_t e = wrap(0, flops, [&] { return launch_fold_in(a, s, n, G, st); })) return e;
        if (hipError_t e = wrap(1, 0.0, [&] { return launch_fold_query(a, s, n, G, U, st); })) return e;
        if (hipError_t e = wrap(0, flops, [&] { return launch_fold_out(a, s, n, U, st); })) return e;
        s += n;
    }
    return hipSuccess;
}
// dst[s - s0] = src[row of sequence s's query position], ld halfs per row
hipError_t launch_gather_query_rows(const f16* src, int ld, SeqMeta sm, int s0, int s1, int row0, f16* dst,
                                   hipStream_t st);
// lab[s - s0] = the label column of sequence s (SeqMeta.label, -1 = the token at its query
// position; tok == null: SeqMeta.label as given), and label_logit[s - s0] = -inf: the EPI_LSE
// epilogue stores a row's label logit only where a valid column equals the label, so a label
// outside [0, vocab) leaves -inf, a -inf log-prob, and the call's range guard reports it
hipError_t launch_gather_labels(const int* tok, SeqMeta sm, int s0, int s1, int* lab, float* label_logit,
                                hipStream_t st);
hipError_t launch_lse_finalize(const float2* part, int n_parts, const float* label_logit,
                               int rows, float* out, hipStream_t st);
// ---- multi-mask rows (query-list calls: several scored positions per sequence) ----
// embed_ln whose [MASK] test is "t is one of the sequence's query positions" (qm.pos, ascending)
hipError_t launch_embed_ln_set(const int* tok, const int* type, SeqMeta sm, QueryMeta qm, int s0, int s1, int mask_id,
                               int vocab, int type_vocab, const float* word, const float* pos, const float* typetab,
                               const float* g, const float* b, float eps, int H, float* x32, float2* stats, f16* h16,
                               int kx, hipStream_t st);
// launch_attention_query over every query of sequences [s0, s1): ctxq / resq row q - qm.first[s0];
// qd: dense Q rows in the same order
hipError_t launch_attention_mquery(const void* qkv, bool qkv32, const float* x32, const float2* stats, const float* g,
                                   const float* b, SeqMeta sm, QueryMeta qm, int s0, int s1, int H, int heads,
                                   f16* ctxq, float* resq, int kx, hipStream_t st, const void* qd = nullptr,
                                   const f16* himg = nullptr);
// dst[q - q0] = src[row of query q's (sequence, position)], queries [q0, q0 + n)
hipError_t launch_gather_query_rows_list(const f16* src, int ld, SeqMeta sm, QueryMeta qm, int q0, int n, f16* dst,
                                        hipStream_t st);
// launch_gather_labels over queries [q0, q0 + n): qm.label, -1 = the token at the query's position
hipError_t launch_gather_labels_list(const int* tok, SeqMeta sm, QueryMeta qm, int q0, int n, int* lab,
                                     float* label_logit, hipStream_t st);

// The MLM decoder over one state row per sequence of [s0, s0 + m_valid): out[i] =
// log_softmax(A[i] . W^T + bias)[label of sequence s0 + i] over the first `vocab` of vpad columns.
// Three launches: the labels (and the label logits' -inf), the EPI_LSE GEMM into part / llog, the
// merge of the 64-column slabs.  A [pad(m_valid, 256), K], W [vpad, K] fp16 operand images,
// vpad % 128 == 0; lab / llog [m_valid], part [m_valid, vpad / 64]: the caller's workspace.
struct MlmDecoder {
    const f16* A;
    const f16* W;
    const float* bias;     // [vpad]
    int m_valid, vpad, vocab, K;
    const int* tok;        // as launch_gather_labels takes them
    SeqMeta sm;
    int s0;
    int* lab;
    float2* part;
    float* llog;
    float* out;            // [m_valid]
    // query-list calls: the rows are queries [s0, s0 + m_valid) of qm (launch_gather_labels_list)
    const QueryMeta* qm = nullptr;
};
// wrap(is_gemm, launch) runs one launch and returns its error: the scorer's profiler scopes
// (rs_api.hip head_mlm), or a plain call (the rs_debug_decoder test entry)
template <class Wrap>
hipError_t launch_mlm_decoder(const MlmDecoder& d, hipStream_t st, Wrap&& wrap) {
    if (hipError_t e = wrap(false, [&] {
            return d.qm ? launch_gather_labels_list(d.tok, d.sm, *d.qm, d.s0, d.m_valid, d.lab, d.llog, st)
                        : launch_gather_labels(d.tok, d.sm, d.s0, d.s0 + d.m_valid, d.lab, d.llog, st);
        }))
        return e;
    EpiArgs ep{};
    ep.bias = d.bias; ep.m_valid = d.m_valid; ep.n_valid = d.vocab; ep.lse_part = d.part;
    ep.n_parts = d.vpad / 64; ep.label = d.lab; ep.label_logit = d.llog;
    const int al = gemm_row_align(), m_pad = (d.m_valid + al - 1) / al * al;
    if (hipError_t e = wrap(true, [&] { return launch_gemm(EPI_LSE, d.A, d.W, m_pad, d.vpad, d.K, ep, st, 0); }))
        return e;
    return wrap(false, [&] { return launch_lse_finalize(d.part, d.vpad / 64, d.llog, d.m_valid, d.out, st); });
}
// The same decoder with the model's k preferred tokens of every row: top_id / top_lp [m_valid, k],
// ordered by (larger logit, lower column), top_lp[i][j] = logit - logsumexp of row i, formed from the
// same slab (max, sum exp) pairs as out (a returned label's log-prob is out's, bitwise).  The GEMM
// runs as EPI_LSE_TOPK over sub-batches of TOPK_SUB_ROWS rows, so that the candidate workspace cand
// stays at topk_cand_bytes(vpad) whatever m_valid is; each sub-batch is merged (topk_merge) before
// the next overwrites cand.  part / llog / out are those of launch_mlm_decoder, bit for bit: a
// row's slab pairs do not depend on the rows launched with it.
struct MlmTopk {
    int k;                 // 1 .. min(TOPK_MAX, vocab)
    float2* cand;          // topk_cand_bytes(vpad)
    int* top_id;           // [m_valid, k]
    float* top_lp;         // [m_valid, k]
};
inline size_t topk_cand_bytes(int vpad) { return (size_t)TOPK_SUB_ROWS * (size_t)(vpad / 64) * TOPK_MAX * sizeof(float2); }
hipError_t launch_topk_merge(const float2* part, int n_parts, const float2* cand, int k, int rows, int* top_id,
                             float* top_lp, hipStream_t st);
template <class Wrap>
hipError_t launch_mlm_decoder_topk(const MlmDecoder& d, const MlmTopk& t, hipStream_t st, Wrap&& wrap) {
    if (t.k < 1 || t.k > TOPK_MAX || t.k > d.vocab) return hipErrorInvalidValue;
    if (hipError_t e = wrap(false, [&] { return launch_gather_labels(d.tok, d.sm, d.s0, d.s0 + d.m_valid, d.lab, d.llog, st); }))
        return e;
    const int n_parts = d.vpad / 64, al = gemm_row_align();
    for (int r0 = 0; r0 < d.m_valid; r0 += TOPK_SUB_ROWS) {
        const int n = d.m_valid - r0 < TOPK_SUB_ROWS ? d.m_valid - r0 : TOPK_SUB_ROWS;
        EpiArgs ep{};
        ep.bias = d.bias; ep.m_valid = n; ep.n_valid = d.vocab; ep.lse_part = d.part + (size_t)r0 * n_parts;
        ep.n_parts = n_parts; ep.label = d.lab + r0; ep.label_logit = d.llog + r0;
        ep.topk_cand = t.cand; ep.topk_k = t.k;
        const f16* A = d.A + (size_t)r0 * d.K;
        if (hipError_t e = wrap(true, [&] { return launch_gemm(EPI_LSE_TOPK, A, d.W, (n + al - 1) / al * al, d.vpad, d.K, ep, st, 0); }))
            return e;
        if (hipError_t e = wrap(false, [&] {
                return launch_topk_merge(ep.lse_part, n_parts, t.cand, t.k, n, t.top_id + (size_t)r0 * t.k,
                                         t.top_lp + (size_t)r0 * t.k, st);
            }))
            return e;
    }
    return wrap(false, [&] { return launch_lse_finalize(d.part, n_parts, d.llog, d.m_valid, d.out, st); });
}
// The same decoder with a caller-chosen list of columns per row (no label): row i owns entries
// [c_off[i], c_off[i + 1]) of cand_id, sorted ascending (duplicates are separate entries), and
// out[perm[t]] = logit of column cand_id[t] - logsumexp of row i, the logsumexp formed by
// lse_finalize's expression from the same slab pairs: the value is bit for bit what
// launch_mlm_decoder gives the row with that column as its label.  An id outside [0, vocab) yields
// -inf.  Three launches: the -inf preset of cand_logit [n_c], the EPI_LSE_CAND GEMM, the finalise.
// d.tok / sm / lab / llog / out are not used.
// The launch may be one chunk of a longer list: its rows' entries are [t0, t0 + n_c) of cand_id / perm,
// c_off holds those absolute entry numbers, and only cand_logit is the chunk's own.
struct MlmCands {
    const int* c_off;      // [m_valid + 1] device, ascending, c_off[0] == t0, c_off[m_valid] == t0 + n_c
    const int* cand_id;    // device, entry t at cand_id[t]
    const int* perm;       // device: the output index of entry t
    int t0, n_c;
    float* cand_logit;     // [n_c] workspace: entry t at cand_logit[t - t0]
    float* out;            // entry t at out[perm[t]]
};
hipError_t launch_fill_f32(float* p, size_t n, float v, hipStream_t st);
hipError_t launch_cand_finalize(const float2* part, int n_parts, const float* cand_logit, const int* c_off,
                                const int* perm, int rows, float* out, hipStream_t st);
template <class Wrap>
hipError_t launch_mlm_decoder_cands(const MlmDecoder& d, const MlmCands& c, hipStream_t st, Wrap&& wrap) {
    if (c.n_c < 0 || c.t0 < 0) return hipErrorInvalidValue;
    if (hipError_t e = wrap(false, [&] { return launch_fill_f32(c.cand_logit, (size_t)c.n_c, -INFINITY, st); })) return e;
    if (c.n_c > 0 && (!c.cand_id || !c.perm || !c.cand_logit || !c.out)) return hipErrorInvalidValue;
    float* const logit0 = c.n_c ? c.cand_logit - c.t0 : nullptr;   // indexed by the absolute entry number, from t0 on
    EpiArgs ep{};
    ep.bias = d.bias; ep.m_valid = d.m_valid; ep.n_valid = d.vocab; ep.lse_part = d.part;
    ep.n_parts = d.vpad / 64; ep.cand_off = c.c_off; ep.cand_id = c.cand_id; ep.cand_logit = logit0;
    const int al = gemm_row_align(), m_pad = (d.m_valid + al - 1) / al * al;
    if (hipError_t e = wrap(true, [&] { return launch_gemm(EPI_LSE_CAND, d.A, d.W, m_pad, d.vpad, d.K, ep, st, 0); }))
        return e;
    return wrap(false, [&] {
        return launch_cand_finalize(d.part, d.vpad / 64, logit0, c.c_off, c.perm, d.m_valid, c.out, st);
    });
}
hipError_t launch_cls_linear(const float* h, int rows, int H, const float* w, const float* b,
                             float* out, hipStream_t st);
hipError_t launch_segsum_f64(const float* row_lp, const int* hyp_seq_off, int n_hyp, double* out,
                             hipStream_t st);
