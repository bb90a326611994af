// N-best confusion network (Nbest_Align/preprocess.py:41-64,92-139; CorrectBart/get_feature.py): the fold of
// the pairwise alignments (top-1, hypothesis n) into one slot table, the table's oracle path against a
// transcript, and a per-slot weighted vote.  rs_align (k_align.hip) supplies the pairwise alignments.
//
// Merge (closed form of the reference's sequential fold, DESIGN "Confusion network"): hypothesis n puts
// k[n][g] of its tokens into gap g of the top-1 (g = 0..L1) and a[n][g] against top-1 position g.  Gap g
// gives K[g] = max_n k[n][g] slots, position g one more.  One workgroup per utterance: for every column the
// lanes scatter pos[r] = alignment entry of top-1 position r into LDS, then run over the gaps
// (k = pos[g] - pos[g-1] - 1, running maximum over n); a block prefix sum over the gaps gives the slot
// offsets.  A count launch writes K and the slot count, the caller sizes the table, a fill launch writes it.
//
// Oracle: E[s][j] = best distance between ref[j:] and the paths through slots[s:], one row per slot from the
// last slot up.  A row is A[j] = min(E[s+1][j] + (no gap in s), E[s+1][j+1] + (ref[j] not in s)) followed by
// the in-row chain E[s][j] = min(A[j], E[s][j+1] + 1), which is the suffix minimum of A[j'] + j' minus j: a
// wave scan, no serial walk.  The forward pass then carries the distance row F of the labels chosen so far
// and takes, per slot, the lowest first-column candidate whose advanced row still reaches E[0][0].
//
// Vote: one wave per slot, lanes over candidate columns; a candidate's mass is added in ascending column
// order in float64 by the lane that owns its first column, so the result does not depend on the launch.
// No atomics, no cross-workgroup waits; every loop is bounded by the lengths passed in.
#include <string>
#include "common.h"
#include "../../include/rescore.h"

namespace {

constexpr int CN_MAX_LEN = 4096;        // tokens per hypothesis / transcript (rs_align's limit; LDS rows)
constexpr int CN_MAX_N = 1024;          // columns staged per slot (oracle, vote)
constexpr int CN_BLOCK = 256;
constexpr int CN_INF = 1 << 29;

// Exclusive prefix sum of v over the block's CN_BLOCK threads (sh: CN_BLOCK ints); total = the block's sum.
__device__ inline int block_scan_excl(int v, int* sh, int& total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < CN_BLOCK; d <<= 1) {
        const int x = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    total = sh[CN_BLOCK - 1];
    const int incl = sh[t];
    __syncthreads();
    return incl - v;
}

struct MergeArgs {
    const int* ref_idx;          // rs_align outputs of the pairs (utterance-major, n ascending)
    const int* hyp_idx;
    const long long* out_off;
    const int* n_al;
    const int* utt_off;          // [n_utt + 1] over hypotheses
    const int* hyp_len;          // [n_hyp]
    const long long* gap_off;    // [n_utt + 1]: K of utterance u at gap_off[u] .. + L1 + 1
    int* K;
    int* n_slots;                // count: written; fill: unused
    const int* slot_off;         // fill: [n_utt + 1]
    const long long* cell_off;   // fill: [n_utt + 1], table of utterance u at cell_off[u], [slots][N]
    int* src;
    long long src_cap;
    int mode;
};

// pos[r] = index of the alignment entry that holds top-1 position r, pos[L1] = the alignment's length
__device__ inline void scatter_pos(const MergeArgs& a, int p, int L1, int* pos) {
    const long long o0 = a.out_off[p];
    const int na = a.n_al[p];
    for (int e = threadIdx.x; e < na; e += CN_BLOCK) {
        const int r = a.ref_idx[o0 + e];
        if (r >= 0 && r < L1) pos[r] = e;
    }
    if (threadIdx.x == 0) pos[L1] = na;
}

__global__ void __launch_bounds__(CN_BLOCK) cn_count_kernel(MergeArgs a) {
    __shared__ int pos[CN_MAX_LEN + 1], kmax[CN_MAX_LEN + 1], sh[CN_BLOCK];
    const int u = blockIdx.x, tid = threadIdx.x;
    const int h0 = a.utt_off[u], N = a.utt_off[u + 1] - h0;
    const int L1 = N > 0 ? a.hyp_len[h0] : 0;
    for (int g = tid; g <= L1; g += CN_BLOCK) kmax[g] = 0;
    __syncthreads();
    for (int c = 1; c < N; ++c) {
        const int p = h0 - u + c - 1, Lh = a.hyp_len[h0 + c];
        scatter_pos(a, p, L1, pos);
        __syncthreads();
        for (int g = tid; g <= L1; g += CN_BLOCK) {
            const int k = pos[g] - (g ? pos[g - 1] : -1) - 1;
            kmax[g] = max(kmax[g], min(max(k, 0), Lh));
        }
        __syncthreads();
    }
    int* K = a.K + a.gap_off[u];
    int carry = 0;
    for (int g0 = 0; g0 <= L1; g0 += CN_BLOCK) {
        const int g = g0 + tid;
        int v = 0, tot;
        if (g <= L1) {
            K[g] = kmax[g];
            v = kmax[g] + (g < L1 ? 1 : 0);
        }
        block_scan_excl(v, sh, tot);
        carry += tot;
    }
    if (tid == 0) a.n_slots[u] = N > 0 ? carry : 0;
}

__global__ void __launch_bounds__(CN_BLOCK) cn_fill_kernel(MergeArgs a) {
    __shared__ int pos[CN_MAX_LEN + 1], base[CN_MAX_LEN + 1], seen[CN_MAX_LEN + 1], sh[CN_BLOCK];
    const int u = blockIdx.x, tid = threadIdx.x;
    const int h0 = a.utt_off[u], N = a.utt_off[u + 1] - h0;
    if (N <= 0) return;
    const int L1 = a.hyp_len[h0];
    const int* K = a.K + a.gap_off[u];
    int carry = 0;
    for (int g0 = 0; g0 <= L1; g0 += CN_BLOCK) {
        const int g = g0 + tid;
        int tot;
        const int v = g <= L1 ? K[g] + (g < L1 ? 1 : 0) : 0;
        const int ex = block_scan_excl(v, sh, tot);
        if (g <= L1) {
            base[g] = carry + ex;
            seen[g] = 0;
        }
        carry += tot;
    }
    __syncthreads();
    const int S = a.slot_off[u + 1] - a.slot_off[u];
    if (carry != S) return;                      // a table sized from other counts: write nothing
    const long long c0 = a.cell_off[u];
    int* src = a.src;
    const long long cap = a.src_cap;
#define CN_PUT(slot, col, val)                                         \
    do {                                                               \
        const long long i_ = c0 + (long long)(slot) * N + (col);       \
        if (i_ >= 0 && i_ < cap) src[i_] = (val);                      \
    } while (0)
    for (int g = tid; g <= L1; g += CN_BLOCK) {  // column 0: the top-1
        const int kg = K[g];
        for (int m = 0; m < kg; ++m) CN_PUT(base[g] + m, 0, -1);
        if (g < L1) CN_PUT(base[g] + kg, 0, g);
    }
    for (int c = 1; c < N; ++c) {
        const int p = h0 - u + c - 1, Lh = a.hyp_len[h0 + c];
        const long long o0 = a.out_off[p];
        const int na = a.n_al[p];
        scatter_pos(a, p, L1, pos);
        __syncthreads();
        for (int g = tid; g <= L1; g += CN_BLOCK) {
            const int first = g ? pos[g - 1] + 1 : 0;
            const int k = min(max(pos[g] - first, 0), Lh);
            const int kg = K[g], sg = seen[g];
            int ag = -1;                          // a[c][g]: the entry against top-1 position g
            if (g < L1 && pos[g] >= 0 && pos[g] < na) ag = a.hyp_idx[o0 + pos[g]];
            for (int m = 0; m < kg; ++m) {
                int v = -1;
                if (m < k) {
                    const int e = first + m;
                    if (e >= 0 && e < na) v = a.hyp_idx[o0 + e];
                } else if (a.mode == RS_CN_REFERENCE && m < sg && g < L1) {
                    v = ag;                       // the reference's copy (its "*" branch keeps j in place)
                }
                CN_PUT(base[g] + m, c, v);
            }
            if (g < L1) CN_PUT(base[g] + kg, c, ag);
            seen[g] = max(sg, k);
        }
        __syncthreads();
    }
#undef CN_PUT
}

struct TableArgs {
    const int* src;
    const int* slot_off;
    const long long* cell_off;
    const int* utt_off;
    const int* tok;              // hypothesis token ids (>= 0), hypothesis h at hyp_off[h]
    const int* hyp_off;
};

// ent[c] = token id of slot s's column c, -1 for a gap
__device__ inline void load_slot(const TableArgs& t, int u, int s, int N, int h0, int* ent, int lane, int step) {
    const int* row = t.src + t.cell_off[u] + (long long)s * N;
    for (int c = lane; c < N; c += step) {
        const int i = row[c];
        const int b = t.hyp_off[h0 + c], len = t.hyp_off[h0 + c + 1] - b;
        ent[c] = (i >= 0 && i < len) ? t.tok[b + i] : -1;
    }
}

__device__ inline int wave_min(int v) {
    for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d));
    return v;
}

__global__ void __launch_bounds__(64)
cn_oracle_kernel(TableArgs t, const int* __restrict__ ref, const int* __restrict__ ref_off,
                 const long long* __restrict__ e_off, int* __restrict__ E, int* __restrict__ dist,
                 int* __restrict__ label) {
    __shared__ int ent[CN_MAX_N], first[CN_MAX_N], Frow[2][CN_MAX_LEN + 1];
    const int u = blockIdx.x, lane = threadIdx.x;
    const int h0 = t.utt_off[u], N = t.utt_off[u + 1] - h0;
    const int S = t.slot_off[u + 1] - t.slot_off[u];
    const int r0 = ref_off[u], R = ref_off[u + 1] - r0;
    const int W = R + 1, nch = (W + 63) >> 6;
    int* Eu = E + e_off[u];
    for (int j = lane; j <= R; j += 64) Eu[(long long)S * W + j] = R - j;
    __threadfence_block();
    __syncthreads();
    for (int s = S - 1; s >= 0; --s) {
        load_slot(t, u, s, N, h0, ent, lane, 64);
        __syncthreads();
        int g = 0, k = 0;
        for (int c = lane; c < N; c += 64) {
            g |= ent[c] < 0;
            k |= ent[c] >= 0;
        }
        const int skip = __any(g) ? 0 : 1;
        const bool hastok = __any(k);
        const int* En = Eu + (long long)(s + 1) * W;
        int* Es = Eu + (long long)s * W;
        int carry = CN_INF;
        for (int ch = nch - 1; ch >= 0; --ch) {
            const int j = (ch << 6) + lane;
            int B = CN_INF;
            if (j <= R) {
                int A = En[j] + skip;
                if (j < R && hastok) {
                    const int rv = ref[r0 + j];
                    int miss = 1;
                    for (int c = 0; c < N; ++c)
                        if (ent[c] == rv) { miss = 0; break; }
                    A = min(A, En[j + 1] + miss);
                }
                B = A + j;
            }
            for (int d = 1; d < 64; d <<= 1) {       // suffix minimum over the lanes
                const int o = __shfl_down(B, d);
                if (lane + d < 64) B = min(B, o);
            }
            B = min(B, carry);
            if (j <= R) Es[j] = B - j;
            carry = __shfl(B, 0);
        }
        __threadfence_block();                        // the row is read by other lanes next
        __syncthreads();
    }
    const int best = Eu[0];
    if (lane == 0) dist[u] = best;
    for (int j = lane; j <= R; j += 64) Frow[0][j] = j;
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < S; ++s) {
        load_slot(t, u, s, N, h0, ent, lane, 64);
        __syncthreads();
        for (int c = lane; c < N; c += 64) {
            int f = 1;
            for (int b = 0; b < c; ++b)
                if (ent[b] == ent[c]) { f = 0; break; }
            first[c] = f;
        }
        __syncthreads();
        const int* En = Eu + (long long)(s + 1) * W;
        const int* F = Frow[cur];
        int* Fn = Frow[cur ^ 1];
        int pick = -1;
        for (int c = 0; c < N; ++c) {                 // candidates in order of their first column
            if (!first[c]) continue;
            const int tv = ent[c];
            int m = CN_INF;
            if (tv < 0) {                             // the gap: the row stays
                for (int j = lane; j <= R; j += 64) m = min(m, F[j] + En[j]);
            } else {
                int carry = CN_INF;
                for (int ch = 0; ch < nch; ++ch) {
                    const int j = (ch << 6) + lane;
                    int C = CN_INF;
                    if (j <= R) {
                        int A = F[j] + 1;
                        if (j >= 1) A = min(A, F[j - 1] + (tv != ref[r0 + j - 1] ? 1 : 0));
                        C = A - j;
                    }
                    for (int d = 1; d < 64; d <<= 1) {    // prefix minimum over the lanes
                        const int o = __shfl_up(C, d);
                        if (lane >= d) C = min(C, o);
                    }
                    C = min(C, carry);
                    if (j <= R) {
                        Fn[j] = C + j;
                        m = min(m, C + j + En[j]);
                    }
                    carry = __shfl(C, 63);
                }
            }
            if (wave_min(m) == best) {
                pick = c;
                if (tv >= 0) cur ^= 1;
                break;
            }
        }
        if (lane == 0) label[t.slot_off[u] + s] = pick;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(CN_BLOCK)
cn_vote_kernel(TableArgs t, const double* __restrict__ w, int* __restrict__ win_tok, int* __restrict__ win_col,
               double* __restrict__ share, int* __restrict__ dec, int* __restrict__ dec_len) {
    __shared__ int ent[CN_BLOCK / 64][CN_MAX_N], sh[CN_BLOCK];
    __shared__ double total_sh;
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int h0 = t.utt_off[u], N = t.utt_off[u + 1] - h0;
    const int s_base = t.slot_off[u], S = t.slot_off[u + 1] - s_base;
    if (tid == 0) {
        double tot = 0.0;
        for (int n = 0; n < N; ++n) tot += w[h0 + n];
        total_sh = tot;
    }
    __syncthreads();
    const double total = total_sh;
    for (int s0 = 0; s0 < S; s0 += CN_BLOCK / 64) {
        const int s = s0 + wv;
        int* e = ent[wv];
        if (s < S) load_slot(t, u, s, N, h0, e, lane, 64);
        __syncthreads();
        if (s < S) {
            double bm = 0.0;
            int bc = 0x7fffffff;
            for (int c = lane; c < N; c += 64) {
                const int tv = e[c];
                bool f = true;
                for (int b = 0; b < c; ++b)
                    if (e[b] == tv) { f = false; break; }
                if (!f) continue;
                double mass = 0.0;
                for (int n = c; n < N; ++n)           // ascending column order: a fixed float64 sum
                    if (e[n] == tv) mass += w[h0 + n];
                if (bc == 0x7fffffff || mass > bm) { bm = mass; bc = c; }
            }
            for (int d = 32; d; d >>= 1) {
                const double om = __shfl_xor(bm, d);
                const int oc = __shfl_xor(bc, d);
                if (oc != 0x7fffffff && (bc == 0x7fffffff || om > bm || (om == bm && oc < bc))) { bm = om; bc = oc; }
            }
            if (lane == 0 && bc != 0x7fffffff) {
                win_tok[s_base + s] = e[bc];
                win_col[s_base + s] = bc;
                share[s_base + s] = bm / total;
            }
        }
        __syncthreads();
    }
    // the decode without gaps: winners written by other waves are read here
    __threadfence_block();
    __syncthreads();
    int carry = 0;
    for (int s0 = 0; s0 < S; s0 += CN_BLOCK) {
        const int s = s0 + tid;
        const int tv = s < S ? win_tok[s_base + s] : -1;
        int tot;
        const int ex = block_scan_excl(tv >= 0 ? 1 : 0, sh, tot);
        if (tv >= 0) dec[s_base + carry + ex] = tv;
        carry += tot;
    }
    if (tid == 0) dec_len[u] = carry;
}

}  // namespace

int rs_fail(int code, const std::string& msg);

static int cn_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RS_OK : rs_fail(RS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

extern "C" {

int rs_cn_merge(const int32_t* d_ref_idx, const int32_t* d_hyp_idx, const int64_t* d_out_off, const int32_t* d_n,
                const int32_t* d_utt_off, const int32_t* d_hyp_len, int32_t n_utt, int32_t max_len,
                const int64_t* d_gap_off, int32_t* d_K, int32_t* d_n_slots, const int32_t* d_slot_off,
                const int64_t* d_cell_off, int32_t* d_src, int64_t src_cap, int32_t mode, void* stream) {
    if (n_utt < 0 || max_len < 0) return rs_fail(RS_EARG, "rs_cn_merge: negative size");
    if (mode != RS_CN_REFERENCE && mode != RS_CN_EXACT) return rs_fail(RS_EARG, "rs_cn_merge: unknown mode");
    if (max_len > CN_MAX_LEN) return rs_fail(RS_EUNSUP, "rs_cn_merge: token lists are limited to 4096 tokens");
    if (n_utt == 0) return RS_OK;
    if (!d_ref_idx || !d_hyp_idx || !d_out_off || !d_n || !d_utt_off || !d_hyp_len || !d_gap_off || !d_K)
        return rs_fail(RS_EARG, "rs_cn_merge: null argument");
    MergeArgs a{d_ref_idx, d_hyp_idx, (const long long*)d_out_off, d_n, d_utt_off, d_hyp_len,
                (const long long*)d_gap_off, d_K, d_n_slots, d_slot_off, (const long long*)d_cell_off, d_src,
                (long long)src_cap, mode};
    if (!d_src) {                                    // count launch
        if (!d_n_slots) return rs_fail(RS_EARG, "rs_cn_merge: count launch without d_n_slots");
        hipLaunchKernelGGL(cn_count_kernel, dim3(n_utt), dim3(CN_BLOCK), 0, (hipStream_t)stream, a);
        return cn_launched("rs_cn_merge (count)");
    }
    if (!d_slot_off || !d_cell_off || src_cap < 0)
        return rs_fail(RS_EARG, "rs_cn_merge: fill launch without slot / cell offsets");
    hipLaunchKernelGGL(cn_fill_kernel, dim3(n_utt), dim3(CN_BLOCK), 0, (hipStream_t)stream, a);
    return cn_launched("rs_cn_merge (fill)");
}

static int cn_table_args(const char* who, const int32_t* d_src, const int32_t* d_slot_off, const int64_t* d_cell_off,
                         const int32_t* d_utt_off, const int32_t* d_tok, const int32_t* d_hyp_off, int32_t n_utt,
                         int32_t max_n, TableArgs& t) {
    if (n_utt < 0 || max_n < 0) return rs_fail(RS_EARG, std::string(who) + ": negative size");
    if (max_n > CN_MAX_N) return rs_fail(RS_EUNSUP, std::string(who) + ": at most 1024 hypotheses per utterance");
    if (n_utt > 0 && (!d_src || !d_slot_off || !d_cell_off || !d_utt_off || !d_tok || !d_hyp_off))
        return rs_fail(RS_EARG, std::string(who) + ": null argument");
    t = TableArgs{d_src, d_slot_off, (const long long*)d_cell_off, d_utt_off, d_tok, d_hyp_off};
    return RS_OK;
}

int rs_cn_oracle(const int32_t* d_src, const int32_t* d_slot_off, const int64_t* d_cell_off,
                 const int32_t* d_utt_off, const int32_t* d_tok, const int32_t* d_hyp_off, int32_t n_utt,
                 int32_t max_n, const int32_t* d_ref, const int32_t* d_ref_off, int32_t max_ref,
                 const int64_t* d_e_off, int32_t* d_E, int32_t* d_dist, int32_t* d_label, void* stream) {
    TableArgs t;
    const int rc = cn_table_args("rs_cn_oracle", d_src, d_slot_off, d_cell_off, d_utt_off, d_tok, d_hyp_off, n_utt,
                                 max_n, t);
    if (rc != RS_OK) return rc;
    if (max_ref < 0) return rs_fail(RS_EARG, "rs_cn_oracle: negative size");
    if (max_ref > CN_MAX_LEN) return rs_fail(RS_EUNSUP, "rs_cn_oracle: transcripts are limited to 4096 tokens");
    if (n_utt == 0) return RS_OK;
    if (!d_ref || !d_ref_off || !d_e_off || !d_E || !d_dist || !d_label)
        return rs_fail(RS_EARG, "rs_cn_oracle: null argument");
    hipLaunchKernelGGL(cn_oracle_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, t, d_ref, d_ref_off,
                       (const long long*)d_e_off, d_E, d_dist, d_label);
    return cn_launched("rs_cn_oracle");
}

int rs_cn_vote(const int32_t* d_src, const int32_t* d_slot_off, const int64_t* d_cell_off,
               const int32_t* d_utt_off, const int32_t* d_tok, const int32_t* d_hyp_off, int32_t n_utt,
               int32_t max_n, const double* d_w, int32_t* d_win_tok, int32_t* d_win_col, double* d_share,
               int32_t* d_dec, int32_t* d_dec_len, void* stream) {
    TableArgs t;
    const int rc = cn_table_args("rs_cn_vote", d_src, d_slot_off, d_cell_off, d_utt_off, d_tok, d_hyp_off, n_utt,
                                 max_n, t);
    if (rc != RS_OK) return rc;
    if (n_utt == 0) return RS_OK;
    if (!d_w || !d_win_tok || !d_win_col || !d_share || !d_dec || !d_dec_len)
        return rs_fail(RS_EARG, "rs_cn_vote: null argument");
    hipLaunchKernelGGL(cn_vote_kernel, dim3(n_utt), dim3(CN_BLOCK), 0, (hipStream_t)stream, t, d_w, d_win_tok,
                       d_win_col, d_share, d_dec, d_dec_len);
    return cn_launched("rs_cn_vote");
}

}  // extern "C"
