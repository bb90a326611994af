// C-ABI trainer (include/rescore.h, rs_trainer_*): RescoreBert distillation training
// (RescoreBert/main.py:104-229 — MD / MD_MWER / MD_MWED) on the GPU.
//
// One step = forward over the batch's hypotheses with every activation the backward needs
// saved (ragged token rows, no padding), the loss and its gradient w.r.t. the CLS scores,
// the backward through the head, the encoder layers and the embeddings, then one
// torch.optim.AdamW update.  Parameters, gradients and Adam moments are single flat fp32
// buffers (one AdamW launch); the fused Q|K|V weight is the contiguous [q; k; v] range of
// the three HF tensors.  GEMMs: tr_sgemm (k_sgemm.hip: f32-input MFMA, exact fp32, split-K
// through an ordered workspace sum — deterministic); RS_TRAIN_ROCBLAS=1 routes them to rocBLAS
// sgemm instead (atomics disabled), kept as the timing / numerics baseline.
// Optimizer options (rs_trainer_accumulate / _apply / _grad_norm / _set_trainable): gradient
// accumulation, clip_grad_norm_ and frozen tensors are range arithmetic over those flat buffers; a
// step that uses none of them launches what it always did.
// All other ops: k_train.hip.  Dropout (BERT's train mode, train.h TrDrop): hidden dropout after
// the embedding LayerNorm and on both residual branches, attention-probability dropout; the keep
// bits are counter-based draws keyed by (dropout_seed, the trainer's dropout-step counter), so a
// step is bitwise reproducible and the backward recomputes the mask.
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>
#include <cstring>
#include <cmath>
#include <cstdlib>

#include <rocblas/rocblas.h>

#include "common.h"
#include "train.h"
#include "host_util.h"

namespace {

// (TRY_ALLOC: the saved attention probabilities of long batches are the large allocation,
// layers * sum_s heads * T_s^2 * 4 bytes)
#define TRY_BLAS(expr)                                                                      \
    do {                                                                                    \
        rocblas_status s_ = (expr);                                                         \
        if (s_ != rocblas_status_success)                                                   \
            return rs_fail(RS_EHIP, std::string(#expr) + ": " + rocblas_status_to_string(s_)); \
    } while (0)

struct TLayer {
    size_t wqkv, bqkv, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2;
};

}  // namespace

struct rs_trainer {
    rs_bert_cfg cfg{};
    int device = 0;
    bool finalized = false;
    rocblas_handle blas = nullptr;
    bool use_rocblas = false;                                 // RS_TRAIN_ROCBLAS=1 (baseline)
    int attn_mode = 0;              // RS_TRAIN_ATTN: 0 auto (tiled above 128 tokens), 1 tiled, 2 legacy
    std::map<std::string, std::pair<size_t, size_t>> table;   // HF key -> (offset, numel) in floats
    std::vector<float> host;                                  // staged parameters until finalize
    std::vector<char> set;                                    // per table entry: provided?
    size_t n_params = 0;
    size_t o_word = 0, o_pos = 0, o_type = 0, o_eg = 0, o_eb = 0, o_wl = 0, o_bl = 0;
    size_t o_wt = 0, o_bt = 0, o_tg = 0, o_tb = 0, o_db = 0;   // MLM head (decoder tied to o_word)
    std::vector<TLayer> lay;
    DevBuf P, G, M1, V1;       // parameters, gradients, Adam moments
    DevBuf act, grad, meta, small, ws;   // ws: split-K partials of tr_sgemm
    long long step = 0;
    uint64_t drop_step = 0;         // dropout-step counter (key of the next dropout-active step)
    std::vector<int> h_tok, h_meta, h_type;
    // rs_trainer_set_token_types: segment ids of the next step, [type_n] device ints (null: all 0)
    const int32_t* type_next = nullptr;
    int64_t type_n = 0;
    // Frozen tensors (rs_trainer_set_trainable): their offsets, and the maximal merged ranges of the
    // trainable ones (64-float aligned; one range [0, n_params) while nothing is frozen) that AdamW,
    // the gradient norm and the accumulation run over
    std::set<size_t> frozen;
    std::vector<TrRange> ranges;
    DevBuf A, nws;             // gradient accumulator (allocated at the first rs_trainer_accumulate); norm partials
    bool have_grad = false;    // t->G holds the gradient of a completed backward under the current trainable set
    bool acc_filled = false;   // a micro-batch has been accumulated since the last clear
    bool on(size_t off) const { return !frozen.count(off); }
};

namespace {

size_t add_tensor(rs_trainer* t, const std::string& key, size_t n) {
    size_t off = (t->n_params + 63) / 64 * 64;
    t->table[key] = {off, n};
    t->n_params = off + n;
    return off;
}

// the maximal merged ranges of the trainable tensors, each tensor padded to its 64-float slot
void merge_ranges(rs_trainer* t) {
    std::map<size_t, size_t> by_off;                          // offset -> numel
    for (auto& kv : t->table) by_off[kv.second.first] = kv.second.second;
    t->ranges.clear();
    for (auto& on : by_off) {
        if (t->frozen.count(on.first)) continue;
        const long long b = (long long)on.first, e = (long long)((on.first + on.second + 63) / 64 * 64);
        if (!t->ranges.empty() && t->ranges.back().off + t->ranges.back().n == b)
            t->ranges.back().n = e - t->ranges.back().off;
        else
            t->ranges.push_back({b, e - b});
    }
}

// rocBLAS baseline (RS_TRAIN_ROCBLAS=1): the same three forms, column-major arguments
rocblas_status blas_nt(rocblas_handle h, int M, int N, int K, const float* X, const float* W, float* Y, float beta) {
    const float one = 1.0f;
    return rocblas_sgemm(h, rocblas_operation_transpose, rocblas_operation_none, N, M, K, &one, W, K, X, K, &beta, Y, N);
}
rocblas_status blas_nn(rocblas_handle h, int M, int N, int K, const float* dY, const float* W, float* dX, float beta) {
    const float one = 1.0f;
    return rocblas_sgemm(h, rocblas_operation_none, rocblas_operation_none, K, M, N, &one, W, K, dY, N, &beta, dX, K);
}
rocblas_status blas_tn(rocblas_handle h, int M, int N, int K, const float* dY, const float* X, float* dW, float beta) {
    const float one = 1.0f;
    return rocblas_sgemm(h, rocblas_operation_none, rocblas_operation_transpose, K, N, M, &one, X, K, dY, N, &beta, dW, K);
}

#define RS_TRY(expr)                     \
    do {                                 \
        if (int r_ = (expr)) return r_;  \
    } while (0)

// row-major Y[M, N] = X[M, K] . W[N, K]^T (+ beta Y)
int gemm_nt(rs_trainer* t, hipStream_t st, int M, int N, int K, const float* X, const float* W, float* Y, float beta) {
    if (t->use_rocblas) {
        TRY_BLAS(blas_nt(t->blas, M, N, K, X, W, Y, beta));
        return RS_OK;
    }
    TRY_HIP(tr_sgemm(M, N, K, X, K, true, W, K, true, Y, N, beta != 0.f, t->ws.as<float>(), t->ws.bytes / 4, st));
    return RS_OK;
}
// row-major dX[M, K] = dY[M, N] . W[N, K] (+ beta dX)
int gemm_nn(rs_trainer* t, hipStream_t st, int M, int N, int K, const float* dY, const float* W, float* dX, float beta) {
    if (t->use_rocblas) {
        TRY_BLAS(blas_nn(t->blas, M, N, K, dY, W, dX, beta));
        return RS_OK;
    }
    TRY_HIP(tr_sgemm(M, K, N, dY, N, true, W, K, false, dX, K, beta != 0.f, t->ws.as<float>(), t->ws.bytes / 4, st));
    return RS_OK;
}
// row-major dW[N, K] = dY[M, N]^T . X[M, K] (+ beta dW)
int gemm_tn(rs_trainer* t, hipStream_t st, int M, int N, int K, const float* dY, const float* X, float* dW, float beta) {
    if (t->use_rocblas) {
        TRY_BLAS(blas_tn(t->blas, M, N, K, dY, X, dW, beta));
        return RS_OK;
    }
    TRY_HIP(tr_sgemm(N, K, M, dY, N, false, X, K, false, dW, K, beta != 0.f, t->ws.as<float>(), t->ws.bytes / 4, st));
    return RS_OK;
}

// split-K workspace for every GEMM shape of a step over M token rows (forward, dgrad, wgrad of
// each Linear; the MLM head's transform and tied decoder)
size_t sgemm_ws_floats(const rs_bert_cfg& c, int M) {
    const int H = c.hidden, F = c.intermediate, V = c.heads_mask == RS_HEAD_MLM ? c.vocab : H;
    size_t w = 0;
    for (int n : {3 * H, H, F, V})
        for (int k : {H, F}) {
            w = std::max(w, tr_sgemm_ws_floats(M, n, k));   // forward (M, n, k)
            w = std::max(w, tr_sgemm_ws_floats(M, k, n));   // dgrad   (M, k, n)
            w = std::max(w, tr_sgemm_ws_floats(n, k, M));   // wgrad   (n, k, M)
        }
    return w;
}

}  // namespace

extern "C" {

int rs_trainer_create(const rs_bert_cfg* cfg, int device, rs_trainer** out) {
    if (!cfg || !out) return rs_fail(RS_EARG, "null argument");
    const rs_bert_cfg& c = *cfg;
    if (int r = check_bert_shape(c, 4)) return r;
    if (c.heads_mask != RS_HEAD_CLS && c.heads_mask != RS_HEAD_MLM)
        return rs_fail(RS_EUNSUP, "the trainer takes one head: RS_HEAD_CLS (RescoreBert) or RS_HEAD_MLM (MLM fine-tuning)");
    if (c.heads_mask == RS_HEAD_MLM && c.vocab % 4) return rs_fail(RS_EUNSUP, "MLM training needs vocab % 4 == 0");
    if (int r = check_device(device)) return r;
    int attn_mode = 0;
    if (const char* v = getenv("RS_TRAIN_ATTN")) {
        const std::string m(v);
        if (m == "tiled") attn_mode = 1;
        else if (m == "legacy") attn_mode = 2;
        else if (!m.empty() && m != "auto") return rs_fail(RS_EARG, "RS_TRAIN_ATTN must be auto, tiled or legacy");
    }
    rs_trainer* t = new (std::nothrow) rs_trainer();
    if (!t) return rs_fail(RS_ENOMEM, "alloc");
    t->attn_mode = attn_mode;
    t->cfg = c;
    t->device = device;
    const size_t H = c.hidden, F = c.intermediate, V = c.vocab;
    const std::string e = "bert.embeddings.";
    t->o_word = add_tensor(t, e + "word_embeddings.weight", V * H);
    t->o_pos = add_tensor(t, e + "position_embeddings.weight", (size_t)c.max_pos * H);
    t->o_type = add_tensor(t, e + "token_type_embeddings.weight", (size_t)c.type_vocab * H);
    t->o_eg = add_tensor(t, e + "LayerNorm.weight", H);
    t->o_eb = add_tensor(t, e + "LayerNorm.bias", H);
    t->lay.resize(c.layers);
    for (int i = 0; i < c.layers; ++i) {
        const std::string p = "bert.encoder.layer." + std::to_string(i) + ".";
        TLayer& L = t->lay[i];
        L.wqkv = add_tensor(t, p + "attention.self.query.weight", H * H);     // H*H % 64 == 0: contiguous
        add_tensor(t, p + "attention.self.key.weight", H * H);
        add_tensor(t, p + "attention.self.value.weight", H * H);
        L.bqkv = add_tensor(t, p + "attention.self.query.bias", H);
        add_tensor(t, p + "attention.self.key.bias", H);
        add_tensor(t, p + "attention.self.value.bias", H);
        L.wo = add_tensor(t, p + "attention.output.dense.weight", H * H);
        L.bo = add_tensor(t, p + "attention.output.dense.bias", H);
        L.g1 = add_tensor(t, p + "attention.output.LayerNorm.weight", H);
        L.be1 = add_tensor(t, p + "attention.output.LayerNorm.bias", H);
        L.w1 = add_tensor(t, p + "intermediate.dense.weight", F * H);
        L.b1 = add_tensor(t, p + "intermediate.dense.bias", F);
        L.w2 = add_tensor(t, p + "output.dense.weight", H * F);
        L.b2 = add_tensor(t, p + "output.dense.bias", H);
        L.g2 = add_tensor(t, p + "output.LayerNorm.weight", H);
        L.be2 = add_tensor(t, p + "output.LayerNorm.bias", H);
    }
    if (c.heads_mask == RS_HEAD_CLS) {
        t->o_wl = add_tensor(t, "linear.weight", H);
        t->o_bl = add_tensor(t, "linear.bias", 1);
    } else {
        const std::string p = "cls.predictions.";
        t->o_wt = add_tensor(t, p + "transform.dense.weight", H * H);
        t->o_bt = add_tensor(t, p + "transform.dense.bias", H);
        t->o_tg = add_tensor(t, p + "transform.LayerNorm.weight", H);
        t->o_tb = add_tensor(t, p + "transform.LayerNorm.bias", H);
        t->o_db = add_tensor(t, p + "bias", V);
    }
    t->n_params = (t->n_params + 63) / 64 * 64;
    t->host.assign(t->n_params, 0.0f);
    t->set.assign(t->table.size(), 0);
    merge_ranges(t);
    *out = t;
    return RS_OK;
}

int rs_trainer_set_tensor(rs_trainer* t, const char* key, const void* host_ptr, int dtype, const int64_t* shape,
                          int ndim) {
    if (!t || !key || !host_ptr || (ndim > 0 && !shape)) return rs_fail(RS_EARG, "null argument");
    if (dtype != RS_DT_F32) return rs_fail(RS_EUNSUP, "only float32 tensors are accepted");
    if (t->finalized) return rs_fail(RS_ESTATE, "trainer already finalized");
    const std::string k(key);
    if (k.rfind("bert.pooler.", 0) == 0) return RS_OK;   // RescoreBert never uses the pooler output: no gradient
    // tied to the word embeddings / to cls.predictions.bias (BertForMaskedLM._tied_weights_keys)
    if (k == "cls.predictions.decoder.weight" || k == "cls.predictions.decoder.bias") return RS_OK;
    auto it = t->table.find(k);
    if (it == t->table.end()) return rs_fail(RS_EARG, "unknown tensor " + k);
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    if ((size_t)n != it->second.second) return rs_fail(RS_EARG, "tensor " + k + " has the wrong size");
    std::memcpy(t->host.data() + it->second.first, host_ptr, (size_t)n * 4);
    t->set[std::distance(t->table.begin(), it)] = 1;
    return RS_OK;
}

int rs_trainer_finalize(rs_trainer* t) {
    if (!t) return rs_fail(RS_EARG, "null trainer");
    if (t->finalized) return RS_OK;
    size_t i = 0;
    for (auto& kv : t->table) {
        if (!t->set[i++]) return rs_fail(RS_ESTATE, "tensor " + kv.first + " (missing)");
    }
    TRY_HIP(hipSetDevice(t->device));
    const size_t bytes = t->n_params * 4;
    TRY_HIP(t->P.ensure(bytes));
    TRY_HIP(t->G.ensure(bytes));
    TRY_HIP(t->M1.ensure(bytes));
    TRY_HIP(t->V1.ensure(bytes));
    TRY_HIP(hipMemcpy(t->P.p, t->host.data(), bytes, hipMemcpyHostToDevice));
    TRY_HIP(hipMemset(t->G.p, 0, bytes));
    TRY_HIP(hipMemset(t->M1.p, 0, bytes));
    TRY_HIP(hipMemset(t->V1.p, 0, bytes));
    TRY_BLAS(rocblas_create_handle(&t->blas));
    TRY_BLAS(rocblas_set_atomics_mode(t->blas, rocblas_atomics_not_allowed));
    {
        const char* v = getenv("RS_TRAIN_ROCBLAS");
        t->use_rocblas = v && v[0] == '1';
    }
    t->host.clear();
    t->host.shrink_to_fit();
    t->finalized = true;
    return RS_OK;
}

static int copy_out(rs_trainer* t, const DevBuf& b, const char* key, void* host_out, int64_t numel) {
    if (!t || !key || !host_out) return rs_fail(RS_EARG, "null argument");
    if (!t->finalized) return rs_fail(RS_ESTATE, "rs_trainer_finalize not called");
    auto it = t->table.find(key);
    if (it == t->table.end()) return rs_fail(RS_EARG, std::string("unknown tensor ") + key);
    if ((size_t)numel != it->second.second) return rs_fail(RS_EARG, std::string("tensor ") + key + " has a different size");
    TRY_HIP(hipSetDevice(t->device));
    TRY_HIP(hipDeviceSynchronize());
    TRY_HIP(hipMemcpy(host_out, b.as<float>() + it->second.first, (size_t)numel * 4, hipMemcpyDeviceToHost));
    return RS_OK;
}

int rs_trainer_get_tensor(rs_trainer* t, const char* key, void* host_out, int64_t numel) {
    return copy_out(t, t ? t->P : DevBuf{}, key, host_out, numel);
}

// torch's .grad of a requires_grad = False tensor is None
static int check_not_frozen(rs_trainer* t, const char* key) {
    if (!t || !key) return RS_OK;                // copy_out reports it
    auto it = t->table.find(key);
    if (it != t->table.end() && !t->on(it->second.first))
        return rs_fail(RS_ESTATE, std::string("tensor ") + key + " is frozen: it has no gradient");
    return RS_OK;
}

int rs_trainer_get_grad(rs_trainer* t, const char* key, void* host_out, int64_t numel) {
    if (int r = check_not_frozen(t, key)) return r;
    return copy_out(t, t ? t->G : DevBuf{}, key, host_out, numel);
}

int rs_trainer_get_accum(rs_trainer* t, const char* key, void* host_out, int64_t numel) {
    if (int r = check_not_frozen(t, key)) return r;
    if (t && !t->acc_filled) return rs_fail(RS_ESTATE, "the accumulator is empty");
    return copy_out(t, t ? t->A : DevBuf{}, key, host_out, numel);
}

}  // extern "C"

namespace {

// One step's ragged batch: metadata on the device, saved activations, gradient scratch.
struct StepCtx {
    rs_trainer* t;
    hipStream_t st;
    int M = 0, S = 0, tmax = 0, n_uniq = 0;
    const int* dm = nullptr;
    const long long* pofs = nullptr;
    const int* seq = nullptr;
    size_t i_tok = 0, i_pos = 0, i_aux = 0, i_utok = 0, i_toff = 0, i_ord = 0, i_klen = 0;
    size_t i_type = 0;              // row types column (0: the step has no segment ids)
    // labelled-row MLM head (rs_train_step_mlm_labeled): R head rows, their row indices and the
    // inverse map (row -> compact index, -1: unlabelled) as metadata columns; R == M without
    int R = 0;
    size_t i_lrow = 0, i_linv = 0;
    const int* row_type() const { return i_type ? dm + i_type : nullptr; }
    float* x0 = nullptr;
    float2* st0 = nullptr;
    struct LA { float *hin, *qkv, *P, *ctx, *x1, *h1, *pre, *act, *x2; float2 *st1, *st2; };
    std::vector<LA> la;
    float *dA = nullptr, *dB = nullptr, *dQKV = nullptr, *dF = nullptr, *part = nullptr, *tail = nullptr;
    bool tiled = false;             // attention form of this step (whole batch, one launch)
    float* dS = nullptr;            // tiled backward: dS of one layer, the saved-P layout
    // MLM head (RS_HEAD_MLM): transform pre-GELU / GELU out (pre-LN) / LN out, stats, logits
    float *tpre = nullptr, *tx = nullptr, *th = nullptr, *logits = nullptr;
    float* hc = nullptr;            // labelled rows of the final hidden state, compact [R, H]
    float2* tst = nullptr;
    // dropout of this step (train mode: update >= 0 and p > 0)
    uint32_t seed = 0, th_hidden = 0, th_attn = 0;
    uint64_t dstep = 0;
    float sc_hidden = 1.f, sc_attn = 1.f;
    TrDrop drop(uint32_t site, bool attn) const {
        TrDrop d;
        d.seed = seed;
        d.step = (uint32_t)dstep;
        d.step_hi = (uint32_t)(dstep >> 32);
        d.site = site;
        d.thresh = attn ? th_attn : th_hidden;
        d.scale = attn ? sc_attn : sc_hidden;
        return d;
    }
};

// A training step takes the segment ids left by rs_trainer_set_token_types and drops the setting
// when it returns, whatever it returns (the scorer's PendingTypes).
struct TypeStep {
    rs_trainer* t;
    const int32_t* d_type = nullptr;
    int64_t n = 0;
    explicit TypeStep(rs_trainer* t_) : t(t_) {
        if (t) { d_type = t->type_next; n = t->type_n; }
    }
    ~TypeStep() {
        if (t) { t->type_next = nullptr; t->type_n = 0; }
    }
};

uint32_t drop_thresh(float p) { return p <= 0.f ? 0u : (uint32_t)std::min(4294967295.0, (double)p * 4294967296.0); }

// train mode (the reference's model.train() under grad_update) with p > 0: this step's key
int set_dropout(StepCtx& c, const rs_train_opts* o) {
    if (!(o->hidden_dropout >= 0.f && o->hidden_dropout < 1.f && o->attn_dropout >= 0.f && o->attn_dropout < 1.f))
        return rs_fail(RS_EARG, "dropout probabilities must be in [0, 1)");
    if (o->update < 0 || (o->hidden_dropout == 0.f && o->attn_dropout == 0.f)) return RS_OK;   // eval mode
    c.seed = o->dropout_seed;
    c.dstep = c.t->drop_step++;
    c.th_hidden = drop_thresh(o->hidden_dropout);
    c.th_attn = drop_thresh(o->attn_dropout);
    c.sc_hidden = (float)(1.0 / (1.0 - (double)o->hidden_dropout));
    c.sc_attn = (float)(1.0 / (1.0 - (double)o->attn_dropout));
    return RS_OK;
}

// host metadata + buffers.  aux: extra int32 array uploaded with the metadata (utt_off);
// h_klen (nullable): per-sequence key lengths (padded-batch rows, rs_train_step_mlm).
// ty: the step's segment ids (d_type null: none), one per token row.
// h_lab (nullable): the n_lab token rows the MLM head runs on, strictly ascending in [0, M) (checked
// by rs_train_step_mlm_labeled before any trainer state moves, and again here, next to the offsets
// that define M, before anything is sized or uploaded from the list); the head
// regions are then sized by n_lab and one more holds the gathered hidden rows.  Without it the head
// has all M rows and the layout is the one rs_train_step_mlm always had.
int prepare(StepCtx& c, const TypeStep& ty, const int32_t* d_tok, const int32_t* h_off, int n_seq,
            const std::vector<int>& aux, const int32_t* h_klen = nullptr, const int32_t* h_lab = nullptr,
            int n_lab = 0) {
    rs_trainer* t = c.t;
    const rs_bert_cfg& cf = t->cfg;
    const int H = cf.hidden, F = cf.intermediate, nh = cf.heads, NL = cf.layers;
    if (n_seq <= 0 || h_off[0] != 0) return rs_fail(RS_EARG, "empty batch or offsets not starting at 0");
    c.S = n_seq;
    c.M = h_off[n_seq];
    if (ty.d_type && ty.n != c.M)
        return rs_fail(RS_EARG, "rs_trainer_set_token_types gave " + std::to_string(ty.n) +
                                    " token types, this step addresses " + std::to_string(c.M) + " tokens");
    for (int s = 0; s < n_seq; ++s) {
        const int T = h_off[s + 1] - h_off[s];
        if (T < 1) return rs_fail(RS_EARG, "empty sequence");
        c.tmax = std::max(c.tmax, T);
    }
    if (c.tmax > cf.max_pos) return rs_fail(RS_EUNSUP, "sequence longer than max_position_embeddings");
    // attention form: the whole-head kernels hold K, V and dS of a head in LDS (T <= 128); a batch
    // with a longer sequence runs the tiled kernels for every sequence in it
    c.tiled = t->attn_mode == 1 || (t->attn_mode == 0 && c.tmax > 128);
    if (!c.tiled && c.tmax > 128)
        return rs_fail(RS_EUNSUP, "training sequences are limited to 128 tokens (RS_TRAIN_ATTN=legacy)");
    if (h_klen)
        for (int s = 0; s < n_seq; ++s)
            if (h_klen[s] < 1 || h_klen[s] > h_off[s + 1] - h_off[s])
                return rs_fail(RS_EARG, "key length outside 1..row length");
    const int M = c.M, S = c.S;
    c.R = h_lab ? n_lab : M;
    for (int k = 0; k < (h_lab ? n_lab : 0); ++k) {
        if (h_lab[k] < 0 || h_lab[k] >= M)
            return rs_fail(RS_EARG, "h_lab_row[" + std::to_string(k) + "] = " + std::to_string(h_lab[k]) +
                                        " is outside the batch's " + std::to_string(M) + " token rows");
        if (k && h_lab[k] <= h_lab[k - 1])
            return rs_fail(RS_EARG, "h_lab_row[" + std::to_string(k) + "] = " + std::to_string(h_lab[k]) +
                                        " is not above h_lab_row[" + std::to_string(k - 1) + "] = " +
                                        std::to_string(h_lab[k - 1]) + " (strictly ascending rows)");
    }
    hipStream_t st = c.st;
    TRY_HIP(hipSetDevice(t->device));
    TRY_BLAS(rocblas_set_stream(t->blas, st));
    t->h_tok.resize(M);
    TRY_HIP(hipMemcpyAsync(t->h_tok.data(), d_tok, (size_t)M * 4, hipMemcpyDeviceToHost, st));
    t->h_type.resize(ty.d_type ? M : 0);
    if (ty.d_type) TRY_HIP(hipMemcpyAsync(t->h_type.data(), ty.d_type, (size_t)M * 4, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    for (int& k : t->h_type) k = std::min(std::max(k, 0), cf.type_vocab - 1);   // clamped like token ids
    std::vector<int> row_pos(M), order(M);
    for (int s = 0; s < S; ++s)
        for (int r = h_off[s]; r < h_off[s + 1]; ++r) row_pos[r] = r - h_off[s];
    for (int r = 0; r < M; ++r) {
        order[r] = r;
        t->h_tok[r] = std::min(std::max(t->h_tok[r], 0), cf.vocab - 1);
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return t->h_tok[a] < t->h_tok[b]; });
    std::vector<int> utok, toff;
    for (int k = 0; k < M; ++k)
        if (k == 0 || t->h_tok[order[k]] != t->h_tok[order[k - 1]]) {
            utok.push_back(t->h_tok[order[k]]);
            toff.push_back(k);
        }
    toff.push_back(M);
    c.n_uniq = (int)utok.size();
    std::vector<long long> pofs(S + 1, 0);
    for (int s = 0; s < S; ++s) {
        const long long T = h_off[s + 1] - h_off[s];
        pofs[s + 1] = pofs[s] + (long long)nh * T * T;
    }
    // int layout: pofs (int64) | row_tok | row_pos | seq_off | aux | utok | toff | order | klen | row_type
    //             | lab_row | lab_inv
    std::vector<int>& hm = t->h_meta;
    hm.assign(2 * (S + 1), 0);
    std::memcpy(hm.data(), pofs.data(), (S + 1) * 8);
    c.i_tok = hm.size();
    hm.insert(hm.end(), t->h_tok.begin(), t->h_tok.end());
    c.i_pos = hm.size();
    hm.insert(hm.end(), row_pos.begin(), row_pos.end());
    const size_t i_seq = hm.size();
    hm.insert(hm.end(), h_off, h_off + S + 1);
    c.i_aux = hm.size();
    hm.insert(hm.end(), aux.begin(), aux.end());
    c.i_utok = hm.size();
    hm.insert(hm.end(), utok.begin(), utok.end());
    c.i_toff = hm.size();
    hm.insert(hm.end(), toff.begin(), toff.end());
    c.i_ord = hm.size();
    hm.insert(hm.end(), order.begin(), order.end());
    c.i_klen = 0;
    if (h_klen) {
        c.i_klen = hm.size();
        hm.insert(hm.end(), h_klen, h_klen + S);
    }
    c.i_type = 0;
    if (ty.d_type) {
        c.i_type = hm.size();
        hm.insert(hm.end(), t->h_type.begin(), t->h_type.end());
    }
    c.i_lrow = c.i_linv = 0;
    if (h_lab) {
        c.i_lrow = hm.size();
        hm.insert(hm.end(), h_lab, h_lab + n_lab);
        c.i_linv = hm.size();
        hm.insert(hm.end(), (size_t)M, -1);
        for (int k = 0; k < n_lab; ++k) hm[c.i_linv + h_lab[k]] = k;
    }
    TRY_ALLOC(t->meta.ensure(hm.size() * 4));
    TRY_HIP(hipMemcpyAsync(t->meta.p, hm.data(), hm.size() * 4, hipMemcpyHostToDevice, st));
    c.dm = (const int*)t->meta.p;
    c.pofs = (const long long*)c.dm;
    c.seq = c.dm + i_seq;

    const bool mlm = cf.heads_mask == RS_HEAD_MLM;
    // every region starts on a 256-byte boundary (an odd row count M would otherwise leave the
    // tensors after the float2 statistics 8-byte aligned under float4 accesses and rocBLAS)
    auto al = [](size_t n) { return (n + 63) & ~(size_t)63; };
    const size_t MH = al((size_t)M * H), MF = al((size_t)M * F), M2 = al((size_t)M * 2), PS = al((size_t)pofs[S]);
    const size_t QKV = al((size_t)M * 3 * H);
    // the MLM head's regions by its own row count R (R == M: the sizes they always had)
    const int R = c.R;
    const size_t RH = al((size_t)R * H), R2 = al((size_t)R * 2), RV = mlm ? al((size_t)R * cf.vocab) : 0;
    const size_t per_layer = MH + QKV + PS + MH + MH + M2 + MH + 2 * MF + MH + M2;
    const size_t n_head = mlm ? 3 * RH + R2 + RV + (h_lab ? RH : 0) : 0;
    const size_t n_act = MH + M2 + NL * per_layer + MH + n_head;
    TRY_ALLOC(t->act.ensure(n_act * 4));
    const int widest = std::max(std::max(3 * H, F), mlm ? cf.vocab : 0);
    const size_t n_part = al(tr_colsum_scratch(M, widest) / 4);   // grows with the rows: covers the head's R <= M
    const size_t n_tail = al(2 * (size_t)S + aux.size() + M + 64);
    const size_t n_grad = 2 * MH + QKV + MF + n_part + n_tail + (c.tiled ? PS : 0);
    TRY_ALLOC(t->grad.ensure(n_grad * 4));
    // the picker may split K differently at the head's R rows: its (R, V, H) shapes sized too
    size_t n_ws = sgemm_ws_floats(cf, M);
    if (R != M) n_ws = std::max(n_ws, sgemm_ws_floats(cf, R));
    TRY_ALLOC(t->ws.ensure(std::max<size_t>(n_ws, 64) * 4));
    float* A = t->act.as<float>();
    c.x0 = A;
    c.st0 = (float2*)(c.x0 + MH);
    float* lbase = c.x0 + MH + M2;
    c.la.assign(NL + 1, StepCtx::LA{});
    for (int l = 0; l <= NL; ++l) {
        float* b = lbase + (size_t)l * per_layer;
        StepCtx::LA& a = c.la[l];
        a.hin = b;
        if (l == NL) break;
        a.qkv = b + MH;
        a.P = a.qkv + QKV;
        a.ctx = a.P + PS;
        a.x1 = a.ctx + MH;
        a.st1 = (float2*)(a.x1 + MH);
        a.h1 = a.x1 + MH + M2;
        a.pre = a.h1 + MH;
        a.act = a.pre + MF;
        a.x2 = a.act + MF;
        a.st2 = (float2*)(a.x2 + MH);
    }
    if (mlm) {
        c.tpre = c.la[NL].hin + MH;
        c.tx = c.tpre + RH;
        c.th = c.tx + RH;
        c.tst = (float2*)(c.th + RH);
        c.logits = c.th + RH + R2;
        c.hc = h_lab ? c.logits + RV : nullptr;
    }
    float* G = t->grad.as<float>();
    c.dA = G;
    c.dB = c.dA + MH;
    c.dQKV = c.dB + MH;
    c.dF = c.dQKV + QKV;
    c.part = c.dF + MF;
    c.tail = c.part + n_part;        // per-sequence / per-row small arrays
    c.dS = c.tiled ? c.tail + n_tail : nullptr;
    return RS_OK;
}

int encoder_forward(StepCtx& c) {
    rs_trainer* t = c.t;
    const rs_bert_cfg& cf = t->cfg;
    const int H = cf.hidden, F = cf.intermediate, nh = cf.heads, M = c.M;
    float* Pm = t->P.as<float>();
    hipStream_t st = c.st;
    TRY_HIP(tr_embed_ln(c.dm + c.i_tok, c.dm + c.i_pos, c.row_type(), M, cf.vocab, cf.type_vocab, Pm + t->o_word,
                        Pm + t->o_pos, Pm + t->o_type, Pm + t->o_eg, Pm + t->o_eb, cf.ln_eps, H, c.x0, c.st0, c.la[0].hin,
                        st, c.drop(0, false)));
    for (int l = 0; l < cf.layers; ++l) {
        const TLayer& L = t->lay[l];
        StepCtx::LA& a = c.la[l];
        RS_TRY(gemm_nt(t, st, M, 3 * H, H, a.hin, Pm + L.wqkv, a.qkv, 0.f));
        TRY_HIP(tr_bias(a.qkv, Pm + L.bqkv, M, 3 * H, st));
        const int* klen = c.i_klen ? c.dm + c.i_klen : nullptr;
        if (c.tiled)
            TRY_HIP(tr_attn_fwd_tiled(a.qkv, c.seq, klen, c.pofs, c.S, c.tmax, H, nh, a.P, a.ctx, st,
                                      c.drop(1 + 3 * l, true)));
        else
            TRY_HIP(tr_attn_fwd(a.qkv, c.seq, klen, c.pofs, c.S, c.tmax, H, nh, a.P, a.ctx, st,
                                c.drop(1 + 3 * l, true)));
        RS_TRY(gemm_nt(t, st, M, H, H, a.ctx, Pm + L.wo, a.x1, 0.f));
        TRY_HIP(tr_bias_res_ln(a.x1, Pm + L.bo, a.hin, M, Pm + L.g1, Pm + L.be1, cf.ln_eps, H, a.st1, a.h1, st,
                               c.drop(2 + 3 * l, false)));
        RS_TRY(gemm_nt(t, st, M, F, H, a.h1, Pm + L.w1, a.pre, 0.f));
        TRY_HIP(tr_bias_gelu(a.pre, Pm + L.b1, a.act, M, F, st));
        RS_TRY(gemm_nt(t, st, M, H, F, a.act, Pm + L.w2, a.x2, 0.f));
        TRY_HIP(tr_bias_res_ln(a.x2, Pm + L.b2, a.h1, M, Pm + L.g2, Pm + L.be2, cf.ln_eps, H, a.st2,
                               c.la[l + 1].hin, st, c.drop(3 + 3 * l, false)));
    }
    return RS_OK;
}

// What of the encoder's backward the trainable set asks for (rs_trainer_set_trainable): emb, any
// embedding tensor trainable; lo, the lowest layer with a trainable tensor (layers: none).  Layers
// below lo launch nothing unless the embeddings need the gradient carried down to them.
struct BwdPlan {
    bool emb = true;
    int lo = 0, n_layers = 0;
    bool any() const { return emb || lo < n_layers; }
};
BwdPlan bwd_plan(const rs_trainer* t) {
    BwdPlan p;
    p.n_layers = t->cfg.layers;
    if (t->frozen.empty()) return p;
    p.emb = t->on(t->o_word) || t->on(t->o_pos) || t->on(t->o_type) || t->on(t->o_eg) || t->on(t->o_eb);
    const size_t HH = (size_t)t->cfg.hidden * t->cfg.hidden, H = t->cfg.hidden;
    for (p.lo = 0; p.lo < p.n_layers; ++p.lo) {
        const TLayer& L = t->lay[p.lo];
        bool any = false;
        for (size_t o : {L.wqkv, L.wqkv + HH, L.wqkv + 2 * HH, L.bqkv, L.bqkv + H, L.bqkv + 2 * H, L.wo, L.bo, L.g1,
                         L.be1, L.w1, L.b1, L.w2, L.b2, L.g2, L.be2})
            any = any || t->on(o);
        if (any) break;
    }
    return p;
}

// from dA = d(final hidden) down to the embeddings; gradients written into t->G (zeroed by
// the caller before the head's backward).  The weight / bias / LayerNorm gradient of a frozen tensor
// is not launched (the fused Q|K|V pair runs while any of its three is trainable; a LayerNorm's
// gamma / beta pair while either is), and the chain stops where nothing below is trainable.  With
// nothing frozen every condition is true: the launches of the unpruned backward, in its order.
int encoder_backward(StepCtx& c) {
    rs_trainer* t = c.t;
    const rs_bert_cfg& cf = t->cfg;
    const int H = cf.hidden, F = cf.intermediate, nh = cf.heads, M = c.M;
    const size_t MH = (size_t)M * H, MF = (size_t)M * F;
    float *Pm = t->P.as<float>(), *Gm = t->G.as<float>();
    float *dA = c.dA, *dB = c.dB, *dF = c.dF, *dQKV = c.dQKV, *part = c.part;
    hipStream_t st = c.st;
    const BwdPlan plan = bwd_plan(t);
    const size_t HH = (size_t)H * H;
    auto on = [t](size_t off) { return t->on(off); };
    for (int l = cf.layers - 1; l >= (plan.emb ? 0 : plan.lo); --l) {
        const TLayer& L = t->lay[l];
        StepCtx::LA& a = c.la[l];
        if (on(L.g2) || on(L.be2)) TRY_HIP(tr_colsum_ln(dA, a.x2, a.st2, M, H, part, Gm + L.g2, Gm + L.be2, st));
        TRY_HIP(tr_ln_bwd(dA, a.x2, a.st2, Pm + L.g2, dB, M, H, st));              // dB = dx2
        // BertOutput dropout: the dense branch sees dx2 * mask * scale (in the free dQKV
        // buffer), the residual branch dx2 itself (dB, copied into dA below)
        const float* dBo = dB;
        if (c.th_hidden) {
            TRY_HIP(tr_dropout(dQKV, dB, (long long)MH, c.drop(3 + 3 * l, false), st));
            dBo = dQKV;
        }
        if (on(L.b2)) TRY_HIP(tr_colsum(dBo, nullptr, nullptr, M, H, 0, part, Gm + L.b2, 0, st));
        if (on(L.w2)) RS_TRY(gemm_tn(t, st, M, H, F, dBo, a.act, Gm + L.w2, 0.f));
        RS_TRY(gemm_nn(t, st, M, H, F, dBo, Pm + L.w2, dF, 0.f));                   // d act
        TRY_HIP(tr_gelu_bwd(dF, a.pre, (long long)MF, st));                         // d pre
        if (on(L.b1)) TRY_HIP(tr_colsum(dF, nullptr, nullptr, M, F, 0, part, Gm + L.b1, 0, st));
        if (on(L.w1)) RS_TRY(gemm_tn(t, st, M, F, H, dF, a.h1, Gm + L.w1, 0.f));
        TRY_HIP(hipMemcpyAsync(dA, dB, MH * 4, hipMemcpyDeviceToDevice, st));      // residual
        RS_TRY(gemm_nn(t, st, M, F, H, dF, Pm + L.w1, dA, 1.f));                     // dA = d h1
        if (on(L.g1) || on(L.be1)) TRY_HIP(tr_colsum_ln(dA, a.x1, a.st1, M, H, part, Gm + L.g1, Gm + L.be1, st));
        TRY_HIP(tr_ln_bwd(dA, a.x1, a.st1, Pm + L.g1, dB, M, H, st));              // dB = dx1
        // BertSelfOutput dropout: masked copy for the dense branch in the free dF buffer
        const float* dBs = dB;
        if (c.th_hidden) {
            TRY_HIP(tr_dropout(dF, dB, (long long)MH, c.drop(2 + 3 * l, false), st));
            dBs = dF;
        }
        if (on(L.bo)) TRY_HIP(tr_colsum(dBs, nullptr, nullptr, M, H, 0, part, Gm + L.bo, 0, st));
        if (on(L.wo)) RS_TRY(gemm_tn(t, st, M, H, H, dBs, a.ctx, Gm + L.wo, 0.f));
        RS_TRY(gemm_nn(t, st, M, H, H, dBs, Pm + L.wo, dA, 0.f));                    // dA = d ctx
        if (c.tiled)
            TRY_HIP(tr_attn_bwd_tiled(a.qkv, a.P, dA, c.seq, c.pofs, c.S, c.tmax, H, nh, c.dS, dQKV, st,
                                      c.drop(1 + 3 * l, true)));
        else
            TRY_HIP(tr_attn_bwd(a.qkv, a.P, dA, c.seq, c.pofs, c.S, c.tmax, H, nh, dQKV, st, c.drop(1 + 3 * l, true)));
        if (on(L.bqkv) || on(L.bqkv + H) || on(L.bqkv + 2 * H))
            TRY_HIP(tr_colsum(dQKV, nullptr, nullptr, M, 3 * H, 0, part, Gm + L.bqkv, 0, st));
        if (on(L.wqkv) || on(L.wqkv + HH) || on(L.wqkv + 2 * HH))
            RS_TRY(gemm_tn(t, st, M, 3 * H, H, dQKV, a.hin, Gm + L.wqkv, 0.f));
        if (!plan.emb && l == plan.lo) break;           // nothing below takes the layer's input gradient
        TRY_HIP(hipMemcpyAsync(dA, dB, MH * 4, hipMemcpyDeviceToDevice, st));      // residual
        RS_TRY(gemm_nn(t, st, M, 3 * H, H, dQKV, Pm + L.wqkv, dA, 1.f));             // dA = d h_in
    }
    if (!plan.emb) return RS_OK;
    // embedding dropout: d(LN output) = d h0 * mask * scale
    if (c.th_hidden) TRY_HIP(tr_dropout(dA, dA, (long long)MH, c.drop(0, false), st));
    if (on(t->o_eg) || on(t->o_eb))
        TRY_HIP(tr_colsum_ln(dA, c.x0, c.st0, M, H, part, Gm + t->o_eg, Gm + t->o_eb, st));
    if (!(on(t->o_word) || on(t->o_pos) || on(t->o_type))) return RS_OK;
    TRY_HIP(tr_ln_bwd(dA, c.x0, c.st0, Pm + t->o_eg, dB, M, H, st));                // dB = dx0
    // word embeddings: += (the tied MLM decoder already wrote its part)
    if (on(t->o_word))
        TRY_HIP(tr_word_grad(dB, c.dm + c.i_utok, c.dm + c.i_toff, c.dm + c.i_ord, c.n_uniq, H, Gm + t->o_word, st));
    if (on(t->o_pos)) TRY_HIP(tr_pos_grad(dB, c.seq, c.S, c.tmax, H, Gm + t->o_pos, st));
    if (!on(t->o_type)) return RS_OK;
    // token types: without segment ids every row into row 0 (the other rows stay 0 from the step's
    // memset); with them, row k from the rows of type k, one predicated pass per type
    if (!c.row_type())
        TRY_HIP(tr_colsum(dB, nullptr, nullptr, M, H, 0, part, Gm + t->o_type, 0, st));
    else
        for (int k = 0; k < cf.type_vocab; ++k)
            TRY_HIP(tr_colsum(dB, nullptr, nullptr, M, H, 0, part, Gm + t->o_type + (size_t)k * H, 0, st, c.row_type(), k));
    return RS_OK;
}

// one AdamW step (number t->step + 1) on the gradient gmul * src over the trainable ranges: a frozen
// tensor keeps its parameter and its moments (no decay).  Nothing frozen and gmul == 1: the one
// tr_adamw launch over the whole flat vector.
int adamw_ranges(rs_trainer* t, const rs_train_opts* o, const float* src, float gmul, hipStream_t st) {
    t->step += 1;
    const TrAdamW a = tr_adamw_scalars(o->lr, o->beta1, o->beta2, o->eps, o->weight_decay, t->step);
    for (const TrRange& r : t->ranges)
        TRY_HIP(tr_adamw_scaled(t->P.as<float>() + r.off, src + r.off, t->M1.as<float>() + r.off,
                                t->V1.as<float>() + r.off, r.n, gmul, a.decay, a.b1w, a.b2, a.b2w, a.step_size,
                                a.bc2_sqrt, a.eps, st));
    return RS_OK;
}

int adamw(rs_trainer* t, const rs_train_opts* o, hipStream_t st) {
    if (o->update != 1) return RS_OK;
    return adamw_ranges(t, o, t->G.as<float>(), 1.0f, st);
}

// a step that runs a backward (update >= 0) needs something to train; raised before any state moves
int check_trainable(const rs_trainer* t, const rs_train_opts* o) {
    if (o->update >= 0 && t->ranges.empty())
        return rs_fail(RS_ESTATE, "every tensor is frozen (rs_trainer_set_trainable): nothing to compute a gradient for");
    return RS_OK;
}

}  // namespace

extern "C" {

int rs_train_step_cls(rs_trainer* t, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                      const int32_t* h_utt_off, int32_t n_utt, const float* d_target, const float* d_am,
                      const float* d_err, const rs_train_opts* o, float* d_scores, float* d_loss, void* stream) {
    TypeStep ty(t);
    if (!t || !h_hyp_off || !h_utt_off || !o || !d_loss || n_hyp <= 0 || n_utt <= 0 || !d_tok || !d_target)
        return rs_fail(RS_EARG, "null argument / empty batch");
    if (!t->finalized) return rs_fail(RS_ESTATE, "rs_trainer_finalize not called");
    if (t->cfg.heads_mask != RS_HEAD_CLS) return rs_fail(RS_ESTATE, "trainer has no RescoreBert head");
    if (o->loss < RS_LOSS_MD || o->loss > RS_LOSS_MWED) return rs_fail(RS_EARG, "unknown loss");
    if (o->loss != RS_LOSS_MD && (!d_am || !d_err)) return rs_fail(RS_EARG, "MWER/MWED need am scores and errors");
    if (h_utt_off[0] != 0 || h_utt_off[n_utt] != n_hyp) return rs_fail(RS_EARG, "utt_off must span 0..n_hyp");
    for (int u = 0; u < n_utt; ++u)
        if (h_utt_off[u + 1] < h_utt_off[u]) return rs_fail(RS_EARG, "utt_off not ascending");
    if (int r = check_trainable(t, o)) return r;
    StepCtx c;
    c.t = t;
    c.st = (hipStream_t)stream;
    if (int r = set_dropout(c, o)) return r;
    if (int r = prepare(c, ty, d_tok, h_hyp_off, n_hyp, std::vector<int>(h_utt_off, h_utt_off + n_utt + 1))) return r;
    if (int r = encoder_forward(c)) return r;
    const int H = t->cfg.hidden, S = c.S;
    float *Pm = t->P.as<float>(), *Gm = t->G.as<float>();
    float* sc = c.tail;
    float* dsc = sc + S;
    float* uloss = dsc + S;
    const float* hfin = c.la[t->cfg.layers].hin;
    hipStream_t st = c.st;
    TRY_HIP(tr_cls_fwd(hfin, c.seq, S, H, Pm + t->o_wl, Pm + t->o_bl, sc, st));
    if (d_scores) TRY_HIP(hipMemcpyAsync(d_scores, sc, (size_t)S * 4, hipMemcpyDeviceToDevice, st));
    TRY_HIP(tr_loss(sc, d_target, d_am, d_err, c.dm + c.i_aux, n_utt, S, o->loss, o->md_loss_weight, dsc, uloss,
                    d_loss, st));
    if (o->update < 0) {                      // loss only (the reference's dev pass)
        TRY_HIP(hipStreamSynchronize(st));
        return RS_OK;
    }
    t->have_grad = false;
    TRY_HIP(hipMemsetAsync(Gm, 0, t->n_params * 4, st));
    TRY_HIP(hipMemsetAsync(c.dA, 0, (size_t)c.M * H * 4, st));
    TRY_HIP(tr_cls_bwd(dsc, hfin, c.seq, S, H, Pm + t->o_wl, c.dA, Gm + t->o_wl, Gm + t->o_bl, st));
    if (int r = encoder_backward(c)) return r;
    if (int r = adamw(t, o, st)) return r;
    TRY_HIP(hipStreamSynchronize(st));        // the metadata upload read t->h_meta
    if (tr_sgemm_failed()) return rs_fail(RS_EHIP, "a stream-K GEMM timed out waiting for a partial tile");
    t->have_grad = true;
    return RS_OK;
}

// The MLM step behind both entries.  h_lab null: the head over all M rows (rs_train_step_mlm, one
// label per row).  Otherwise over the n_lab rows h_lab names: their final hidden rows gathered into
// c.hc, the same head sequence on n_lab rows (CE mean over n_lab), and the head's gradient w.r.t.
// the hidden state expanded back to [M, H] with zeros at the unlabelled rows.
static int mlm_step(rs_trainer* t, const TypeStep& ty, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                    const int32_t* h_key_len, const int32_t* h_lab, int32_t n_lab, const int32_t* d_labels,
                    const rs_train_opts* o, float* d_loss, void* stream) {
    if (int r = check_trainable(t, o)) return r;
    StepCtx c;
    c.t = t;
    c.st = (hipStream_t)stream;
    if (int r = set_dropout(c, o)) return r;
    if (int r = prepare(c, ty, d_ids, h_seq_off, n_seq, {}, h_key_len, h_lab, n_lab)) return r;
    if (int r = encoder_forward(c)) return r;
    const rs_bert_cfg& cf = t->cfg;
    const int H = cf.hidden, V = cf.vocab, M = c.M, R = c.R;
    float *Pm = t->P.as<float>(), *Gm = t->G.as<float>();
    hipStream_t st = c.st;
    const float* hfin = c.la[cf.layers].hin;
    if (h_lab) {
        TRY_HIP(tr_gather_rows(hfin, c.dm + c.i_lrow, R, H, c.hc, st));
        hfin = c.hc;
    }
    // BertOnlyMLMHead: transform (dense + GELU + LN), tied decoder + bias (modeling_bert.py:466-506)
    RS_TRY(gemm_nt(t, st, R, H, H, hfin, Pm + t->o_wt, c.tpre, 0.f));
    TRY_HIP(tr_bias_gelu(c.tpre, Pm + t->o_bt, c.tx, R, H, st));
    TRY_HIP(tr_bias_res_ln(c.tx, nullptr, nullptr, R, Pm + t->o_tg, Pm + t->o_tb, cf.ln_eps, H, c.tst, c.th, st));
    RS_TRY(gemm_nt(t, st, R, V, H, c.th, Pm + t->o_word, c.logits, 0.f));
    TRY_HIP(tr_bias(c.logits, Pm + t->o_db, R, V, st));
    float* rl = c.tail;
    TRY_HIP(tr_ce(c.logits, d_labels, R, V, rl, d_loss, st));       // logits <- dlogits
    if (o->update < 0) {                      // loss only (the reference's dev pass)
        TRY_HIP(hipStreamSynchronize(st));
        return RS_OK;
    }
    t->have_grad = false;
    TRY_HIP(hipMemsetAsync(Gm, 0, t->n_params * 4, st));
    float* dT = c.dB;
    float* dT2 = c.dF;
    // a frozen tensor's gradient is not launched (the tied decoder's part of the word embeddings with them)
    if (t->on(t->o_db)) TRY_HIP(tr_colsum(c.logits, nullptr, nullptr, R, V, 0, c.part, Gm + t->o_db, 0, st));
    if (t->on(t->o_word)) RS_TRY(gemm_tn(t, st, R, V, H, c.logits, c.th, Gm + t->o_word, 0.f));   // tied decoder part
    RS_TRY(gemm_nn(t, st, R, V, H, c.logits, Pm + t->o_word, dT, 0.f));
    if (t->on(t->o_tg) || t->on(t->o_tb))
        TRY_HIP(tr_colsum_ln(dT, c.tx, c.tst, R, H, c.part, Gm + t->o_tg, Gm + t->o_tb, st));
    TRY_HIP(tr_ln_bwd(dT, c.tx, c.tst, Pm + t->o_tg, dT2, R, H, st));
    TRY_HIP(tr_gelu_bwd(dT2, c.tpre, (long long)R * H, st));
    if (t->on(t->o_bt)) TRY_HIP(tr_colsum(dT2, nullptr, nullptr, R, H, 0, c.part, Gm + t->o_bt, 0, st));
    if (t->on(t->o_wt)) RS_TRY(gemm_tn(t, st, R, H, H, dT2, hfin, Gm + t->o_wt, 0.f));
    if (!bwd_plan(t).any()) {
        // only the head is trainable: nothing takes the gradient of the hidden state
    } else if (h_lab) {
        // d hidden of the labelled rows into dT (free since tr_ln_bwd), then every row of dA
        RS_TRY(gemm_nn(t, st, R, H, H, dT2, Pm + t->o_wt, dT, 0.f));
        TRY_HIP(tr_expand_rows(dT, c.dm + c.i_linv, M, H, c.dA, st));
    } else {
        RS_TRY(gemm_nn(t, st, M, H, H, dT2, Pm + t->o_wt, c.dA, 0.f));              // dA = d hidden
    }
    if (int r = encoder_backward(c)) return r;
    if (int r = adamw(t, o, st)) return r;
    TRY_HIP(hipStreamSynchronize(st));
    if (tr_sgemm_failed()) return rs_fail(RS_EHIP, "a stream-K GEMM timed out waiting for a partial tile");
    t->have_grad = true;
    return RS_OK;
}

int rs_train_step_mlm(rs_trainer* t, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                      const int32_t* h_key_len, const int32_t* d_labels, const rs_train_opts* o, float* d_loss,
                      void* stream) {
    TypeStep ty(t);
    if (!t || !h_seq_off || !o || !d_loss || n_seq <= 0 || !d_ids || !d_labels)
        return rs_fail(RS_EARG, "null argument / empty batch");
    if (!t->finalized) return rs_fail(RS_ESTATE, "rs_trainer_finalize not called");
    if (t->cfg.heads_mask != RS_HEAD_MLM) return rs_fail(RS_ESTATE, "trainer has no MLM head");
    return mlm_step(t, ty, d_ids, h_seq_off, n_seq, h_key_len, nullptr, 0, d_labels, o, d_loss, stream);
}

int rs_train_step_mlm_labeled(rs_trainer* t, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                              const int32_t* h_key_len, const int32_t* h_lab_row, int32_t n_lab,
                              const int32_t* d_lab_id, const rs_train_opts* o, float* d_loss, void* stream) {
    TypeStep ty(t);
    if (!t || !h_seq_off || !o || !d_loss || n_seq <= 0 || !d_ids)
        return rs_fail(RS_EARG, "null argument / empty batch");
    if (!t->finalized) return rs_fail(RS_ESTATE, "rs_trainer_finalize not called");
    if (t->cfg.heads_mask != RS_HEAD_MLM) return rs_fail(RS_ESTATE, "trainer has no MLM head");
    if (n_lab <= 0)
        return rs_fail(RS_EARG, "n_lab = " + std::to_string(n_lab) + ": a labelled step needs at least one labelled row");
    if (!h_lab_row || !d_lab_id) return rs_fail(RS_EARG, "null label rows / label ids");
    // the row list against the batch's M rows, before the dropout-step counter or anything else moves
    const int M = h_seq_off[n_seq];
    for (int k = 0; k < n_lab; ++k) {
        if (h_lab_row[k] < 0 || h_lab_row[k] >= M)
            return rs_fail(RS_EARG, "h_lab_row[" + std::to_string(k) + "] = " + std::to_string(h_lab_row[k]) +
                                        " is outside the batch's " + std::to_string(M) + " token rows");
        if (k && h_lab_row[k] <= h_lab_row[k - 1])
            return rs_fail(RS_EARG, "h_lab_row[" + std::to_string(k) + "] = " + std::to_string(h_lab_row[k]) +
                                        " is not above h_lab_row[" + std::to_string(k - 1) + "] = " +
                                        std::to_string(h_lab_row[k - 1]) + " (strictly ascending rows)");
    }
    return mlm_step(t, ty, d_ids, h_seq_off, n_seq, h_key_len, h_lab_row, n_lab, d_lab_id, o, d_loss, stream);
}

}  // extern "C"

namespace {

// HF aliases of one Parameter (BertForMaskedLM ties the decoder to the word embeddings and to
// cls.predictions.bias): the key the trainer's table holds
std::string table_key(const rs_trainer* t, const std::string& k) {
    if (t->cfg.heads_mask == RS_HEAD_MLM) {
        if (k == "cls.predictions.decoder.weight") return "bert.embeddings.word_embeddings.weight";
        if (k == "cls.predictions.decoder.bias") return "cls.predictions.bias";
    }
    return k;
}

// whole dotted components: the key is the prefix, or starts with prefix + "."
bool prefix_matches(const std::string& key, const std::string& prefix) {
    return key.compare(0, prefix.size(), prefix) == 0 && (key.size() == prefix.size() || key[prefix.size()] == '.');
}

int clear_accum(rs_trainer* t, hipStream_t st) {
    if (t->A.p) TRY_HIP(hipMemsetAsync(t->A.p, 0, t->n_params * 4, st));
    t->acc_filled = false;
    return RS_OK;
}

// the gradient source of rs_trainer_apply / rs_trainer_grad_norm
int grad_source(rs_trainer* t, int32_t source, const float** src) {
    if (source != 0 && source != 1)
        return rs_fail(RS_EARG, "source must be 0 (the last step's gradient) or 1 (the accumulator)");
    if (source == 0 && !t->have_grad)
        return rs_fail(RS_ESTATE, "no gradient: no backward has run (since the trainable set last changed)");
    if (source == 1 && !t->acc_filled) return rs_fail(RS_ESTATE, "the accumulator is empty");
    if (t->ranges.empty()) return rs_fail(RS_ESTATE, "every tensor is frozen");
    *src = source == 0 ? t->G.as<float>() : t->A.as<float>();
    return RS_OK;
}

// sqrt of the ordered float64 sum of squares over the trainable ranges; synchronises the stream
int grad_norm(rs_trainer* t, const float* src, double* norm, hipStream_t st) {
    TRY_ALLOC(t->nws.ensure(tr_sumsq_ws_doubles((int)t->ranges.size()) * 8));
    TRY_HIP(tr_sumsq(src, t->ranges.data(), (int)t->ranges.size(), t->nws.as<double>(), st));
    double ss = 0.0;
    TRY_HIP(hipMemcpyAsync(&ss, t->nws.p, 8, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    *norm = std::sqrt(ss);
    return RS_OK;
}

}  // namespace

extern "C" {

int rs_trainer_set_trainable(rs_trainer* t, const char* hf_key_prefix, int32_t trainable) {
    if (!t || !hf_key_prefix) return rs_fail(RS_EARG, "null argument");
    if (t->acc_filled)
        return rs_fail(RS_ESTATE, "the accumulator holds gradients: apply or clear it before changing what is trainable");
    std::string pre(hf_key_prefix);
    while (!pre.empty() && pre.back() == '.') pre.pop_back();
    if (pre.empty()) return rs_fail(RS_EARG, "empty prefix");
    std::vector<std::string> keys;
    for (auto& kv : t->table) keys.push_back(kv.first);
    if (t->cfg.heads_mask == RS_HEAD_MLM) {
        keys.push_back("cls.predictions.decoder.weight");
        keys.push_back("cls.predictions.decoder.bias");
    }
    int n = 0;
    for (const std::string& k : keys) {
        if (!prefix_matches(k, pre)) continue;
        const size_t off = t->table[table_key(t, k)].first;
        if (trainable) t->frozen.erase(off);
        else t->frozen.insert(off);
        ++n;
    }
    if (!n) return rs_fail(RS_EARG, "no tensor matches the prefix " + pre);
    merge_ranges(t);
    t->have_grad = false;      // t->G was computed for another trainable set
    return RS_OK;
}

int rs_trainer_is_trainable(const rs_trainer* t, const char* hf_key) {
    if (!t || !hf_key) return rs_fail(RS_EARG, "null argument");
    auto it = t->table.find(table_key(t, hf_key));
    if (it == t->table.end()) return rs_fail(RS_EARG, std::string("unknown tensor ") + hf_key);
    return t->on(it->second.first) ? 1 : 0;
}

int rs_trainer_accumulate(rs_trainer* t, float weight, void* stream) {
    if (!t) return rs_fail(RS_EARG, "null trainer");
    if (!t->finalized) return rs_fail(RS_ESTATE, "rs_trainer_finalize not called");
    if (!t->have_grad)
        return rs_fail(RS_ESTATE, "no gradient to accumulate: no backward has run (since the trainable set last changed)");
    hipStream_t st = (hipStream_t)stream;
    TRY_HIP(hipSetDevice(t->device));
    if (!t->A.p) {
        TRY_ALLOC(t->A.ensure(t->n_params * 4));
        TRY_HIP(hipMemsetAsync(t->A.p, 0, t->n_params * 4, st));
    }
    for (const TrRange& r : t->ranges)
        TRY_HIP(tr_accum(t->A.as<float>() + r.off, t->G.as<float>() + r.off, r.n, weight, st));
    t->acc_filled = true;
    return RS_OK;
}

int rs_trainer_zero_accum(rs_trainer* t) {
    if (!t) return rs_fail(RS_EARG, "null trainer");
    TRY_HIP(hipSetDevice(t->device));
    TRY_HIP(hipDeviceSynchronize());
    if (t->A.p) TRY_HIP(hipMemset(t->A.p, 0, t->n_params * 4));
    t->acc_filled = false;
    return RS_OK;
}

int rs_trainer_grad_norm(rs_trainer* t, int32_t source, double* h_norm, void* stream) {
    if (!t || !h_norm) return rs_fail(RS_EARG, "null argument");
    if (!t->finalized) return rs_fail(RS_ESTATE, "rs_trainer_finalize not called");
    const float* src = nullptr;
    if (int r = grad_source(t, source, &src)) return r;
    TRY_HIP(hipSetDevice(t->device));
    return grad_norm(t, src, h_norm, (hipStream_t)stream);
}

int rs_trainer_apply(rs_trainer* t, const rs_train_opts* o, const rs_apply_opts* a, double* h_norm,
                     int32_t* h_applied, void* stream) {
    if (!t || !o || !a) return rs_fail(RS_EARG, "null argument");
    if (!t->finalized) return rs_fail(RS_ESTATE, "rs_trainer_finalize not called");
    if (!std::isfinite(a->grad_scale)) return rs_fail(RS_EARG, "grad_scale must be finite");
    const float* src = nullptr;
    if (int r = grad_source(t, a->source, &src)) return r;
    hipStream_t st = (hipStream_t)stream;
    TRY_HIP(hipSetDevice(t->device));
    double n = 0.0;
    if (int r = grad_norm(t, src, &n, st)) return r;
    n *= std::fabs((double)a->grad_scale);
    if (h_norm) *h_norm = n;
    if (h_applied) *h_applied = 0;
    if (!std::isfinite(n)) {                   // the skipped step of a non-finite gradient: nothing moves
        if (a->source == 1) RS_TRY(clear_accum(t, st));
        TRY_HIP(hipStreamSynchronize(st));
        return RS_OK;
    }
    // clip_grad_norm_'s coefficient; the gradient's whole multiplier rounded once
    const double c = a->max_grad_norm > 0.f ? std::min(1.0, (double)a->max_grad_norm / (n + 1e-6)) : 1.0;
    const float gmul = (float)((double)a->grad_scale * c);
    RS_TRY(adamw_ranges(t, o, src, gmul, st));
    if (a->source == 1) RS_TRY(clear_accum(t, st));
    TRY_HIP(hipStreamSynchronize(st));
    if (h_applied) *h_applied = 1;
    return RS_OK;
}

int rs_trainer_reset_optimizer(rs_trainer* t) {
    if (!t) return rs_fail(RS_EARG, "null trainer");
    if (!t->finalized) return rs_fail(RS_ESTATE, "rs_trainer_finalize not called");
    TRY_HIP(hipSetDevice(t->device));
    TRY_HIP(hipDeviceSynchronize());
    TRY_HIP(hipMemset(t->M1.p, 0, t->n_params * 4));
    TRY_HIP(hipMemset(t->V1.p, 0, t->n_params * 4));
    t->step = 0;
    return RS_OK;
}

int rs_trainer_set_token_types(rs_trainer* t, const int32_t* d_type, int64_t n) {
    if (!t) return rs_fail(RS_EARG, "null trainer");
    if (d_type && n < 0) return rs_fail(RS_EARG, "negative count");
    t->type_next = d_type;
    t->type_n = d_type ? n : 0;
    return RS_OK;
}

int64_t rs_trainer_dropout_step(const rs_trainer* t) { return t ? (int64_t)t->drop_step : -1; }

int rs_trainer_set_dropout_step(rs_trainer* t, int64_t step) {
    if (!t || step < 0) return rs_fail(RS_EARG, "bad argument");
    t->drop_step = (uint64_t)step;
    return RS_OK;
}

int rs_dropout_keep(uint32_t seed, uint64_t step, uint32_t site, float p, int64_t n, uint8_t* d_keep, void* stream) {
    if (n < 0 || (n > 0 && !d_keep)) return rs_fail(RS_EARG, "null argument");
    if (!(p >= 0.f && p < 1.f)) return rs_fail(RS_EARG, "p must be in [0, 1)");
    TrDrop d;
    d.seed = seed;
    d.step = (uint32_t)step;
    d.step_hi = (uint32_t)(step >> 32);
    d.site = site;
    d.thresh = drop_thresh(p);
    TRY_HIP(tr_dropout_keep(d_keep, (long long)n, d, (hipStream_t)stream));
    return RS_OK;
}

void rs_trainer_destroy(rs_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    if (t->blas) (void)rocblas_destroy_handle(t->blas);
    for (DevBuf* b : {&t->P, &t->G, &t->M1, &t->V1, &t->act, &t->grad, &t->meta, &t->small, &t->ws, &t->A, &t->nws})
        b->release();
    delete t;
}

}  // extern "C"
