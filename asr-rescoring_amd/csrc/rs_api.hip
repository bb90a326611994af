// C-ABI host side of librescore (see include/rescore.h): weight packing, ragged
// sequence scheduling into launch chunks, and the per-chunk kernel pipeline.
//
// Scheduling replaces the reference's DataLoader of 32 padded rows
// (MLM_PLL/main.py:57-70, RescoreBert/main.py:71-79): all sequences of a call are
// flattened into ragged token rows and cut into chunks of <= max_rows rows, so every
// GEMM launch sees tens of thousands of rows and no padding tokens.
#include <map>
#include <string>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cmath>
#include <algorithm>

#include "common.h"
#include "seq_plan.h"
#include "bertscore_plan.h"
#include "host_util.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

struct Layer {
    f16 *wqkv, *wo, *w1, *w2;       // operand images of the precision mode (kx parts, planar)
    f16 *iqkv = nullptr, *io = nullptr, *i1 = nullptr, *i2 = nullptr;   // fp16x3: interleaved two-part
                                    // images [W_hi | W_lo*64] of the split-operand GEMMs (ldw = 2K)
    float *bqkv, *bo, *b1, *b2, *g1, *be1, *g2, *be2;
    float *wkf = nullptr, *wvt = nullptr;   // last layer, fp16x3: fp32 weight images of the folded
                                    // attention (common.h AttnFold: Wk / 8, Wv transposed)
};

// Pinned staging buffer (int words) of one asynchronous upload per call: the next call waits for
// the previous upload's event before it overwrites the buffer.  The event is created at first use.
struct Staging {
    int* p = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    // waits for the previous upload and grows the buffer p to n ints
    hipError_t begin(size_t n) {
        hipError_t e = done ? hipEventSynchronize(done) : hipSuccess;
        if (e == hipSuccess && n > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            e = hipHostMalloc((void**)&p, std::max<size_t>(n, 1) * 4, hipHostMallocDefault);
            cap = e == hipSuccess ? n : 0;
        }
        return e;
    }
    // the first n ints -> dst (grown to hold them), asynchronously on st
    hipError_t upload(DevBuf& dst, size_t n, hipStream_t st) {
        hipError_t e = dst.ensure(std::max<size_t>(n, 1) * 4);
        if (e == hipSuccess) e = hipMemcpyAsync(dst.p, p, n * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && !done) e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
        return e == hipSuccess ? hipEventRecord(done, st) : e;
    }
    ~Staging() {       // with the model (rs_model_destroy, on the model's device)
        if (p) (void)hipHostFree(p);
        if (done) (void)hipEventDestroy(done);
    }
};

}  // namespace

struct rs_model {
    rs_bert_cfg cfg{};
    int device = 0;
    bool finalized = false;
    std::map<std::string, std::vector<float>> host;   // fp32 state_dict staged until finalize
    std::vector<void*> allocs;                          // packed weights
    // packed weights
    float *word32 = nullptr, *pos32 = nullptr, *type32 = nullptr, *eg = nullptr, *eb = nullptr;
    std::vector<Layer> layers;
    f16* wt = nullptr;  float *bt = nullptr, *gt = nullptr, *bet = nullptr;   // MLM transform
    f16* wdec = nullptr; float* bdec = nullptr; int vpad = 0;                // tied decoder
    float *wlin = nullptr, *blin = nullptr;                                   // RescoreBert linear
    // workspace
    int64_t max_rows = 0;
    int s_cap = 0, r_pad = 0, m_pad = 0;
    int kx = 1;                 // fp16 operand image width (1: fp16, 3: fp16x3)
    bool x3s_w = false;         // the split-operand weight images exist (fp16x3, every projection
                                // weight |w| < 1023.75 so that 64 W_hi is finite in the x3s K loop)
    DevBuf xst, h16, t32, qkv, ctx, inter;   // xst: (mean, rstd) of the pre-LN rows in t32
    DevBuf xst1;                // statistics of the post-attention stream (deferred residual)
    DevBuf lnx, lncnt, lnerr;   // EPI_LNRES_IMG: per-tile row statistics, gang-ticket words (left
                                // zeroed by every launch), sticky statistics-wait timeout flag
    DevBuf ctxq, resq, tq32, hq32, hq16, interq, lab, llog, part, rowlp_tmp;
    DevBuf meta;
    DevBuf topk_cand;           // top-k calls (topk_begin): topk_cand_bytes(vpad), from the first such call on
    // candidate calls (rs_masked_logprob_cands), from the first such call on: the call's offsets,
    // sorted ids and permutation (one upload), and the candidate logits of one chunk
    DevBuf cand_meta, cand_logit;
    // rs_model_set_token_types: segment ids pending for the next encoder call, [type_n] device ints
    // parallel to its tokens (PendingTypes hands them to that call and clears them)
    const int32_t* type_next = nullptr;
    int64_t type_n = 0;
    DevBuf emb, plan;           // rs_bertscore_recall: token embeddings, work-item plan
    DevBuf flag;                // non-finite-output flag of the last scoring call(s) (range guard)
    bool sync_check = true;     // scoring calls synchronise and report their flags (rs_model_set_sync_check)
    int* pinned_flag = nullptr;
    // metadata (run_all) and BERTScore plan uploads: rs_bertscore_recall does both in one call, and
    Staging stage_meta, stage_plan;   // a shared buffer would make it wait on the host in between
    Staging stage_cand;               // rs_masked_logprob_cands: the candidate lists (before its stage_meta upload)
    // call ordering across streams: the end of the last call's work (any stream); a call on another
    // stream first makes its stream wait for it (CallOrder)
    hipEvent_t call_done = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    bool order_lost = false;     // a call could not record call_done (order_begin reports it)
    // profiling
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    struct Rec { int kind; hipEvent_t a, b; double flops; };
    std::vector<Rec> recs;
    double prof_ms[RS_K_COUNT] = {};
    int64_t prof_n[RS_K_COUNT] = {};
    double prof_flops[RS_K_COUNT] = {};
};

namespace {

// Tail of the weight uploads: allocate, remember (freed by rs_model_destroy), copy.
void* to_device(rs_model* m, const void* src, size_t bytes, hipError_t* err) {
    void* p = nullptr;
    *err = hipMalloc(&p, bytes);
    if (*err != hipSuccess) return nullptr;
    m->allocs.push_back(p);
    *err = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    return p;
}

// Weight W [rows, cols] (nn.Linear [out, in]) -> fp16 operand image [rows_pad, kx*cols]:
// kx == 1: [hi]; kx == 3: [hi | lo*64 | hi/64] (pairs with the activation image
// [hi | hi/64 | lo*64], common.h put_split: the factors keep lo out of the fp16 subnormals).
f16* upload_f16(rs_model* m, const std::vector<float>& src, size_t rows_pad, size_t cols, int kx,
                hipError_t* err) {
    std::vector<f16> tmp(rows_pad * cols * kx, (f16)0.0f);
    const size_t rows = src.size() / cols;
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) {
            const float v = src[r * cols + c];
            const f16 hi = (f16)v;
            f16* row = tmp.data() + r * cols * kx;
            row[c] = hi;
            if (kx == 3) {
                row[cols + c] = (f16)((v - (float)hi) * 64.f);
                row[2 * cols + c] = (f16)((float)hi * (1.f / 64.f));
            }
        }
    return (f16*)to_device(m, tmp.data(), tmp.size() * sizeof(f16), err);
}

// Weight W [rows, cols] -> the split-operand GEMM's interleaved two-part image [rows, 2 cols]
// (common.h, kx == 2): per 32-column K-step [hi 32 | lo*64 32], the same hi / lo*64 values as the
// planar three-part image's first two parts.
f16* upload_il(rs_model* m, const std::vector<float>& src, size_t cols, hipError_t* err) {
    const size_t rows = src.size() / cols;
    std::vector<f16> tmp(rows * cols * 2, (f16)0.0f);
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) {
            const float v = src[r * cols + c];
            const f16 hi = (f16)v;
            f16* row = tmp.data() + r * cols * 2;
            row[il_hi((int)c)] = hi;
            row[il_hi((int)c) + 32] = (f16)((v - (float)hi) * 64.f);
        }
    return (f16*)to_device(m, tmp.data(), tmp.size() * sizeof(f16), err);
}

// The split-operand K loop forms 64 W_hi in fp16 (k_gemm.hip kstep16): finite only for
// |W_hi| <= 1023.5, i.e. |w| < 1023.75.  A model with a larger projection weight runs its fp16x3
// layers in the K-concatenated form instead (no 64x factor on W_hi), which holds |w| <= 65504.
bool x3s_range_ok(const std::vector<float>& v) {
    for (float x : v)
        if (!(std::fabs(x) < 1023.75f)) return false;
    return true;
}

float* upload_f32(rs_model* m, const std::vector<float>& src, size_t n_pad, hipError_t* err) {
    std::vector<float> tmp(std::max(n_pad, src.size()), 0.0f);
    std::memcpy(tmp.data(), src.data(), src.size() * sizeof(float));
    return (float*)to_device(m, tmp.data(), tmp.size() * sizeof(float), err);
}

// The fp16 operand images (fp16 and fp16x3 modes) hold |x| <= 65504: a weight beyond it
// would become inf in its hi part (and NaN in lo), where the reference's fp32 forward stays
// finite.  Checked once at finalize.
bool fp16_range_ok(const std::vector<float>& v) {
    for (float x : v)
        if (!(std::fabs(x) <= 65504.f)) return false;
    return true;
}

// Activations are checked through their consequence: an operand that leaves the fp16 range
// becomes inf (hi) / NaN (lo) in its image, and inf / NaN then reaches every score that
// depends on it (LayerNorm, softmax and the log-softmax turn it into NaN; the fp32 reference
// stays finite there).  One pass over a call's outputs sets a flag, the call synchronises
// its stream and fails with RS_EUNSUP instead of returning non-finite scores.
template <class T>
__global__ void __launch_bounds__(256) nonfinite_kernel(const T* __restrict__ v, size_t n, int* __restrict__ flag) {
    int bad = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        bad |= !__builtin_isfinite((float)v[i]);
    if (bad) flag[0] = 1;          // plain vector store; every writer stores the same value
}

// Reads the flags (non-finite output, statistics-wait timeout) after synchronising the stream,
// clears them and turns them into the call's error.
int report_flags(rs_model* m, hipStream_t st, const char* what) {
    if (!m->pinned_flag) TRY_HIP(hipHostMalloc((void**)&m->pinned_flag, 8, hipHostMallocDefault));
    m->pinned_flag[0] = 0;
    m->pinned_flag[1] = 0;
    if (m->flag.p) TRY_HIP(hipMemcpyAsync(m->pinned_flag, m->flag.p, 4, hipMemcpyDeviceToHost, st));
    if (m->lnerr.p) TRY_HIP(hipMemcpyAsync(m->pinned_flag + 1, m->lnerr.p, 4, hipMemcpyDeviceToHost, st));
    TRY_HIP(hipStreamSynchronize(st));
    const int bad = m->pinned_flag[0], lnto = m->pinned_flag[1];
    if (bad && m->flag.p) TRY_HIP(hipMemset(m->flag.p, 0, 4));
    if (lnto) {
        TRY_HIP(hipMemset(m->lnerr.p, 0, 4));
        return fail(RS_EHIP, "a residual-LayerNorm GEMM timed out waiting for its row statistics "
                             "(set RS_LNFUSE=0 to use the separate LayerNorm pass)");
    }
    if (bad)
        return fail(RS_EUNSUP, std::string("non-finite ") + what +
                                   ": an activation left the fp16 range of the operand images (|x| > 65504); "
                                   "the fp32 reference stays finite here");
    return RS_OK;
}

// End of every scoring call: one pass over its outputs sets the non-finite flag.  Synchronous
// mode (default): the call waits for its stream and reports the flags.  Deferred mode
// (rs_model_set_sync_check(m, 0)): the pass is only enqueued, the flags accumulate on the device
// and rs_check reports them, so pipelined callers keep their stream asynchronous.
// (mark_nonfinite: the pass alone, for a call with a second output to check.)
template <class T>
int mark_nonfinite(rs_model* m, hipStream_t st, const T* p, size_t n) {
    if (!m->flag.p) {
        TRY_HIP(m->flag.ensure(4));
        TRY_HIP(hipMemset(m->flag.p, 0, 4));
    }
    if (n > 0) {
        const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
        hipLaunchKernelGGL(nonfinite_kernel<T>, dim3(blocks), dim3(256), 0, st, p, n, m->flag.as<int>());
        TRY_HIP(hipGetLastError());
    }
    return RS_OK;
}
template <class T>
int check_finite(rs_model* m, hipStream_t st, const T* p, size_t n, const char* what) {
    if (int r = mark_nonfinite(m, st, p, n)) return r;
    if (!m->sync_check) return RS_OK;
    return report_flags(m, st, what);
}

// Start of every scoring call in synchronous mode: a timeout flag left by an earlier call that
// failed before its report is dropped (each call reports only its own).
int begin_call(rs_model* m, hipStream_t st) {
    if (m->sync_check && m->lnerr.p) TRY_HIP(hipMemsetAsync(m->lnerr.p, 0, 4, st));
    if (m->sync_check && m->flag.p) TRY_HIP(hipMemsetAsync(m->flag.p, 0, 4, st));
    return RS_OK;
}

// Calls on one model handle are ordered, whatever streams they come on: the handle's workspace,
// LayerNorm gang tickets and flags are shared by every call, so a call on a different stream than the
// previous call first makes its stream wait (device-side, hipStreamWaitEvent) for the previous call's
// work, and every call records the end of its own work in call_done (created at finalize on the
// model's device).  Host threads must still not share a handle.  A failed wait fails the call
// (RS_EHIP); a failed record cannot change the return of the call it ends, so it is sticky: the next
// call on the handle fails with RS_EHIP instead of running unordered.
int order_begin(rs_model* m, hipStream_t st) {
    if (m->order_lost) {
        m->order_lost = false;
        return fail(RS_EHIP, "the previous call on this handle could not record its end (hipEventRecord "
                             "failed): cross-stream ordering was lost; synchronise the device and retry");
    }
    if (m->have_last && st != m->last_stream && m->call_done)
        TRY_HIP(hipStreamWaitEvent(st, m->call_done, 0));
    return RS_OK;
}
struct CallOrder {
    rs_model* m;
    hipStream_t st;
    CallOrder(rs_model* m_, hipStream_t st_) : m(m_), st(st_) {}
    ~CallOrder() {
        if (!m->call_done) return;                // not finalized: no call ran kernels
        if (hipEventRecord(m->call_done, st) == hipSuccess) {
            m->last_stream = st;
            m->have_last = true;
        } else {
            m->order_lost = true;
        }
    }
};
// Opening of every entry point that enqueues work: the model's device, then the call ordering.
#define CALL_ORDER(m_, st_)                                   \
    TRY_HIP(hipSetDevice(m_->device));                         \
    if (int r_ = order_begin((m_), (st_))) return r_;         \
    CallOrder order_((m_), (st_))

// Row count padded to the GEMM kernels' row alignment.
int pad_rows(int64_t rows) {
    const int al = gemm_row_align();
    return (int)((rows + al - 1) / al * al);
}

int reserve_impl(rs_model* m, int64_t max_rows) {
    const rs_bert_cfg& c = m->cfg;
    if (max_rows < 512) return fail(RS_EARG, "max_rows must be >= 512");
    if (max_rows > (int64_t)1 << 26) return fail(RS_EARG, "max_rows too large");
    m->max_rows = max_rows;
    m->m_pad = pad_rows(max_rows);
    m->s_cap = (int)(max_rows / 3) + 1;
    m->r_pad = pad_rows(m->s_cap);
    const size_t M = m->m_pad, R = m->r_pad, H = c.hidden, F = c.intermediate;
    TRY_HIP(hipSetDevice(m->device));
    const size_t kx = m->kx;
    TRY_HIP(m->xst.ensure(M * sizeof(float2)));
    TRY_HIP(m->xst1.ensure(M * sizeof(float2)));
    TRY_HIP(m->lnx.ensure(lnres_granules((int)M) * 8));
    TRY_HIP(hipMemset(m->lnx.p, 0, m->lnx.bytes));               // granule tags start at 0 (never a launch's)
    if (!m->lncnt.p) {
        TRY_HIP(m->lncnt.ensure(lnres_counter_bytes()));
        TRY_HIP(hipMemset(m->lncnt.p, 0, m->lncnt.bytes));
    }
    TRY_HIP(m->lnerr.ensure(16));
    TRY_HIP(hipMemset(m->lnerr.p, 0, 16));
    TRY_HIP(m->h16.ensure(M * H * 2 * kx));
    TRY_HIP(m->t32.ensure(M * H * 4));
    TRY_HIP(m->qkv.ensure(M * 3 * H * (kx == 3 ? 4 : 2)));
    TRY_HIP(m->ctx.ensure(M * H * 2 * kx));
    TRY_HIP(m->inter.ensure(M * F * 2 * kx));
    TRY_HIP(m->ctxq.ensure(R * H * 2 * kx));
    TRY_HIP(m->resq.ensure(R * H * 4));
    TRY_HIP(m->tq32.ensure(R * H * 4));
    TRY_HIP(m->hq32.ensure(R * H * 4));
    TRY_HIP(m->hq16.ensure(R * H * 2 * kx));
    TRY_HIP(m->interq.ensure(R * F * 2 * kx));
    TRY_HIP(m->lab.ensure(R * 4));
    TRY_HIP(m->llog.ensure(R * 4));
    if (c.heads_mask & RS_HEAD_MLM) TRY_HIP(m->part.ensure(R * (size_t)(m->vpad / 64) * sizeof(float2)));
    // zero the padded activations once: GEMMs read pad rows (never stored back)
    TRY_HIP(hipMemset(m->h16.p, 0, m->h16.bytes));
    TRY_HIP(hipMemset(m->ctx.p, 0, m->ctx.bytes));
    TRY_HIP(hipMemset(m->inter.p, 0, m->inter.bytes));
    TRY_HIP(hipMemset(m->ctxq.p, 0, m->ctxq.bytes));
    TRY_HIP(hipMemset(m->hq16.p, 0, m->hq16.bytes));
    TRY_HIP(hipMemset(m->interq.p, 0, m->interq.bytes));
    TRY_HIP(hipMemset(m->t32.p, 0, m->t32.bytes));    // pad rows of the residual stream stay finite
    TRY_HIP(hipMemset(m->xst.p, 0, m->xst.bytes));
    TRY_HIP(hipMemset(m->xst1.p, 0, m->xst1.bytes));
    return RS_OK;
}

const std::vector<float>* need(rs_model* m, const std::string& k, size_t n, std::string* missing) {
    auto it = m->host.find(k);
    if (it == m->host.end()) {
        if (missing->empty()) *missing = k + " (missing)";
        return nullptr;
    }
    if (it->second.size() != n) {
        if (missing->empty()) *missing = k + " (wrong size)";
        return nullptr;
    }
    return &it->second;
}

// ---- profiling helpers ----------------------------------------------------------------
hipEvent_t next_event(rs_model* m) {
    if (m->ev_used == m->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        m->ev_pool.push_back(e);
    }
    return m->ev_pool[m->ev_used++];
}

struct ProfScope {
    rs_model* m;
    hipStream_t st;
    int kind;
    double flops;
    hipEvent_t a = nullptr;
    ProfScope(rs_model* m_, hipStream_t st_, int kind_, double flops_) : m(m_), st(st_), kind(kind_), flops(flops_) {
        if (m->prof) {
            a = next_event(m);
            if (a) (void)hipEventRecord(a, st);
        }
    }
    ~ProfScope() {
        if (m->prof && a) {
            hipEvent_t b = next_event(m);
            if (b) {
                (void)hipEventRecord(b, st);
                m->recs.push_back({kind, a, b, flops});
            }
        }
    }
};

// One launch under a profile scope of its own, no flops recorded (m, st: the caller's).
#define LAUNCH(kind_, call_) do { ProfScope ps_(m, st, (kind_), 0); TRY_HIP(call_); } while (0)
#define LAUNCH_OTHER(call_) LAUNCH(RS_K_OTHER, call_)

enum Mode { MODE_MLM = 0, MODE_CLS = 1, MODE_EMB = 2 };

// What one encoder call fixes.  Every entry point builds one on its stack; run_all and ChunkCtx read
// it and nothing call-scoped from the handle, so no return path has anything to put back.
struct Call {
    int mode;
    const int* d_tok;
    float* out_rows = nullptr;                // MLM / CLS: one float per sequence
    const int* d_label = nullptr;             // device labels in place of the sequence list's column
    const int32_t* d_type = nullptr;          // segment ids parallel to d_tok (null: every row type 0)
    const std::vector<int>* extra = nullptr;  // extra ints of the metadata upload (e.g. hypothesis ->
    int** d_extra = nullptr;                  // sequence offsets), and where their device copy lands
    f16* emb_dst = nullptr;                   // MODE_EMB output
    // top-k request (topk_begin): k != 0 makes head_mlm run the top-k decoder form into [sequence, k]
    int topk_k = 0;
    int32_t* topk_id = nullptr;
    float* topk_lp = nullptr;
    // candidate request (query-list calls; cands_begin): head_mlm runs the candidate decoder form,
    // out_rows then holds one float per candidate, in the caller's order
    const struct CandLists* cands = nullptr;
    // multi-mask rows: several scored positions per sequence (seq_plan.h QueryList); the last layer
    // and the head then run one row per query, out_rows holds one float per query
    const QueryList* ql = nullptr;
};

// The candidate lists of a call, query q's at entries [off[q], off[q + 1]): ids sorted by (id,
// original index) inside each list, perm the original (caller's) index of every entry.
struct CandLists {
    std::vector<int> off;                     // [n_q + 1] host
    const int *d_off = nullptr, *d_id = nullptr, *d_perm = nullptr;   // their device copies (cand_meta)
    float* d_logit = nullptr;                 // one chunk's candidate logits (cand_logit)
};

// The environment switches of one scoring call: read once (call_opts, at the top of run_all) and
// passed down, so that the chunk cap, the dedup plan and the chunk runner see the same resolved
// forms.  Read per call, not once per process, so that a test can flip a switch in-process.
struct CallOpts {
    bool lastq, dedup, chunk_align;
    bool lastfold;                        // the last layer's K / V projections folded into the query side
    int ln_diag;
    // the layer forms that run, resolved against the model's precision mode, weights and shape
    bool x3s, imgres, lnfuse, x3_dedup;   // fp16x3
    bool oproj_f16, ffn2_f16;             // fp16
    int lnres_defer;                      // fp16: 0, 1 or 2; 0 where there is no fp16 O output to defer
};

CallOpts call_opts(const rs_model* m) {
    const rs_bert_cfg& cf = m->cfg;
    auto is = [](const char* name, const char* v) { const char* e = getenv(name); return e && !strcmp(e, v); };
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    CallOpts o{};
    // RS_LASTQ: "0" = full Q/K/V GEMM at the last layer (default: Q of the scored rows only)
    o.lastq = !is("RS_LASTQ", "0");
    // RS_DEDUP (default 1): layer-0 dedup (plan_unique_rows): MLM mode, fp16 operands (or the
    // fp16x3 form below), >= 2 layers (layer 0 is not the query-only layer)
    o.dedup = num("RS_DEDUP", 1) != 0;
    // RS_CHUNK_ALIGN: "0" = chunks of max_rows (default: whole LayerNorm-gang rounds, chunk_cap)
    o.chunk_align = !is("RS_CHUNK_ALIGN", "0");
    // RS_OPROJ: "f16" (default in the fp16 precision mode: fp16-output O projection + fused
    // residual/LayerNorm rows kernel) or "resln" (residual rebuilt in the GEMM's accumulators)
    o.oproj_f16 = m->kx == 1 && !is("RS_OPROJ", "resln");
    // RS_FFN2: "resln" (default) or "f16" (the O-projection split applied to BertOutput)
    o.ffn2_f16 = m->kx == 1 && is("RS_FFN2", "f16");
    // RS_LNRES_DEFER (fp16 mode, O-projection split): ln_res_rows writes only the statistics and
    // the fp16 image of the post-attention stream x = LN0(x32) + o1 (o1 = fp16 O-projection
    // output), so x never round-trips through HBM in fp32, and x is rebuilt downstream:
    //   2 (default): BertOutput is a lean fp16-output GEMM (o2) and one second ln_res_rows pass
    //                forms LN2(LN1(LN0(x32) + o1) + o2) — no residual traffic in any GEMM epilogue;
    //   1: the BertOutput GEMM rebuilds x in its accumulator init (EpiArgs.res_o16) — slower: the
    //      extra loads sit in front of the tile's first MFMA;
    //   0: ln_res_rows writes x back into x32 and BertOutput reads it (EPI_RESLN_F32).
    const int defer = num("RS_LNRES_DEFER", 2);
    o.lnres_defer = !o.oproj_f16 || o.ffn2_f16 || defer == 0 ? 0 : defer == 2 ? 2 : 1;
    // RS_LNFUSE_DIAG=8 (tests): every statistics / gang wait times out at once (the RS_EHIP
    // path); no other bit is honoured (no diagnostic changes scores)
    o.ln_diag = num("RS_LNFUSE_DIAG", 0) & 8;
    // RS_X3S (fp16x3 mode, default 1): the encoder projections run as split-operand GEMMs
    // (gemm_x3s_kernel: two-part activation images, three fp16 products formed in registers, fp32
    // outputs + ln_res32 rows for the residual blocks); 0 = the K-concatenated three-part form.
    o.x3s = m->kx == 3 && !is("RS_X3S", "0") && m->x3s_w && cf.hidden % 256 == 0 && cf.intermediate % 256 == 0;
    // RS_X3S_IMGRES (split-operand layers, default 1): the residual stream is held only as the
    // two-part image of the normalised hidden state (ln_res_img: 12 B per element per residual
    // block, no fp32 pre-LN stream or statistics); 0 = ln_res32 over the fp32 pre-LN stream.
    o.imgres = o.x3s && !is("RS_X3S_IMGRES", "0");
    // RS_LNFUSE (image-held residual; default 1): the residual add + LayerNorm of both blocks run in
    // the O-projection / BertOutput GEMM epilogues (EPI_LNRES_IMG: full rows through an in-launch
    // exchange of row statistics) instead of as ln_res_img passes (RS_LNFUSE=0).
    o.lnfuse = o.imgres && !is("RS_LNFUSE", "0") && cf.hidden % 256 == 0 && cf.hidden <= 1024;
    // fp16x3 layer-0 dedup: the split-operand layer with the image-held residual (its attention
    // kernel reads the unique rows for chunks with T <= 64)
    o.x3_dedup = o.imgres;
    // RS_LASTFOLD (default 1; split-operand layers with the image-held residual, single-query
    // sequences): the last layer applies its K / V projections to the query side
    // (launch_attention_fold) instead of projecting K and V for every row; 0 = the all-rows K / V GEMM
    // and attention_query.  Independent of RS_LASTQ, which only says where the scored rows' Q comes
    // from (their own GEMM, or the Q columns of the full Q/K/V GEMM: the same bits), so the default and
    // RS_LASTQ=0 stay bitwise equal.
    o.lastfold = o.imgres && !is("RS_LASTFOLD", "0") && attention_fold_ok(cf.hidden, cf.heads) &&
                 !m->layers.empty() && m->layers.back().wkf != nullptr;
    return o;
}

// One chunk's run of the encoder + head over sequences [c.s0, c.s1): what the call fixed, and the
// typed workspace pointers.  Aggregate: the first seven members are given, the rest follow.
struct ChunkCtx {
    rs_model* m;
    hipStream_t st;
    const Call& call;
    const SeqMeta& sm;
    const Chunk& c;
    const CallOpts& o;
    const QueryMeta& qm;                      // query-list calls (call.ql), else unused
    const rs_bert_cfg& cf = m->cfg;
    const int H = cf.hidden, F = cf.intermediate, nh = cf.heads, kx = m->kx;
    const float eps = cf.ln_eps;
    const bool q32 = kx == 3;                 // fp16x3: QKV kept in fp32 for attention
    const int qkv_epi = q32 ? EPI_BIAS_F32 : EPI_BIAS_F16;   // (split-operand layers are fp16x3: fp32)
    const int rows = c.rows, ns = c.s1 - c.s0;
    // rows of the query-row-only layer and the head, and the first of them in the call's output:
    // one per sequence, or (query-list calls) one per query
    const bool mq = call.ql != nullptr;
    const int nr = mq ? c.nq : ns, r0 = mq ? c.q0 : c.s0;
    const bool dedup = c.urows > 0;           // layer-0 Q/K/V over unique rows (MLM; fp16, or fp16x3 split)
    const int kxf = o.x3s ? 2 : kx;           // width factor of the full-row operand images (split: two-part)
    float2 *xst = m->xst.as<float2>(), *xst1 = m->xst1.as<float2>();
    float* t32 = m->t32.as<float>();          // residual stream, pre-LN fp32 (LN rebuilt from xst)
    f16* h16 = m->h16.as<f16>();              // ... or, with imgres, its image here
    void* qkv = m->qkv.p;
    f16 *ctx = m->ctx.as<f16>(), *inter = m->inter.as<f16>();
    // one row per sequence or query (query-row-only layer and heads)
    f16 *ctxq = m->ctxq.as<f16>(), *hq16 = m->hq16.as<f16>(), *interq = m->interq.as<f16>();
    float *resq = m->resq.as<float>(), *tq = m->tq32.as<float>(), *hq32 = m->hq32.as<float>();

    // One GEMM over m_valid rows (padded to the kernels' row alignment), profiled as `kind`.
    // split: the split-operand kernel (A a two-part image, W rows of 2K halfs, K the logical depth:
    // three fp16 products, 2·m·n·3K flops); else launch_gemm (K the operand images' width, 2·m·n·K).
    int gemm(int kind, int epi, bool split, const f16* A, const f16* W, int m_valid, int N_pad, int K, EpiArgs ep,
             int n_flop_cols) {
        ep.m_valid = m_valid;
        ProfScope ps(m, st, kind, 2.0 * m_valid * (double)n_flop_cols * (split ? 3.0 * K : K));
        if (split) TRY_HIP(launch_gemm_x3s(epi, A, W, 2 * K, pad_rows(m_valid), N_pad, K, ep, st));
        else TRY_HIP(launch_gemm(epi, A, W, pad_rows(m_valid), N_pad, K, ep, st,
                                kind == RS_K_OPROJ ? 1 : kind == RS_K_FFN2 ? 2 : 0));
        return RS_OK;
    }
    // out <- acc + bias (+ res: fp32 rows of the same layout)
    EpiArgs bias_ep(const float* bias, void* out, int ldc, const float* res = nullptr) const {
        EpiArgs e{};
        e.bias = bias; e.out = out; e.ldc = ldc; e.res = res;
        return e;
    }
    // GELU output as an operand image of width factor w
    EpiArgs gelu_ep(const float* bias, f16* out, int w) const {
        EpiArgs e = bias_ep(bias, out, w * F);
        e.kx = w; e.nlog = F;
        return e;
    }
    // residual GEMM: t32 <- acc + bias + LN(t32) (in place: a tile reads and writes only its own
    // rows x columns), LN given by the statistics in xst and the LN parameters (lg, lb)
    EpiArgs resln_ep(const float* bias, const float* lg, const float* lb) const {
        EpiArgs e = bias_ep(bias, t32, H, t32);
        e.res_stats = xst; e.res_g = lg; e.res_b = lb;
        return e;
    }
    // LayerNorm that produced layer li's input (embeddings LN, or the previous BertOutput LN)
    const float* prev_g(int li) const { return li ? m->layers[li - 1].g2 : m->eg; }
    const float* prev_b(int li) const { return li ? m->layers[li - 1].be2 : m->eb; }
    int embed() {
        ProfScope ps(m, st, RS_K_OTHER, 0);
        // dedup: the per-copy pass keeps only the fp32 residual + LN statistics; the layer-0
        // GEMM operand is built over the chunk's unique rows (plan_unique_rows)
        // (split-operand dedup: every copy row's image stays in h16 — it is the layer-0
        // residual — and the unique rows' image goes to the idle FFN buffer)
        // (segment ids, call.d_type: indexed like d_tok, so a unique row, keyed by hypothesis and
        // position, has one type and the plan is the same with and without them)
        // (multi-mask rows: the [MASK] set is the sequence's query list; never with dedup)
        if (mq && call.ql->masked) {
            TRY_HIP(launch_embed_ln_set(call.d_tok, call.d_type, sm, qm, c.s0, c.s1, cf.mask_id, cf.vocab, cf.type_vocab,
                                       m->word32, m->pos32, m->type32, m->eg, m->eb, eps, H, o.imgres ? nullptr : t32,
                                       o.imgres ? nullptr : xst, h16, kxf, st));
            return RS_OK;
        }
        TRY_HIP(launch_embed_ln(call.d_tok, call.d_type, sm, c.s0, c.s1, 0, cf.mask_id, cf.vocab, cf.type_vocab, m->word32,
                               m->pos32, m->type32, m->eg, m->eb, eps, H, o.imgres ? nullptr : t32,
                               o.imgres ? nullptr : xst, dedup && !o.x3s ? nullptr : h16, kxf, st));
        if (dedup)
            TRY_HIP(launch_embed_unique(call.d_tok, call.d_type, sm, c.s0, c.s1, c.urows, cf.mask_id, cf.vocab,
                                       cf.type_vocab, m->word32, m->pos32, m->type32, m->eg, m->eb, eps, H,
                                       o.x3s ? inter : h16, kxf, st));
        return RS_OK;
    }

    // Q/K/V projection of layer li into qkv, in the layer's GEMM form (split-operand or plain).
    // uq: over the chunk's unique rows (layer-0 dedup).  qrow: the query-row-only form, which
    // leaves the dense Q in tq.
    int qkv_proj(int li, bool last, bool uq, bool qrow) {
        const Layer& L = m->layers[li];
        const bool sp = o.x3s;
        const f16* W = sp ? L.iqkv : L.wqkv;
        const int K = sp ? H : kx * H, ldw = sp ? 2 * H : kx * H;   // GEMM depth as gemm() takes it; halfs per weight row
        if (!qrow)
            return gemm(RS_K_QKV, qkv_epi, sp, uq && sp ? inter : h16, W, uq ? c.urows : rows, 3 * H, K,
                        bias_ep(L.bqkv, qkv, 3 * H), last ? 2 * H : 3 * H);
        // K and V for every row (rows H..3H of the fused weight, written into columns H..3H of
        // qkv), Q only for the scored row(s) of each sequence (gathered operand rows -> dense
        // [sequence or query, H] in the idle tq32 buffer)
        // (folded last layer: no K / V row is projected, layer_query applies Wk and Wv to the query side)
        if (!fold()) {
            if (int r = gemm(RS_K_QKV, qkv_epi, sp, h16, W + (size_t)H * ldw, rows, 2 * H, K,
                             bias_ep(L.bqkv + H, (char*)qkv + H * (size_t)(q32 ? 4 : 2), 3 * H), 2 * H)) return r;
        }
        if (mq) LAUNCH_OTHER(launch_gather_query_rows_list(h16, kxf * H, sm, qm, c.q0, c.nq, hq16, st));
        else LAUNCH_OTHER(launch_gather_query_rows(h16, kxf * H, sm, c.s0, c.s1, 0, hq16, st));
        return gemm(RS_K_QKV, qkv_epi, sp, hq16, W, nr, H, K, bias_ep(L.bqkv, tq, H), H);
    }

    // Residual block of the split-operand layer: h16 <- image(LN(A·Wᵀ + b + h16)) in the GEMM
    // epilogue (lnfuse), or an fp32 GEMM output (o32 in the dead QKV buffer) closed by a separate
    // residual + LayerNorm pass: ln_res_img on the image, or ln_res32 (x32 <- LN(x32; pg, pb) + o32,
    // next two-part image) on the fp32 pre-LN stream.
    int split_block(int kind, const f16* A, const f16* W, int K, const float* bias, const float* pg, const float* pb,
                    const float* g, const float* be) {
        if (o.lnfuse) {
            EpiArgs e = bias_ep(bias, h16, 2 * H);
            e.nlog = H; e.res_g = g; e.res_b = be; e.ln_eps = eps; e.lnx = m->lnx.p;
            e.lncnt = m->lncnt.as<unsigned>(); e.lnerr = m->lnerr.as<unsigned>(); e.diag = o.ln_diag;
            return gemm(kind, EPI_LNRES_IMG, true, A, W, rows, H, K, e, H);
        }
        float* o32 = (float*)qkv;
        if (int r = gemm(kind, EPI_BIAS_F32, true, A, W, rows, H, K, bias_ep(bias, o32, H), H)) return r;
        if (o.imgres) LAUNCH_OTHER(launch_ln_res_img(h16, o32, rows, g, be, eps, H, st));
        else LAUNCH_OTHER(launch_ln_res32(t32, xst, xst, pg, pb, o32, rows, g, be, eps, H, h16, 2, st));
        return RS_OK;
    }
    // fp16x3 split-operand full layer
    int layer_split(int li, bool uq) {
        const Layer& L = m->layers[li];
        LAUNCH(RS_K_ATTN, launch_attention_full(qkv, true, sm, c.s0, c.s1, 0, H, nh, ctx, 2, st, uq, c.max_len));
        if (int r = split_block(RS_K_OPROJ, ctx, L.io, H, L.bo, prev_g(li), prev_b(li), L.g1, L.be1)) return r;
        if (int r = gemm(RS_K_FFN1, EPI_GELU_F16, true, h16, L.i1, rows, F, H, gelu_ep(L.b1, inter, 2), F)) return r;
        return split_block(RS_K_FFN2, inter, L.i2, F, L.b2, L.g1, L.be1, L.g2, L.be2);
    }

    // fp16 / K-concatenated fp16x3 full layer.  Each of its two residual blocks is a GEMM and a rows
    // pass; which pair closes it is o.oproj_f16 / o.lnres_defer, then o.lnres_defer / o.ffn2_f16.
    int layer_f16(int li, bool uq) {
        const Layer& L = m->layers[li];
        const float *pg = prev_g(li), *pb = prev_b(li);
        LAUNCH(RS_K_ATTN, launch_attention_full(qkv, q32, sm, c.s0, c.s1, 0, H, nh, ctx, kx, st, uq, c.max_len));
        // O-projection output (fp16): the dead QKV buffer when the BertOutput GEMM reads it
        // back (deferred residual: it must survive FFN1), else the (free) FFN1 buffer
        f16* o16 = o.lnres_defer ? (f16*)qkv : inter;
        if (!o.oproj_f16) {
            // residual rebuilt in the GEMM's accumulators, LayerNorm as a rows pass
            if (int r = gemm(RS_K_OPROJ, EPI_RESLN_F32, false, ctx, L.wo, rows, H, kx * H, resln_ep(L.bo, pg, pb), H))
                return r;
            LAUNCH_OTHER(launch_ln_rows(t32, rows, L.g1, L.be1, eps, H, nullptr, xst, h16, kx, st));
        } else {
            // O projection as a persistent fp16-output GEMM; the residual add + LayerNorm
            // move into ln_res_rows, off the GEMM's critical path
            if (int r = gemm(RS_K_OPROJ, EPI_BIAS_F16, false, ctx, L.wo, rows, H, H, bias_ep(L.bo, o16, H), H)) return r;
            if (o.lnres_defer)    // x = LN0(x32) + o1 is not written back: its statistics go to xst1
                LAUNCH_OTHER(launch_ln_res_rows(t32, xst, xst1, pg, pb, o16, rows, L.g1, L.be1, eps, H, h16, false, st));
            else
                LAUNCH_OTHER(launch_ln_res_rows(t32, xst, xst, pg, pb, o16, rows, L.g1, L.be1, eps, H, h16, true, st));
        }
        if (int r = gemm(RS_K_FFN1, EPI_GELU_F16, false, h16, L.w1, rows, F, kx * H, gelu_ep(L.b1, inter, kx), F)) return r;
        if (o.lnres_defer == 2) {
            // BertOutput as a persistent fp16-output GEMM into the (free) ctx buffer; both
            // residual blocks of the layer are closed by one ln_res_rows pass
            if (int r = gemm(RS_K_FFN2, EPI_BIAS_F16, false, inter, L.w2, rows, H, F, bias_ep(L.b2, ctx, H), H)) return r;
            LAUNCH_OTHER(launch_ln_res_rows(t32, xst, xst, pg, pb, o16, rows, L.g2, L.be2, eps, H, h16, true, st, xst1,
                                            L.g1, L.be1, ctx));
        } else if (o.ffn2_f16) {
            // same split for BertOutput: fp16-output GEMM into the (free) ctx buffer
            if (int r = gemm(RS_K_FFN2, EPI_BIAS_F16, false, inter, L.w2, rows, H, F, bias_ep(L.b2, ctx, H), H)) return r;
            LAUNCH_OTHER(launch_ln_res_rows(t32, xst, xst, L.g1, L.be1, ctx, rows, L.g2, L.be2, eps, H, h16, true, st));
        } else if (o.lnres_defer == 1) {
            // the GEMM rebuilds the post-attention stream from (x32, o1) in its accumulator init
            EpiArgs ep = resln_ep(L.b2, L.g1, L.be1);
            ep.res_stats = xst1; ep.res_o16 = o16; ep.res_stats0 = xst; ep.res_g0 = pg; ep.res_b0 = pb;
            if (int r = gemm(RS_K_FFN2, EPI_RESLN_F32, false, inter, L.w2, rows, H, kx * F, ep, H)) return r;
            LAUNCH_OTHER(launch_ln_rows(t32, rows, L.g2, L.be2, eps, H, nullptr, xst, h16, kx, st));
        } else {
            if (int r = gemm(RS_K_FFN2, EPI_RESLN_F32, false, inter, L.w2, rows, H, kx * F, resln_ep(L.b2, L.g1, L.be1), H))
                return r;
            LAUNCH_OTHER(launch_ln_rows(t32, rows, L.g2, L.be2, eps, H, nullptr, xst, h16, kx, st));
        }
        return RS_OK;
    }

    // The last layer (layer_query) runs folded (CallOpts.lastfold): single-query calls
    bool fold() const { return o.lastfold && !mq; }
    // Folded attention of the scored rows: G and U live in the QKV buffer, dead in this layer.  The
    // two fold GEMMs count as qkv (2 M N K each), the query kernel as attn.
    int attention_fold(const Layer& L) {
        AttnFold a{};
        a.himg = h16; a.tq = tq; a.wkf = L.wkf; a.wvt = L.wvt; a.bv = L.bqkv + 2 * H;
        a.sm = sm; a.s0 = c.s0; a.s1 = c.s1; a.row0 = 0; a.H = H; a.heads = nh; a.kx = kx;
        a.work = qkv; a.work_bytes = m->qkv.bytes; a.ctxq = ctxq; a.resq = resq;
        TRY_HIP(launch_attention_fold(a, st, [&](int kind, double flops, auto&& launch) {
            ProfScope ps(m, st, kind == 0 ? RS_K_QKV : RS_K_ATTN, flops);
            return launch();
        }));
        return RS_OK;
    }

    // Last layer of the scoring modes: only the scored rows (one per sequence, or one per query)
    int layer_query(int li, bool qrow) {
        const Layer& L = m->layers[li];
        if (fold()) {
            // RS_LASTQ=0: the scored rows' Q out of the full Q/K/V GEMM's output, which is dead from then on
            if (!qrow) LAUNCH_OTHER(launch_gather_q32((const float*)qkv, 3 * H, sm, c.s0, c.s1, 0, H, tq, st));
            if (int r = attention_fold(L)) return r;
        } else if (mq)
            LAUNCH(RS_K_ATTN, launch_attention_mquery(qkv, q32, t32, xst, prev_g(li), prev_b(li), sm, qm, c.s0, c.s1, H, nh,
                                                      ctxq, resq, kx, st, qrow ? tq : nullptr, o.imgres ? h16 : nullptr));
        else
            LAUNCH(RS_K_ATTN, launch_attention_query(qkv, q32, t32, xst, prev_g(li), prev_b(li), sm, c.s0, c.s1, 0, H, nh,
                                                     ctxq, resq, kx, st, qrow ? tq : nullptr, o.imgres ? h16 : nullptr));
        if (int r = gemm(RS_K_OPROJ, EPI_RES_F32, false, ctxq, L.wo, nr, H, kx * H, bias_ep(L.bo, tq, H, resq), H))
            return r;
        LAUNCH_OTHER(launch_ln_rows(tq, nr, L.g1, L.be1, eps, H, hq32, nullptr, hq16, kx, st));
        if (int r = gemm(RS_K_FFN1, EPI_GELU_F16, false, hq16, L.w1, nr, F, kx * H, gelu_ep(L.b1, interq, kx), F)) return r;
        if (int r = gemm(RS_K_FFN2, EPI_RES_F32, false, interq, L.w2, nr, H, kx * F, bias_ep(L.b2, tq, H, hq32), H))
            return r;
        LAUNCH_OTHER(launch_ln_rows(tq, nr, L.g2, L.be2, eps, H, hq32, nullptr, hq16, kx, st));
        return RS_OK;
    }

    int head_mlm() {
        if (int r = gemm(RS_K_DECODER, EPI_GELU_F32, false, hq16, m->wt, nr, H, kx * H, bias_ep(m->bt, tq, H), H)) return r;
        LAUNCH_OTHER(launch_ln_rows(tq, nr, m->gt, m->bet, eps, H, hq32, nullptr, hq16, kx, st));
        const MlmDecoder d{hq16, m->wdec, m->bdec, nr, m->vpad, cf.vocab, kx * H, call.d_tok, sm, r0, m->lab.as<int>(),
                           m->part.as<float2>(), m->llog.as<float>(), call.out_rows + r0, mq ? &qm : nullptr};
        if (call.cands) {
            // the only fork of a candidate call: the decoder launcher, over the chunk's queries' lists
            const CandLists& cl = *call.cands;
            const int t0 = cl.off[r0], n_c = cl.off[r0 + nr] - t0;
            const MlmCands cc{cl.d_off + r0, cl.d_id, cl.d_perm, t0, n_c, cl.d_logit, call.out_rows};
            TRY_HIP(launch_mlm_decoder_cands(d, cc, st, [&](bool is_gemm, auto&& launch) {
                ProfScope ps(m, st, is_gemm ? RS_K_DECODER : RS_K_OTHER, is_gemm ? 2.0 * nr * (double)cf.vocab * (kx * H) : 0);
                return launch();
            }));
            return RS_OK;
        }
        if (call.topk_k) {
            // the only fork of a top-k call: the decoder launcher (its GEMM runs in n_gemm sub-batches)
            const int k = call.topk_k, n_gemm = (ns + TOPK_SUB_ROWS - 1) / TOPK_SUB_ROWS;
            const MlmTopk t{k, m->topk_cand.as<float2>(), call.topk_id + (size_t)c.s0 * k, call.topk_lp + (size_t)c.s0 * k};
            TRY_HIP(launch_mlm_decoder_topk(d, t, st, [&](bool is_gemm, auto&& launch) {
                ProfScope ps(m, st, is_gemm ? RS_K_DECODER : RS_K_OTHER,
                             is_gemm ? 2.0 * ns * (double)cf.vocab * (kx * H) / n_gemm : 0);
                return launch();
            }));
            return RS_OK;
        }
        TRY_HIP(launch_mlm_decoder(d, st, [&](bool is_gemm, auto&& launch) {
            ProfScope ps(m, st, is_gemm ? RS_K_DECODER : RS_K_OTHER, is_gemm ? 2.0 * nr * (double)cf.vocab * (kx * H) : 0);
            return launch();
        }));
        return RS_OK;
    }
    int head_cls() {
        LAUNCH_OTHER(launch_cls_linear(hq32, ns, H, m->wlin, m->blin, call.out_rows + c.s0, st));
        return RS_OK;
    }
    int emb_out() {
        LAUNCH_OTHER(launch_embed_out(t32, xst, prev_g(cf.layers), prev_b(cf.layers), sm, c.s0, c.s1, 0, H, call.emb_dst,
                                      st, o.imgres ? h16 : nullptr, kx == 3));
        return RS_OK;
    }
    int run() {
        if (int r = embed()) return r;
        for (int li = 0; li < cf.layers; ++li) {
            const bool last = call.mode != MODE_EMB && li == cf.layers - 1;   // the scoring modes' last layer
            const bool uq = dedup && li == 0;
            const bool qrow = last && !uq && o.lastq;                     // query-row-only Q projection
            if (int r = qkv_proj(li, last, uq, qrow)) return r;
            if (int r = last ? layer_query(li, qrow) : o.x3s ? layer_split(li, uq) : layer_f16(li, uq)) return r;
        }
        if (call.mode == MODE_EMB) return emb_out();
        return call.mode == MODE_MLM ? head_mlm() : head_cls();
    }
};

int validate_call(const rs_model* m, int mode) {
    if (!m->finalized) return fail(RS_ESTATE, "rs_model_finalize not called");
    if (mode == MODE_MLM && !(m->cfg.heads_mask & RS_HEAD_MLM)) return fail(RS_ESTATE, "model has no MLM head");
    if (mode == MODE_CLS && !(m->cfg.heads_mask & RS_HEAD_CLS)) return fail(RS_ESTATE, "model has no CLS linear head");
    return RS_OK;
}

// Chunk rows: with the fused residual + LayerNorm GEMMs (lnfuse), a chunk of P row panels runs
// ceil(P / G) rounds of whole panels on G = gemm_lnres_workgroups / (H / 256) gangs, so the
// chunks are cut at a multiple of 256 * G rows (bert-base on 256 CUs: 85 gangs, 21760 rows;
// 262144 -> 261120 rows = 12 full rounds instead of 12 + a 4-panel 13th); RS_CHUNK_ALIGN=0: max_rows.
int64_t chunk_cap(const rs_model* m, const CallOpts& o) {
    int64_t cap = m->max_rows;
    const int ntn = m->cfg.hidden / 256;
    if (o.lnfuse && o.chunk_align && ntn > 0) {
        const int64_t unit = (int64_t)256 * (gemm_lnres_workgroups(m->cfg.hidden) / ntn);
        if (unit > 0 && cap >= unit) cap = cap / unit * unit;
    }
    return cap;
}

// Chunks of <= cap rows and <= s_cap sequences (ql: and <= s_cap queries); sets sl.row (first row
// of a sequence in its chunk).
int cut_chunks(const rs_model* m, SeqList& sl, const QueryList* ql, int64_t cap, std::vector<Chunk>* chunks) {
    for (int T : sl.len) {
        if (T > m->cfg.max_pos) return fail(RS_EUNSUP, "sequence longer than max_position_embeddings");
        if (T < 1) return fail(RS_EARG, "empty sequence");
        if (T > m->max_rows) return fail(RS_EARG, "sequence longer than the reserved rows");
    }
    if (!ql) {
        cut_rows(sl, cap, m->s_cap, chunks);
        return RS_OK;
    }
    // query-list call: a chunk's queries fit the per-query workspace (s_cap rows, as its sequences do)
    const int bad = cut_rows_queries(sl, *ql, cap, m->s_cap, chunks);
    if (bad >= 0)
        return fail(RS_EARG, "row " + std::to_string(bad) + " scores " + std::to_string(ql->count(bad)) +
                                 " positions, the reserved workspace holds " + std::to_string(m->s_cap) +
                                 " per launch: rs_model_reserve max_rows >= " +
                                 std::to_string(3 * ((int64_t)ql->count(bad) - 1)) + " would fit it");
    return RS_OK;
}

// Layer-0 dedup plan (seq_plan.h plan_unique_rows) of every chunk it applies to (call_opts: RS_DEDUP,
// x3_dedup) and whose unique rows fit the reserved rows (unique_rows_fit; else the chunk runs plain).
void plan_dedup(const rs_model* m, const CallOpts& o, int mode, SeqList& sl, std::vector<Chunk>& chunks) {
    if (!(o.dedup && mode == MODE_MLM && (m->kx == 1 || o.x3_dedup) && m->cfg.layers >= 2)) return;
    for (Chunk& c : chunks)
        if (m->kx == 1 || c.max_len <= 64)
            c.urows = unique_rows_fit(plan_unique_rows(sl, c.s0, c.s1), gemm_row_align(), m->m_pad);
}

// One upload of all metadata through the pinned staging buffer: the nine SeqList columns, then
// the call's extra ints (-> *call.d_extra), then the query list (call.ql -> *qm: first [S + 1],
// and seq, pos, label per query); call.d_label: device labels instead of the list's (per query
// with a query list, else per sequence).
int upload_meta(rs_model* m, hipStream_t st, const Call& call, const SeqList& sl, SeqMeta* sm, QueryMeta* qm) {
    const QueryList* ql = call.ql;
    const size_t S = sl.size(), n_extra = call.extra ? call.extra->size() : 0, Q = ql ? ql->size() : 0;
    const size_t n_seq_int = 9 * S + n_extra, n_int = n_seq_int + (ql ? S + 1 + 3 * Q : 0);
    TRY_HIP(m->stage_meta.begin(n_int));
    int* p = m->stage_meta.p;
    const std::vector<int>* cols[9] = {&sl.tok_off, &sl.len, &sl.mask, &sl.query, &sl.label, &sl.row,
                                       &sl.urow_h, &sl.urow_m, &sl.mask_end};
    for (int k = 0; k < 9; ++k) std::memcpy(p + k * S, cols[k]->data(), S * 4);
    if (n_extra) std::memcpy(p + 9 * S, call.extra->data(), n_extra * 4);
    if (ql) {
        int* q = p + n_seq_int;
        std::memcpy(q, ql->first.data(), (S + 1) * 4);
        int* seq = q + S + 1;
        for (size_t s = 0; s < S; ++s) std::fill(seq + ql->first[s], seq + ql->first[s + 1], (int)s);
        std::memcpy(seq + Q, ql->pos.data(), Q * 4);
        std::memcpy(seq + 2 * Q, ql->label.data(), Q * 4);
    }
    TRY_HIP(m->stage_meta.upload(m->meta, n_int, st));
    int* d = m->meta.as<int>();
    if (ql) {
        int* q = d + n_seq_int;
        *qm = QueryMeta{q, q + S + 1, q + S + 1 + Q, q + S + 1 + 2 * Q};
        if (call.d_label && Q)
            TRY_HIP(hipMemcpyAsync(q + S + 1 + 2 * Q, call.d_label, Q * 4, hipMemcpyDeviceToDevice, st));
    } else if (call.d_label) {
        TRY_HIP(hipMemcpyAsync(d + 4 * S, call.d_label, S * 4, hipMemcpyDeviceToDevice, st));
    }
    *sm = SeqMeta{d, d + S, d + 2 * S, d + 3 * S, d + 4 * S, d + 5 * S, d + 6 * S, d + 7 * S, d + 8 * S};
    if (call.d_extra) *call.d_extra = d + 9 * S;
    return RS_OK;
}

// Chunks the call's sequence list, uploads metadata, runs every chunk.
int run_all(rs_model* m, hipStream_t st, const Call& call, SeqList& sl) {
    const CallOpts opts = call_opts(m);
    if (int r = validate_call(m, call.mode)) return r;
    if (m->max_rows == 0)
        if (int r = reserve_impl(m, 65536)) return r;
    TRY_HIP(hipSetDevice(m->device));
    if (int r = begin_call(m, st)) return r;
    std::vector<Chunk> chunks;
    if (int r = cut_chunks(m, sl, call.ql, chunk_cap(m, opts), &chunks)) return r;
    if (!call.ql) plan_dedup(m, opts, call.mode, sl, chunks);   // query-list calls run layer 0 over all rows
    SeqMeta sm{};
    QueryMeta qm{};
    if (int r = upload_meta(m, st, call, sl, &sm, &qm)) return r;
    for (const Chunk& c : chunks) {
        ChunkCtx cx{m, st, call, sm, c, opts, qm};
        if (int r = cx.run()) return r;
    }
    return RS_OK;
}

// A top-k call: checks k and the outputs, makes sure of the candidate workspace and puts the
// request into the call (head_mlm then runs the top-k decoder form).
int topk_begin(rs_model* m, int k, int32_t* d_top_id, float* d_top_lp, Call* call) {
    if (!d_top_id || !d_top_lp) return fail(RS_EARG, "null argument");
    if (k < 1 || k > RS_TOPK_MAX) return fail(RS_EARG, "k must be 1 .. RS_TOPK_MAX (16)");
    if (k > m->cfg.vocab) return fail(RS_EARG, "k larger than the vocabulary");
    if (int r = validate_call(m, MODE_MLM)) return r;
    TRY_HIP(hipSetDevice(m->device));
    if (m->topk_cand.ensure(topk_cand_bytes(m->vpad)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RS_ENOMEM, "top-k candidate workspace (" + std::to_string(topk_cand_bytes(m->vpad)) + " bytes)");
    }
    call->topk_k = k; call->topk_id = d_top_id; call->topk_lp = d_top_lp;
    return RS_OK;
}

// A candidate call (rs_masked_logprob_cands) after its offsets are checked: validates the ids, sorts
// every query's list by (id, original index), uploads offsets, ids and permutation in one copy, and
// makes sure of the candidate-logit workspace: the most candidates any run of s_cap consecutive
// queries holds, which bounds every chunk (cut_rows_queries gives a chunk at most s_cap queries).
int cands_begin(rs_model* m, hipStream_t st, const int32_t* h_c_off, const int32_t* h_cand, int n_q, CandLists* cl) {
    const int n_c = h_c_off[n_q];
    cl->off.assign(h_c_off, h_c_off + n_q + 1);
    TRY_HIP(m->stage_cand.begin((size_t)n_q + 1 + 2 * (size_t)n_c));
    int* off = m->stage_cand.p;
    int *id = off + n_q + 1, *perm = id + n_c;
    std::memcpy(off, h_c_off, ((size_t)n_q + 1) * 4);
    for (int q = 0; q < n_q; ++q) {
        const int a = h_c_off[q], b = h_c_off[q + 1];
        for (int t = a; t < b; ++t) {
            if (h_cand[t] < 0 || h_cand[t] >= m->cfg.vocab)
                return fail(RS_EARG, "query " + std::to_string(q) + ": candidate " + std::to_string(t - a) + " is id " +
                                         std::to_string(h_cand[t]) + ", outside [0, " + std::to_string(m->cfg.vocab) + ")");
            perm[t] = t;
        }
        std::sort(perm + a, perm + b, [&](int x, int y) { return h_cand[x] != h_cand[y] ? h_cand[x] < h_cand[y] : x < y; });
        for (int t = a; t < b; ++t) id[t] = h_cand[perm[t]];
    }
    if (m->max_rows == 0)
        if (int r = reserve_impl(m, 65536)) return r;
    int most = 0;
    for (int q = 0; q < n_q; ++q) most = std::max(most, h_c_off[std::min<int64_t>((int64_t)q + m->s_cap, n_q)] - h_c_off[q]);
    if (m->cand_logit.ensure(std::max<size_t>(most, 1) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RS_ENOMEM, "candidate workspace (" + std::to_string((size_t)most * 4) + " bytes)");
    }
    TRY_HIP(m->stage_cand.upload(m->cand_meta, (size_t)n_q + 1 + 2 * (size_t)n_c, st));
    cl->d_off = m->cand_meta.as<int>();
    cl->d_id = cl->d_off + n_q + 1;
    cl->d_perm = cl->d_id + n_c;
    cl->d_logit = m->cand_logit.as<float>();
    return RS_OK;
}

// Held by every entry point that runs the encoder, from its first line: whatever the entry returns
// (argument errors and empty calls included), the segment ids left by rs_model_set_token_types are
// dropped with it, so the setting never outlives one call.  take: they must cover the call's n_tok
// tokens; the call gets the pointer.
struct PendingTypes {
    rs_model* m;
    explicit PendingTypes(rs_model* m_) : m(m_) {}
    ~PendingTypes() {
        if (m) { m->type_next = nullptr; m->type_n = 0; }
    }
    int take(int64_t n_tok, Call* call) {
        if (!m->type_next) return RS_OK;
        if (m->type_n != n_tok)
            return fail(RS_EARG, "rs_model_set_token_types gave " + std::to_string(m->type_n) +
                                     " token types, this call addresses " + std::to_string(n_tok) + " tokens");
        call->d_type = m->type_next;
        return RS_OK;
    }
};

// ---- sequence lists of the entry points --------------------------------------------------
// rs_masked_logprob / rs_masked_topk: the caller's rows (ids already masked) with a query position
// each; label column 0: the call's device labels replace it, or its log-prob is unused (top-k).
int rows_query(const int32_t* h_seq_off, const int32_t* h_query, int n_seq, SeqList& sl) {
    for (int s = 0; s < n_seq; ++s) {
        const int o = h_seq_off[s], T = h_seq_off[s + 1] - o;
        if (h_query[s] < 0 || h_query[s] >= T) return fail(RS_EARG, "query position outside its sequence");
        sl.push(o, T, -1, -1, h_query[s], 0);
    }
    return RS_OK;
}
// rs_cls_score / token_embed: whole hypotheses with the query at [CLS] (RescoreBert/model.py:19);
// check(h, o, T): the entry's own test of a hypothesis (its error, or 0).
template <class Check>
int rows_whole(const int32_t* h_hyp_off, int n_hyp, SeqList& sl, Check&& check) {
    for (int h = 0; h < n_hyp; ++h) {
        const int o = h_hyp_off[h], T = h_hyp_off[h + 1] - o;
        if (int r = check(h, o, T)) return r;
        sl.push(o, T, -1, -1, 0, 0);
    }
    return RS_OK;
}

// End of the PLL entries: the rows' buffer (the caller's, else rowlp_tmp), the run, the
// float64 sum per hypothesis when d_pll is given, then the finite checks of every output.
// One output row per sequence, or (call.ql) per query; hso counts the same.
int pll_tail(rs_model* m, hipStream_t st, Call& call, SeqList& sl, const std::vector<int>& hso, int n_hyp,
             double* d_pll, float* d_row_lp) {
    float* rows = d_row_lp;
    const size_t n_out = call.ql ? call.ql->size() : sl.size();
    if (!rows) {
        TRY_HIP(m->rowlp_tmp.ensure(std::max<size_t>(n_out, 1) * 4));
        rows = m->rowlp_tmp.as<float>();
    }
    int* d_hso = nullptr;
    call.out_rows = rows; call.extra = &hso; call.d_extra = &d_hso;
    if (int r = run_all(m, st, call, sl)) return r;
    if (d_pll) LAUNCH_OTHER(launch_segsum_f64(rows, d_hso, n_hyp, d_pll, st));
    if (!call.topk_k) return check_finite(m, st, rows, n_out, "masked-token log-probability");
    if (int r = mark_nonfinite(m, st, rows, sl.size())) return r;
    return check_finite(m, st, call.topk_lp, sl.size() * call.topk_k, "masked-token or top-k log-probability");
}

// Opening of the multi-mask entries: the model can run a query-list call (MLM head; the query-row
// layer is not layer 0).
int validate_sets(const rs_model* m) {
    if (int r = validate_call(m, MODE_MLM)) return r;
    if (m->cfg.layers < 2) return fail(RS_EUNSUP, "multi-mask rows need a model of at least 2 layers");
    return RS_OK;
}
// an offsets array [n + 1]: starts at 0, never descends
int offsets_ok(const int32_t* off, int n, const char* name) {
    if (off[0] != 0) return fail(RS_EARG, std::string(name) + "[0] must be 0");
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(RS_EARG, std::string(name) + " not ascending at " + std::to_string(i));
    return RS_OK;
}
std::string positions_text(const int32_t* p, int n) {
    std::string t;
    for (int i = 0; i < n && i < 8; ++i) t += (i ? ", " : "") + std::to_string(p[i]);
    return n > 8 ? t + ", ..." : t;
}

// rs_pll_score / rs_pll_topk after their argument checks: every word position of every hypothesis
// masked in turn (the do_job rows, p = mask_pos); hso: hypothesis -> first sequence.
int pll_words(rs_model* m, hipStream_t st, PendingTypes& ty, Call& call, const int32_t* h_hyp_off, int n_hyp,
              double* d_pll, float* d_row_lp) {
    if (n_hyp == 0) return RS_OK;
    if (int r = ty.take(h_hyp_off[n_hyp], &call)) return r;
    CALL_ORDER(m, st);
    SeqList sl;
    std::vector<int> hso(n_hyp + 1, 0);
    for (int h = 0; h < n_hyp; ++h) {
        const int o = h_hyp_off[h], T = h_hyp_off[h + 1] - o;
        if (T < 3) return fail(RS_EARG, "hypothesis " + std::to_string(h) + " has no word (T < 3)");
        for (int p = 1; p <= T - 2; ++p) sl.push(o, T, p, p + 1, p, -1);
        hso[h + 1] = (int)sl.size();
    }
    return pll_tail(m, st, call, sl, hso, n_hyp, d_pll, d_row_lp);
}

// rs_token_embed, and the first half of rs_bertscore_recall: the L2-normalised last hidden state of
// every token of the hypotheses into d_emb.  call: MODE_EMB with the caller's tokens and segment ids.
int token_embed(rs_model* m, hipStream_t st, Call& call, const int32_t* h_hyp_off, int n_hyp, void* d_emb) {
    SeqList sl;
    if (int r = rows_whole(h_hyp_off, n_hyp, sl, [](int h, int o, int T) {
            return o < 0 || T < 1 ? fail(RS_EARG, "hypothesis " + std::to_string(h) + " is empty") : RS_OK;
        }))
        return r;
    call.emb_dst = (f16*)d_emb;
    if (int r = run_all(m, st, call, sl)) return r;
    // every token row of the hypotheses (contiguous from h_hyp_off[0]) is written
    const size_t W = (size_t)m->cfg.hidden * (m->kx == 3 ? 2 : 1);
    return check_finite(m, st, (const f16*)d_emb + (size_t)h_hyp_off[0] * W,
                        (size_t)(h_hyp_off[n_hyp] - h_hyp_off[0]) * W, "token embedding");
}

void prof_collect(rs_model* m) {
    if (m->recs.empty()) return;
    (void)hipEventSynchronize(m->recs.back().b);
    for (auto& r : m->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            m->prof_ms[r.kind] += ms;
            m->prof_n[r.kind] += 1;
            m->prof_flops[r.kind] += r.flops;
        }
    }
    m->recs.clear();
    m->ev_used = 0;
}

}  // namespace

// =======================================================================================
extern "C" {

int rs_version(void) { return 1; }

const char* rs_last_error(void) { return g_err.c_str(); }

int rs_model_create(const rs_bert_cfg* cfg, int device, rs_model** out) {
    if (!cfg || !out) return fail(RS_EARG, "null argument");
    const rs_bert_cfg& c = *cfg;
    if (int r = check_bert_shape(c, 128)) return r;
    if (!(c.heads_mask & (RS_HEAD_MLM | RS_HEAD_CLS | RS_HEAD_EMB))) return fail(RS_EARG, "heads_mask selects no head");
    if (int r = check_device(device)) return r;
    rs_model* m = new (std::nothrow) rs_model();
    if (!m) return fail(RS_ENOMEM, "alloc");
    m->cfg = c;
    m->device = device;
    if (c.precision != RS_PREC_FP16 && c.precision != RS_PREC_FP16X3) {
        delete m;
        return fail(RS_EARG, "unknown precision");
    }
    m->kx = c.precision == RS_PREC_FP16X3 ? 3 : 1;
    *out = m;
    return RS_OK;
}

int rs_model_set_tensor(rs_model* m, const char* key, const void* host_ptr, int dtype,
                        const int64_t* shape, int ndim) {
    if (!m || !key || !host_ptr || (ndim > 0 && !shape)) return fail(RS_EARG, "null argument");
    if (dtype != RS_DT_F32) return fail(RS_EUNSUP, "only float32 tensors are accepted");
    if (m->finalized) return fail(RS_ESTATE, "model already finalized");
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) return fail(RS_EARG, "negative dim");
        n *= shape[i];
    }
    std::vector<float> v((size_t)n);
    std::memcpy(v.data(), host_ptr, (size_t)n * 4);
    m->host[key] = std::move(v);
    return RS_OK;
}

int rs_model_finalize(rs_model* m) {
    if (!m) return fail(RS_EARG, "null model");
    if (m->finalized) return RS_OK;
    TRY_HIP(hipSetDevice(m->device));
    const rs_bert_cfg& c = m->cfg;
    const size_t H = c.hidden, F = c.intermediate, V = c.vocab;
    std::string miss;
    const std::string e = "bert.embeddings.";
    auto* word = need(m, e + "word_embeddings.weight", V * H, &miss);
    auto* pos = need(m, e + "position_embeddings.weight", (size_t)c.max_pos * H, &miss);
    auto* typ = need(m, e + "token_type_embeddings.weight", (size_t)c.type_vocab * H, &miss);
    auto* eg = need(m, e + "LayerNorm.weight", H, &miss);
    auto* eb = need(m, e + "LayerNorm.bias", H, &miss);
    if (!miss.empty()) return fail(RS_ESTATE, "tensor " + miss);
    hipError_t err = hipSuccess;
#define UP32(dst, src, n) do { dst = upload_f32(m, *(src), (n), &err); if (err != hipSuccess) return fail(RS_EHIP, "upload"); } while (0)
#define UP16(dst, src, rp, cols) do {                                                                             \
        if (!fp16_range_ok(*(src)))                                                                             \
            return fail(RS_EUNSUP, std::string("weight '") + #src + "' has a value outside the fp16 range "    \
                                   "(|w| > 65504) of the GEMM operand images");                              \
        dst = upload_f16(m, *(src), (rp), (cols), m->kx, &err);                                                 \
        if (err != hipSuccess) return fail(RS_EHIP, "upload");                                                 \
    } while (0)
    UP32(m->word32, word, V * H);
    UP32(m->pos32, pos, (size_t)c.max_pos * H);
    UP32(m->type32, typ, (size_t)c.type_vocab * H);   // row 0 alone without segment ids (modeling_bert.py:88-94)
    UP32(m->eg, eg, H);
    UP32(m->eb, eb, H);
    m->layers.resize(c.layers);
    // fp16x3: the split-operand GEMMs' interleaved weight images, when every projection weight
    // keeps 64 W_hi finite (x3s_range_ok); else the K-concatenated form runs every layer
    bool x3s_w = m->kx == 3;
    for (int i = 0; i < c.layers && x3s_w; ++i) {
        const std::string p = "bert.encoder.layer." + std::to_string(i) + ".";
        for (const char* k : {"attention.self.query.weight", "attention.self.key.weight", "attention.self.value.weight",
                              "attention.output.dense.weight", "intermediate.dense.weight", "output.dense.weight"}) {
            auto it = m->host.find(p + k);
            if (it != m->host.end() && !x3s_range_ok(it->second)) x3s_w = false;
        }
    }
#define UPIL(dst, src, cols) do { dst = upload_il(m, *(src), (cols), &err); if (err != hipSuccess) return fail(RS_EHIP, "upload"); } while (0)
    for (int i = 0; i < c.layers; ++i) {
        const std::string p = "bert.encoder.layer." + std::to_string(i) + ".";
        auto* wq = need(m, p + "attention.self.query.weight", H * H, &miss);
        auto* bq = need(m, p + "attention.self.query.bias", H, &miss);
        auto* wk = need(m, p + "attention.self.key.weight", H * H, &miss);
        auto* bk = need(m, p + "attention.self.key.bias", H, &miss);
        auto* wv = need(m, p + "attention.self.value.weight", H * H, &miss);
        auto* bv = need(m, p + "attention.self.value.bias", H, &miss);
        auto* wo = need(m, p + "attention.output.dense.weight", H * H, &miss);
        auto* bo = need(m, p + "attention.output.dense.bias", H, &miss);
        auto* g1 = need(m, p + "attention.output.LayerNorm.weight", H, &miss);
        auto* be1 = need(m, p + "attention.output.LayerNorm.bias", H, &miss);
        auto* w1 = need(m, p + "intermediate.dense.weight", F * H, &miss);
        auto* b1 = need(m, p + "intermediate.dense.bias", F, &miss);
        auto* w2 = need(m, p + "output.dense.weight", H * F, &miss);
        auto* b2 = need(m, p + "output.dense.bias", H, &miss);
        auto* g2 = need(m, p + "output.LayerNorm.weight", H, &miss);
        auto* be2 = need(m, p + "output.LayerNorm.bias", H, &miss);
        if (!miss.empty()) return fail(RS_ESTATE, "tensor " + miss);
        std::vector<float> wqkv, bqkv;
        wqkv.reserve(3 * H * H);
        for (auto* w : {wq, wk, wv}) wqkv.insert(wqkv.end(), w->begin(), w->end());
        for (auto* b : {bq, bk, bv}) bqkv.insert(bqkv.end(), b->begin(), b->end());
        Layer& L = m->layers[i];
        UP16(L.wqkv, &wqkv, 3 * H, H);
        UP32(L.bqkv, &bqkv, 3 * H);
        UP16(L.wo, wo, H, H);
        UP32(L.bo, bo, H);
        UP32(L.g1, g1, H);
        UP32(L.be1, be1, H);
        UP16(L.w1, w1, F, H);
        UP32(L.b1, b1, F);
        UP16(L.w2, w2, H, F);
        UP32(L.b2, b2, H);
        UP32(L.g2, g2, H);
        UP32(L.be2, be2, H);
        if (x3s_w && i == c.layers - 1 && attention_fold_ok((int)H, c.heads)) {
            // folded last-layer attention (RS_LASTFOLD): Wk / 8 (exact: the softmax scale of head_dim 64)
            // and Wv transposed, fp32
            std::vector<float> wkf(H * H), wvt(H * H);
            for (size_t r = 0; r < H; ++r)
                for (size_t j = 0; j < H; ++j) {
                    wkf[r * H + j] = (*wk)[r * H + j] * 0.125f;
                    wvt[j * H + r] = (*wv)[r * H + j];
                }
            UP32(L.wkf, &wkf, H * H);
            UP32(L.wvt, &wvt, H * H);
        }
        if (x3s_w) {
            UPIL(L.iqkv, &wqkv, H);
            UPIL(L.io, wo, H);
            UPIL(L.i1, w1, H);
            UPIL(L.i2, w2, F);
        }
    }
#undef UPIL
    m->x3s_w = x3s_w;
    if (c.heads_mask & RS_HEAD_MLM) {
        const std::string p = "cls.predictions.";
        auto* wt = need(m, p + "transform.dense.weight", H * H, &miss);
        auto* bt = need(m, p + "transform.dense.bias", H, &miss);
        auto* gt = need(m, p + "transform.LayerNorm.weight", H, &miss);
        auto* bet = need(m, p + "transform.LayerNorm.bias", H, &miss);
        auto* bd = need(m, p + "bias", V, &miss);
        if (!miss.empty()) return fail(RS_ESTATE, "tensor " + miss);
        // decoder weight is tied to the word embeddings (BertForMaskedLM._tied_weights_keys);
        // an explicitly provided cls.predictions.decoder.weight must equal it.
        auto it = m->host.find(p + "decoder.weight");
        const std::vector<float>* dec = word;
        if (it != m->host.end()) {
            if (it->second.size() != V * H) return fail(RS_EARG, "decoder.weight has wrong size");
            dec = &it->second;
        }
        m->vpad = (int)((V + 127) / 128 * 128);
        UP16(m->wt, wt, H, H);
        UP32(m->bt, bt, H);
        UP32(m->gt, gt, H);
        UP32(m->bet, bet, H);
        UP16(m->wdec, dec, (size_t)m->vpad, H);
        UP32(m->bdec, bd, (size_t)m->vpad);
    }
    if (c.heads_mask & RS_HEAD_CLS) {
        auto* wl = need(m, "linear.weight", H, &miss);
        auto* bl = need(m, "linear.bias", 1, &miss);
        if (!miss.empty()) return fail(RS_ESTATE, "tensor " + miss);
        UP32(m->wlin, wl, H);
        UP32(m->blin, bl, 1);
    }
#undef UP32
#undef UP16
    if (!m->call_done) TRY_HIP(hipEventCreateWithFlags(&m->call_done, hipEventDisableTiming));
    m->host.clear();
    m->finalized = true;
    return RS_OK;
}

int rs_model_reserve(rs_model* m, int64_t max_rows) {
    if (!m) return fail(RS_EARG, "null model");
    if (!m->finalized) return fail(RS_ESTATE, "rs_model_finalize not called");
    return reserve_impl(m, max_rows);
}

int rs_pll_score(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                 double* d_pll, float* d_row_lp, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_hyp_off || n_hyp < 0 || (n_hyp > 0 && (!d_tok || !d_pll))) return fail(RS_EARG, "null argument");
    Call call{MODE_MLM, d_tok};
    return pll_words(m, (hipStream_t)stream, ty, call, h_hyp_off, n_hyp, d_pll, d_row_lp);
}

int rs_pll_score_spans(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                       const int32_t* h_row_off, const int32_t* h_lo, const int32_t* h_hi, const int32_t* h_query,
                       double* d_pll, float* d_row_lp, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_hyp_off || !h_row_off || n_hyp < 0 || (n_hyp > 0 && (!d_tok || !d_pll)))
        return fail(RS_EARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (n_hyp == 0) return RS_OK;
    if (h_row_off[0] != 0) return fail(RS_EARG, "row_off[0] must be 0");
    for (int h = 0; h < n_hyp; ++h)
        if (h_row_off[h + 1] < h_row_off[h]) return fail(RS_EARG, "row_off not ascending at hypothesis " + std::to_string(h));
    if (h_row_off[n_hyp] > 0 && (!h_lo || !h_hi || !h_query)) return fail(RS_EARG, "null argument");
    Call call{MODE_MLM, d_tok};
    if (int r = ty.take(h_hyp_off[n_hyp], &call)) return r;
    CALL_ORDER(m, st);
    SeqList sl;
    std::vector<int> hso(h_row_off, h_row_off + n_hyp + 1);     // one sequence per row
    for (int h = 0; h < n_hyp; ++h) {
        const int o = h_hyp_off[h], T = h_hyp_off[h + 1] - o;
        for (int r = h_row_off[h]; r < h_row_off[h + 1]; ++r) {
            if (!span_ok(T, h_lo[r], h_hi[r], h_query[r]))
                return fail(RS_EARG, "row " + std::to_string(r) + " (hypothesis " + std::to_string(h) + ", T = " +
                                         std::to_string(T) + "): need 1 <= lo <= query < hi <= T - 1, got lo " +
                                         std::to_string(h_lo[r]) + ", hi " + std::to_string(h_hi[r]) + ", query " +
                                         std::to_string(h_query[r]));
            sl.push(o, T, h_lo[r], h_hi[r], h_query[r], -1);
        }
    }
    return pll_tail(m, st, call, sl, hso, n_hyp, d_pll, d_row_lp);
}

int rs_pll_score_sets(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                      const int32_t* h_row_off, const int32_t* h_pos_off, const int32_t* h_pos, double* d_pll,
                      float* d_pos_lp, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_hyp_off || !h_row_off || n_hyp < 0 || (n_hyp > 0 && (!d_tok || !d_pll)))
        return fail(RS_EARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (n_hyp == 0) return RS_OK;
    if (int r = validate_sets(m)) return r;
    if (int r = offsets_ok(h_row_off, n_hyp, "row_off")) return r;
    const int n_rows = h_row_off[n_hyp];
    if (n_rows > 0 && (!h_pos_off || !h_pos)) return fail(RS_EARG, "null argument");
    if (n_rows > 0)
        if (int r = offsets_ok(h_pos_off, n_rows, "pos_off")) return r;
    Call call{MODE_MLM, d_tok};
    if (int r = ty.take(h_hyp_off[n_hyp], &call)) return r;
    CALL_ORDER(m, st);
    SeqList sl;
    QueryList ql;
    ql.masked = true;
    std::vector<int> hso(n_hyp + 1, 0);                         // hypothesis -> first query
    for (int h = 0; h < n_hyp; ++h) {
        const int o = h_hyp_off[h], T = h_hyp_off[h + 1] - o;
        for (int r = h_row_off[h]; r < h_row_off[h + 1]; ++r) {
            const int32_t* p = h_pos + h_pos_off[r];
            const int n = h_pos_off[r + 1] - h_pos_off[r];
            if (!positions_ok(p, n, 1, T - 2))
                return fail(RS_EARG, "row " + std::to_string(r) + " (hypothesis " + std::to_string(h) + ", T = " +
                                         std::to_string(T) + "): need at least one position, strictly ascending, "
                                         "1 <= p <= T - 2, got " + std::to_string(n) + " [" + positions_text(p, n) + "]");
            sl.push(o, T, -1, -1, 0, -1);
            ql.push(p, n, -1);
        }
        hso[h + 1] = (int)ql.size();
    }
    call.ql = &ql;
    return pll_tail(m, st, call, sl, hso, n_hyp, d_pll, d_pos_lp);
}

int rs_masked_logprob_multi(rs_model* m, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                            const int32_t* h_q_off, const int32_t* h_qpos, const int32_t* d_label, float* d_out,
                            void* stream) {
    PendingTypes ty(m);
    if (!m || !h_seq_off || !h_q_off || n_seq < 0 || (n_seq > 0 && !d_ids)) return fail(RS_EARG, "null argument");
    if (n_seq == 0) return RS_OK;
    if (int r = validate_sets(m)) return r;
    if (int r = offsets_ok(h_q_off, n_seq, "q_off")) return r;
    // (no query at all: the first row is reported below, whatever the query arrays are)
    if (h_q_off[n_seq] > 0 && (!h_qpos || !d_label || !d_out)) return fail(RS_EARG, "null argument");
    Call call{MODE_MLM, d_ids, d_out, d_label};
    if (int r = ty.take(h_seq_off[n_seq], &call)) return r;
    hipStream_t st = (hipStream_t)stream;
    CALL_ORDER(m, st);
    SeqList sl;
    QueryList ql;
    for (int s = 0; s < n_seq; ++s) {
        const int o = h_seq_off[s], T = h_seq_off[s + 1] - o;
        const int n = h_q_off[s + 1] - h_q_off[s];
        const int32_t* p = n ? h_qpos + h_q_off[s] : nullptr;
        if (!positions_ok(p, n, 0, T - 1))
            return fail(RS_EARG, "row " + std::to_string(s) + " (T = " + std::to_string(T) +
                                     "): need at least one query position, strictly ascending, 0 <= p < T, got " +
                                     std::to_string(n) + " [" + positions_text(p, n) + "]");
        sl.push(o, T, -1, -1, 0, 0);
        ql.push(p, n, 0);
    }
    call.ql = &ql;
    if (int r = run_all(m, st, call, sl)) return r;
    return check_finite(m, st, d_out, ql.size(), "masked-token log-probability");
}

int rs_masked_logprob_cands(rs_model* m, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                            const int32_t* h_q_off, const int32_t* h_qpos, const int32_t* h_c_off, const int32_t* h_cand,
                            float* d_out, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_seq_off || !h_q_off || n_seq < 0 || (n_seq > 0 && !d_ids)) return fail(RS_EARG, "null argument");
    if (n_seq == 0) return RS_OK;
    if (int r = validate_sets(m)) return r;
    if (int r = offsets_ok(h_q_off, n_seq, "q_off")) return r;
    const int n_q = h_q_off[n_seq];
    if (n_q > 0 && (!h_qpos || !h_c_off)) return fail(RS_EARG, "null argument");
    if (n_q > 0)
        if (int r = offsets_ok(h_c_off, n_q, "c_off")) return r;
    const int n_c = n_q > 0 ? h_c_off[n_q] : 0;
    if (n_c > 0 && (!h_cand || !d_out)) return fail(RS_EARG, "null argument");
    Call call{MODE_MLM, d_ids, d_out};
    if (int r = ty.take(h_seq_off[n_seq], &call)) return r;
    hipStream_t st = (hipStream_t)stream;
    CALL_ORDER(m, st);
    SeqList sl;
    QueryList ql;
    for (int s = 0; s < n_seq; ++s) {
        const int o = h_seq_off[s], T = h_seq_off[s + 1] - o;
        const int n = h_q_off[s + 1] - h_q_off[s];
        const int32_t* p = n ? h_qpos + h_q_off[s] : nullptr;
        if (!positions_ok(p, n, 0, T - 1))
            return fail(RS_EARG, "row " + std::to_string(s) + " (T = " + std::to_string(T) +
                                     "): need at least one query position, strictly ascending, 0 <= p < T, got " +
                                     std::to_string(n) + " [" + positions_text(p, n) + "]");
        sl.push(o, T, -1, -1, 0, 0);
        ql.push(p, n, 0);
    }
    CandLists cl;
    if (int r = cands_begin(m, st, h_c_off, h_cand, n_q, &cl)) return r;
    call.ql = &ql;
    call.cands = &cl;
    if (int r = run_all(m, st, call, sl)) return r;
    return check_finite(m, st, d_out, (size_t)n_c, "masked-token log-probability");
}

int rs_masked_logprob(rs_model* m, const int32_t* d_ids, const int32_t* h_seq_off,
                      const int32_t* h_query, const int32_t* d_label, int32_t n_seq, float* d_out,
                      void* stream) {
    PendingTypes ty(m);
    if (!m || !h_seq_off || !h_query || n_seq < 0 || (n_seq > 0 && (!d_ids || !d_label || !d_out)))
        return fail(RS_EARG, "null argument");
    if (n_seq == 0) return RS_OK;
    Call call{MODE_MLM, d_ids, d_out, d_label};
    if (int r = ty.take(h_seq_off[n_seq], &call)) return r;
    hipStream_t st = (hipStream_t)stream;
    CALL_ORDER(m, st);
    SeqList sl;
    if (int r = rows_query(h_seq_off, h_query, n_seq, sl)) return r;
    if (int r = run_all(m, st, call, sl)) return r;
    return check_finite(m, st, d_out, (size_t)n_seq, "masked-token log-probability");
}

int rs_masked_topk(rs_model* m, const int32_t* d_ids, const int32_t* h_seq_off, const int32_t* h_query,
                   int32_t n_seq, int32_t k, int32_t* d_top_id, float* d_top_lp, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_seq_off || !h_query || n_seq < 0 || (n_seq > 0 && !d_ids)) return fail(RS_EARG, "null argument");
    Call call{MODE_MLM, d_ids};
    if (int r = topk_begin(m, k, d_top_id, d_top_lp, &call)) return r;
    if (n_seq == 0) return RS_OK;
    if (int r = ty.take(h_seq_off[n_seq], &call)) return r;
    hipStream_t st = (hipStream_t)stream;
    CALL_ORDER(m, st);
    SeqList sl;
    if (int r = rows_query(h_seq_off, h_query, n_seq, sl)) return r;
    TRY_HIP(m->rowlp_tmp.ensure(sl.size() * 4));
    call.out_rows = m->rowlp_tmp.as<float>();
    if (int r = run_all(m, st, call, sl)) return r;
    return check_finite(m, st, d_top_lp, (size_t)n_seq * k, "top-k log-probability");
}

int rs_pll_topk(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp, int32_t k,
                double* d_pll, float* d_row_lp, int32_t* d_top_id, float* d_top_lp, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_hyp_off || n_hyp < 0 || (n_hyp > 0 && !d_tok)) return fail(RS_EARG, "null argument");
    Call call{MODE_MLM, d_tok};
    if (int r = topk_begin(m, k, d_top_id, d_top_lp, &call)) return r;
    return pll_words(m, (hipStream_t)stream, ty, call, h_hyp_off, n_hyp, d_pll, d_row_lp);
}

int rs_cls_score(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                 float* d_out, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_hyp_off || n_hyp < 0 || (n_hyp > 0 && (!d_tok || !d_out))) return fail(RS_EARG, "null argument");
    if (n_hyp == 0) return RS_OK;
    Call call{MODE_CLS, d_tok, d_out};
    if (int r = ty.take(h_hyp_off[n_hyp], &call)) return r;
    hipStream_t st = (hipStream_t)stream;
    CALL_ORDER(m, st);
    SeqList sl;
    if (int r = rows_whole(h_hyp_off, n_hyp, sl,
                           [](int, int, int T) { return T < 1 ? fail(RS_EARG, "empty hypothesis") : RS_OK; }))
        return r;
    if (int r = run_all(m, st, call, sl)) return r;
    return check_finite(m, st, d_out, (size_t)n_hyp, "RescoreBert score");
}

int rs_token_embed(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                   void* d_emb, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_hyp_off || n_hyp < 0 || (n_hyp > 0 && (!d_tok || !d_emb))) return fail(RS_EARG, "null argument");
    if (n_hyp == 0) return RS_OK;
    Call call{MODE_EMB, d_tok};
    if (int r = ty.take(h_hyp_off[n_hyp], &call)) return r;
    CALL_ORDER(m, (hipStream_t)stream);
    return token_embed(m, (hipStream_t)stream, call, h_hyp_off, n_hyp, d_emb);
}

// The recall launch over an embedding buffer: the plan (bertscore_plan.h: runs of whole ref
// hypotheses fitting one COLS-column tile, a longer one alone), one upload through `stage` into
// `plan`, the kernel.  m: the model whose profile records the launch, or null.
static int recall_launch(rs_model* m, Staging& stage, DevBuf& plan, const f16* emb, int H, bool two,
                         const int32_t* h_hyp_off, const int32_t* h_utt_off, int n_utt, float* d_rmat, float* d_rmat0,
                         hipStream_t st) {
    const int n_hyp = h_utt_off[n_utt];
    BertscorePlan bp;
    plan_bertscore_items(h_hyp_off, h_utt_off, n_utt, bertscore_cols(two), &bp);
    const BertscoreUpload w = bertscore_upload_layout(bp, n_hyp, n_utt);
    TRY_HIP(stage.begin(w.n_int));
    bertscore_upload_pack(bp, w, h_hyp_off, h_utt_off, n_hyp, n_utt, stage.p);
    TRY_HIP(stage.upload(plan, w.n_int, st));
    const int* d = plan.as<int>();
    auto go = [&] {
        return launch_bertscore_recall(emb, H, d + w.hyp_off, d + w.utt_off, (const long long*)(d + w.moff),
                                       (const int4*)(d + w.items), bp.n_items(), d_rmat, d_rmat0, st, two);
    };
    if (m) LAUNCH_OTHER(go());
    else TRY_HIP(go());
    return RS_OK;
}

int rs_bertscore_recall(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off,
                        const int32_t* h_utt_off, int32_t n_utt, float* d_rmat, float* d_rmat0, void* stream) {
    PendingTypes ty(m);
    if (!m || !h_hyp_off || !h_utt_off || n_utt < 0 || (n_utt > 0 && (!d_tok || !d_rmat)))
        return fail(RS_EARG, "null argument");
    if (n_utt == 0) return RS_OK;
    const std::string bad = bertscore_layout_error(h_hyp_off, h_utt_off, n_utt);
    if (!bad.empty()) return fail(RS_EARG, bad);
    const int n_hyp = h_utt_off[n_utt];
    hipStream_t st = (hipStream_t)stream;
    CALL_ORDER(m, st);
    const int H = m->cfg.hidden;
    const size_t n_tok = (size_t)h_hyp_off[n_hyp];
    const bool two = m->kx == 3;                 // fp16x3: two-part embeddings, split-operand cosines
    TRY_HIP(m->emb.ensure(std::max<size_t>(n_tok, 1) * H * 2 * (two ? 2 : 1)));
    if (n_hyp > 0) {
        Call call{MODE_EMB, d_tok};
        if (int r = ty.take(h_hyp_off[n_hyp], &call)) return r;
        if (int r = token_embed(m, st, call, h_hyp_off, n_hyp, m->emb.p)) return r;
    }
    return recall_launch(m, m->stage_plan, m->plan, m->emb.as<f16>(), H, two, h_hyp_off, h_utt_off, n_utt, d_rmat,
                         d_rmat0, st);
}

// Test entry (not part of the scoring path): the recall kernel on the caller's embedding buffer
// d_emb [hyp_off[n_hyp], H] fp16, or (two != 0) the planar two-part image [.., 2H] — the layout
// checks, the plan, the upload and the launch of rs_bertscore_recall without its encoder.
// Synchronises the stream before it returns (the plan buffers are the call's own).
int rs_debug_bertscore_recall(const void* d_emb, int32_t H, int32_t two, const int32_t* h_hyp_off,
                              const int32_t* h_utt_off, int32_t n_utt, float* d_rmat, float* d_rmat0, void* stream) {
    if (!h_hyp_off || !h_utt_off || n_utt < 0 || (n_utt > 0 && (!d_emb || !d_rmat)))
        return fail(RS_EARG, "null argument");
    if (H <= 0 || H % 256 || H > 1024) return fail(RS_EUNSUP, "hidden must be 256/512/768/1024");
    if (n_utt == 0) return RS_OK;
    const std::string bad = bertscore_layout_error(h_hyp_off, h_utt_off, n_utt);
    if (!bad.empty()) return fail(RS_EARG, bad);
    hipStream_t st = (hipStream_t)stream;
    Staging stage;
    DevBuf plan;
    const int r = recall_launch(nullptr, stage, plan, (const f16*)d_emb, H, two != 0, h_hyp_off, h_utt_off, n_utt,
                                d_rmat, d_rmat0, st);
    const hipError_t e = hipStreamSynchronize(st);
    plan.release();
    if (r) return r;
    TRY_HIP(e);
    return RS_OK;
}

// Test entry (host only, no GPU call): plan_unique_rows (seq_plan.h) on the caller's host arrays
// tok_off / len / mask / mask_end [n_seq] for the chunk [s0, s1).  Fills urow_h / urow_m [n_seq] at
// [s0, s1) (the other entries are left as given) and returns the chunk's unique-row count (0: dedup
// not applicable), or a negative RS_E* code.
int rs_debug_plan_unique(const int32_t* tok_off, const int32_t* len, const int32_t* mask, const int32_t* mask_end,
                         int32_t n_seq, int32_t s0, int32_t s1, int32_t* urow_h, int32_t* urow_m) {
    if (!tok_off || !len || !mask || !mask_end || !urow_h || !urow_m) return fail(RS_EARG, "null argument");
    if (s0 < 0 || s1 <= s0 || s1 > n_seq) return fail(RS_EARG, "bad sequence range");
    SeqList sl;
    for (int s = 0; s < n_seq; ++s) sl.push(tok_off[s], len[s], mask[s], mask_end[s], 0, -1);
    const int urows = plan_unique_rows(sl, s0, s1);
    for (int s = s0; s < s1 && urows > 0; ++s) {
        urow_h[s] = sl.urow_h[s];
        urow_m[s] = sl.urow_m[s];
    }
    return urows;
}

int rs_model_set_token_types(rs_model* m, const int32_t* d_type, int64_t n) {
    if (!m) return fail(RS_EARG, "null model");
    if (d_type && n < 0) return fail(RS_EARG, "negative count");
    m->type_next = d_type;
    m->type_n = d_type ? n : 0;
    return RS_OK;
}

int rs_model_set_sync_check(rs_model* m, int on) {
    if (!m) return fail(RS_EARG, "null model");
    m->sync_check = on != 0;
    return RS_OK;
}

int rs_check(rs_model* m, void* stream) {
    if (!m) return fail(RS_EARG, "null model");
    CALL_ORDER(m, (hipStream_t)stream);
    return report_flags(m, (hipStream_t)stream, "scores");
}

int rs_profile_enable(rs_model* m, int on) {
    if (!m) return fail(RS_EARG, "null model");
    prof_collect(m);
    m->prof = on != 0;
    for (int k = 0; k < RS_K_COUNT; ++k) m->prof_ms[k] = 0, m->prof_n[k] = 0, m->prof_flops[k] = 0;
    return RS_OK;
}

int rs_profile_read(rs_model* m, int kind, double* ms, int64_t* launches, double* flops) {
    if (!m || kind < 0 || kind >= RS_K_COUNT) return fail(RS_EARG, "bad argument");
    prof_collect(m);
    if (ms) *ms = m->prof_ms[kind];
    if (launches) *launches = m->prof_n[kind];
    if (flops) *flops = m->prof_flops[kind];
    return RS_OK;
}

void rs_model_destroy(rs_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    for (void* p : m->allocs) (void)hipFree(p);
    for (DevBuf* b : {&m->xst, &m->xst1, &m->h16, &m->t32, &m->qkv, &m->ctx, &m->inter, &m->ctxq, &m->resq,
                      &m->tq32, &m->hq32, &m->hq16, &m->interq, &m->lab, &m->llog, &m->part, &m->topk_cand,
                      &m->cand_meta, &m->cand_logit,
                      &m->rowlp_tmp, &m->meta, &m->emb, &m->plan, &m->flag, &m->lnx, &m->lncnt,
                      &m->lnerr})
        b->release();
    if (m->pinned_flag) (void)hipHostFree(m->pinned_flag);
    if (m->call_done) (void)hipEventDestroy(m->call_done);
    for (hipEvent_t e : m->ev_pool) (void)hipEventDestroy(e);
    delete m;
}

}  // extern "C"

// shared error slot for the other C-ABI translation units (train_api.hip)
int rs_fail(int code, const std::string& msg) { return fail(code, msg); }
