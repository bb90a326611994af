// Host-side helpers of the C-ABI translation units (rs_api.hip, train_api.hip): the shared error
// slot, the HIP-error macros, the growable device buffer and the common part of the rs_bert_cfg
// validation.  Host only: no kernel includes it.
#pragma once
#include <string>
#include <hip/hip_runtime.h>
#include "../../include/rescore.h"

// Stores msg as the calling thread's rs_last_error() and returns code (defined in rs_api.hip).
int rs_fail(int code, const std::string& msg);

// A failed HIP call as the entry point's return: RS_EHIP, or (alloc) RS_ENOMEM when out of memory.
inline int hip_fail(hipError_t e, const char* expr, bool alloc) {
    if (alloc && e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return rs_fail(RS_ENOMEM, std::string(expr) + ": out of device memory");
    }
    return rs_fail(RS_EHIP, std::string(expr) + ": " + hipGetErrorString(e));
}
#define TRY_HIP(expr)                                                \
    do {                                                             \
        hipError_t e_ = (expr);                                      \
        if (e_ != hipSuccess) return hip_fail(e_, #expr, false);     \
    } while (0)
#define TRY_ALLOC(expr)                                              \
    do {                                                             \
        hipError_t e_ = (expr);                                      \
        if (e_ != hipSuccess) return hip_fail(e_, #expr, true);      \
    } while (0)

// Device buffer that only grows (contents are not kept across a growth).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T* as() const { return (T*)p; }
};

// The encoder shape both rs_model_create and rs_trainer_create accept (inter_mult: the caller's
// granularity of cfg.intermediate), and the device lookup that ends their validation.
inline int check_bert_shape(const rs_bert_cfg& c, int inter_mult) {
    if (c.hidden <= 0 || c.hidden % 256 || c.hidden > 1024) return rs_fail(RS_EUNSUP, "hidden must be 256/512/768/1024");
    if (c.heads <= 0 || c.hidden / c.heads != 64 || c.hidden % c.heads) return rs_fail(RS_EUNSUP, "head_dim must be 64");
    if (c.intermediate <= 0 || c.intermediate % inter_mult)
        return rs_fail(RS_EUNSUP, "intermediate must be a multiple of " + std::to_string(inter_mult));
    if (c.layers < 1 || c.vocab < 1 || c.max_pos < 3 || c.type_vocab < 1) return rs_fail(RS_EARG, "bad config");
    return RS_OK;
}
inline int check_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return rs_fail(RS_EHIP, "no such HIP device");
    return RS_OK;
}
