// afv_host.h — host-only helpers of every runtime behind the C-ABI, whatever its context type: afv_runtime.h includes it for the
// translation units around afv_ctx, the AKAZE61 runtime (akaze_api.hip, akaze_plan.hip: a context of its own) includes it directly.
// Needs nothing but a `last_error` string in the context.  Not part of the public interface.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <new>
#include <string>

#include "../../include/afv_hip.h"

// internal functions that cross translation units without entering the library's dynamic symbol table
#define AFV_LOCAL __attribute__((visibility("hidden")))

#define HIPCHK(ctx, call)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);                  \
            return e_ == hipErrorOutOfMemory ? AFV_ENOMEM : AFV_EHIP;                                \
        }                                                                                            \
    } while (0)

// the C-ABI never throws: host allocation failures inside an entry point become AFV_ENOMEM
template <class Ctx, class F>
static inline int guarded(Ctx *c, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        if (c) c->last_error = "out of host memory";
        return AFV_ENOMEM;
    } catch (...) {
        if (c) c->last_error = "unexpected exception";
        return AFV_EHIP;
    }
}

static inline int cv_round(float v) { return (int)lrintf(v); }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The per-level feature quotas of FeatureExtractor.cpp:97-108 (and of cv::ORB's computeKeyPoints): a geometric series over the levels
// with ratio `factor` = 1 / scaleFactor, rounded level by level, the last level takes the rest.  `factor` comes from the caller because
// the callers form the reciprocal differently (in float / through double), and a quota must not move by a last bit of it.
static inline void afv_level_quotas(int nfeatures, float factor, int nlevels, int *out) {
    float desired = (float)nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; ++l) {
        out[l] = cv_round(desired);
        sum += out[l];
        desired *= factor;
    }
    out[nlevels - 1] = std::max(nfeatures - sum, 0);
}

// true when `p` is page-locked host memory the DMA engines can reach directly (hipHostMalloc / hipHostRegister / torch pin_memory)
static inline bool is_pinned_host(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // plain malloc'ed memory: "invalid value", not an error for us
        return false;
    }
    return at.type == hipMemoryTypeHost;
}
// ... for a whole buffer: first and last byte are probed (one registration covers a buffer)
static inline bool is_pinned_range(const void *p, size_t bytes) {
    return is_pinned_host(p) && is_pinned_host(static_cast<const uint8_t *>(p) + bytes - 1);
}
