// akaze_plan.h — what the pure host mathematics of the AKAZE61 path (akaze_plan.hip: no HIP call, it also links into the stand-alone check
// tools/akaze_plan_check.cpp) hands the runtime that owns the device (akaze_api.hip).  afv_akaze_plan_for is public: include/afv_akaze.h.
#pragma once
#include "../../include/afv_akaze.h"
#include "afv_host.h"
#include "akz_jobs.h"

#define AKD_ENTRY_CAP 65535   // keypoints per frame after detection
#define AKD_SLOT_CAP 131072   // slot space of the ordered suppression: one slot per candidate (all levels of a frame)

// A frame's detection arrays for a plan: per level the candidate slice (w * h / 8 + 64 extrema candidates, afv_akaze.h), the row offset and
// the constants the kernels read, the strides over a frame, the grids of the ordered suppression.  afv_akaze_create sizes its buffers with
// the layout of the largest plan, akz_detect_enqueue hands the current one to the kernels (and fills in planes and thresholds).  Slices and
// strides are always filled; the return value is the verdict on the grids (AFV_EUNSUPPORTED: akd_box packing, u8 list lengths).
AFV_LOCAL int akz_detect_layout(const afv_akaze_plan &P, float derivative_factor, AkdParams &D);

// the plugin tail's budget: quadtree quotas (FeatureExtractor.cpp:97-108) for nfeatures / scaleFactor of the settings over the plan's
// levels, and the per-level selection capacity, the output capacity and the quadtree's node capacity that follow from them
AFV_LOCAL void akz_quota_plan(const afv_akaze_params &prm, int nlevels, int *quota, int *sel_cap, int *out_cap, int *qt_M);

struct AkzArena {  // pinned staging of a host-pointer call: [frames in][status][counts][keypoints][descriptors, 64-byte rows], 256-byte aligned
    size_t in_bytes, off_status, off_count, off_kps, off_desc, total;
    AkzArena(int nframes, size_t img, size_t out_cap) {
        const size_t nf = (size_t)nframes;
        in_bytes = nf * img;
        off_status = align_up(in_bytes, 256);
        off_count = off_status + 256;
        off_kps = off_count + align_up(nf * sizeof(int), 256);
        off_desc = off_kps + align_up(nf * out_cap * sizeof(afv_keypoint), 256);
        total = off_desc + nf * out_cap * 64;
    }
};
