// akaze_api.hip — host runtime of the AKAZE61 path (include/afv_akaze.h): the context and its HBM layout, frame staging, stage enqueue,
// the status rule and the entry points.  The evolution plan and every layout computation are host mathematics of their own: akaze_plan.hip.
#include <cstring>
#include <vector>

#include "akaze_plan.h"

struct afv_akaze {
    int device = 0;
    afv_akaze_params prm{};
    afv_akaze_plan plan{};  // for the current frame size
    hipStream_t stream = nullptr;
    std::string last_error;
    // HBM: per level 3 planes x max_batch frames (level 0: Lsmooth aliases Lt); scratch at level-0 size.  The first derivatives have no
    // planes (round 5): k_akz_dhess keeps them in registers, the descriptor stage evaluates them where it samples (k_akaze_desc.hip)
    float *lt[AFV_AKZ_MAX_LEVELS] = {}, *lsm[AFV_AKZ_MAX_LEVELS] = {}, *ldet[AFV_AKZ_MAX_LEVELS] = {};
    float *flow = nullptr, *pong = nullptr, *half = nullptr;
    float *d_taps = nullptr;  // gauss_soffset[32] | gauss_one[8]
    unsigned int *d_hmax = nullptr;
    int *d_hist = nullptr;
    float *d_kcontrast = nullptr;
    uint8_t *d_gray = nullptr;
    size_t gray_bytes = 0;
    int cur_w = 0, cur_h = 0, cur_frames = 0;
    // detection
    AkdParams dp{};
    AkdState ds{};
    float *d_cand_resp = nullptr;
    unsigned long long *d_mask = nullptr;  // [frame][rows][32] candidate bitmap words
    int *d_row_count = nullptr, *d_row_start = nullptr, *d_cand = nullptr, *d_cand_count = nullptr, *d_kp_count = nullptr, *d_status = nullptr;
    afv_keypoint *d_kps = nullptr;
    size_t cand_stride_max = 0, rows_stride_max = 0, grid_cells_max = 0, grid_elems_max = 0, cells_bytes = 0;
    bool have_scale_space = false, have_keypoints = false, have_descriptors = false;
    // plugin tail: quadtree filter + descriptors
    int *d_lvl_idx = nullptr, *d_sel = nullptr, *d_sel_count = nullptr, *d_out_count = nullptr;
    uint16_t *d_lvl_node = nullptr;
    afv_keypoint *d_out_kps = nullptr;
    uint8_t *d_out_desc = nullptr;
    int sel_cap = 0, out_cap = 0, qt_M = 0;
    int quota[AFV_AKZ_MAX_LEVELS] = {};
    bool step_by_step = false;  // test hook: one kernel per FED step instead of the fused level kernel
    int suppress_mode = 2;      // ordered duplicate suppression: 0 = speculative rounds, 1 = fixed point, 2 = fixed point, falling back to 0
                                // for a batch in which a candidate has more than AKF_K earlier in-range candidates (or the pass bound is hit)
    bool detect_fallback = false;  // this scale space already needed the fallback
    bool profiling = false;
    hipEvent_t ev[3] = {};
    float ms_ss = 0, ms_hess = 0;
    int launches = 0;
    std::vector<void *> allocs;
    // pinned staging of the host-pointer calls (grow-only; layout: AkzArena)
    uint8_t *h_pin = nullptr;
    size_t pin_bytes = 0;
};

// An entry point's body: arguments checked (AFV_EINVAL), the C ABI never throws, the context's device is current
template <class F>
static int akz_call(afv_akaze *a, bool valid, F &&body) {
    if (!a || !valid) return AFV_EINVAL;
    return guarded(a, [&]() -> int {
        HIPCHK(a, hipSetDevice(a->device));
        return body();
    });
}

extern "C" const char *afv_akaze_last_error(const afv_akaze *a) { return a ? a->last_error.c_str() : "null context"; }

extern "C" void afv_akaze_destroy(afv_akaze *a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    if (a->stream) (void)hipStreamSynchronize(a->stream);
    for (void *p : a->allocs)
        if (p) (void)hipFree(p);
    if (a->d_gray) (void)hipFree(a->d_gray);
    if (a->h_pin) (void)hipHostFree(a->h_pin);
    for (hipEvent_t e : a->ev)
        if (e) (void)hipEventDestroy(e);
    if (a->stream) (void)hipStreamDestroy(a->stream);
    delete a;
}

// the device allocations of afv_akaze_create: the first failure sticks and every later request is skipped
struct AkzAllocator {
    afv_akaze *a;
    int rc = AFV_OK;
    template <class T>
    void operator()(T **p, size_t count) {
        if (rc == AFV_OK) rc = bytes(reinterpret_cast<void **>(p), std::max<size_t>(count, 1) * sizeof(T));
    }
    AFV_LOCAL int bytes(void **p, size_t n) {
        HIPCHK(a, hipMalloc(p, n));
        a->allocs.push_back(*p);
        return AFV_OK;
    }
};

static int akz_create_buffers(afv_akaze *a) {
    const afv_akaze_params &prm = a->prm;
    const afv_akaze_plan &plan = a->plan;
    const size_t B = (size_t)prm.max_batch;
    AkzAllocator al{a};
    for (int i = 0; i < plan.nlevels; ++i) {
        const size_t n = (size_t)plan.lv[i].w * plan.lv[i].h * B;
        al(&a->lt[i], n);
        if (i == 0) a->lsm[0] = a->lt[0];  // evolution_[0].Lt.copyTo(evolution_[0].Lsmooth)
        else al(&a->lsm[i], n);
        al(&a->ldet[i], n);
    }
    const size_t n0 = (size_t)prm.max_width * prm.max_height * B;
    al(&a->flow, n0);
    al(&a->pong, n0);
    al(&a->half, n0 / 4 + B);
    al(&a->d_taps, 40);
    // maxima and histograms of the contrast percentile in one block: one memset per call clears both
    al(&a->d_hmax, B + B * (size_t)(prm.kcontrast_nbins + 1));
    if (al.rc == AFV_OK) a->d_hist = reinterpret_cast<int *>(a->d_hmax + B);
    al(&a->d_kcontrast, B);
    {   // detection buffers sized for the largest frame.  A plain 16 below is the per-frame stride of the level counters that the kernels
        // use as well (d_cand_count, d_sel_count, ds.ticket, ds.used: k_akaze_detect.hip, k_akaze_desc.hip), not AFV_AKZ_MAX_LEVELS
        AkdParams D{};
        const int grid_rc = akz_detect_layout(plan, prm.derivative_factor, D);
        const size_t cands = (size_t)D.cand_stride, rows = (size_t)D.rows_stride;
        a->cand_stride_max = cands;
        a->rows_stride_max = rows;
        al(&a->d_mask, rows * 32 * B);
        al(&a->d_row_start, rows * B);
        al(&a->d_cand, cands * B);
        al(&a->d_cand_resp, cands * B);
        al(&a->d_cand_count, 16 * B);
        al(&a->d_kp_count, B);
        al(&a->d_kps, (size_t)AKD_ENTRY_CAP * B);
        al(&a->ds.entry, (size_t)AKD_SLOT_CAP * B);
        al(&a->ds.keep, (size_t)AKD_SLOT_CAP * B);
        // one cell grid per level (the levels of a frame are suppressed as a pipeline), sized for the largest frame
        if (al.rc == AFV_OK) al.rc = grid_rc;
        a->grid_cells_max = (size_t)D.gcells;
        a->grid_elems_max = (size_t)D.gelems;
        al(&a->ds.cells, (size_t)D.gelems * B);
        a->cells_bytes = (size_t)D.gelems * B * sizeof(uint4);
        al(&a->ds.gcnt, (size_t)D.gcells * B);
        al(&a->ds.ticket, (size_t)8 + 16 * B);
        al(&a->ds.used, (size_t)16 * B);
        al(&a->ds.chunk_cnt, (size_t)(AKD_SLOT_CAP / 1024) * B);
        // fixed-point engine
        al(&a->ds.fp_nbr, (size_t)AKD_SLOT_CAP * AKF_K * B);
        al(&a->ds.fp_state, (size_t)AKD_SLOT_CAP * 2 * B);
        al(&a->ds.fp_active, (size_t)AKD_SLOT_CAP * 2 * B);
        al(&a->ds.fp_ctl, (size_t)AKF_CTL * B + 1);  // + the status word: one memset per detection
        if (al.rc == AFV_OK) a->d_status = a->ds.fp_ctl + (size_t)AKF_CTL * B;
        al(&a->ds.wpre, rows * 32 * B);
    }
    {   // plugin tail
        const int nl = plan.nlevels;
        akz_quota_plan(prm, nl, a->quota, &a->sel_cap, &a->out_cap, &a->qt_M);
        if (afv_akz_select_lds_bytes(a->qt_M) > 150 * 1024) al.rc = AFV_EUNSUPPORTED;
        al(&a->d_lvl_idx, (size_t)nl * AKD_ENTRY_CAP * B);
        al(&a->d_lvl_node, (size_t)nl * AKD_ENTRY_CAP * B);
        al(&a->d_sel, (size_t)nl * a->sel_cap * B);
        al(&a->d_sel_count, 16 * B);
        al(&a->d_out_count, B);
        al(&a->d_out_kps, (size_t)a->out_cap * B);
        al(&a->d_out_desc, (size_t)a->out_cap * 64 * B);
    }
    for (hipEvent_t &e : a->ev)
        if (al.rc == AFV_OK && hipEventCreate(&e) != hipSuccess) al.rc = AFV_EHIP;
    return al.rc;
}

extern "C" int afv_akaze_create(int device, const afv_akaze_params *prm, afv_akaze **out) {
    if (!prm || !out) return AFV_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AFV_ENODEV;  // no CPU fallback: fail loudly
    if (device < 0 || device >= ndev) return AFV_ENODEV;
    if (prm->max_batch < 1 || prm->max_width < 80 || prm->max_height < 40 || prm->nfeatures < 1 || prm->nfeatures > 8000 ||
        !(prm->scale_factor > 1.0f))
        return AFV_EINVAL;
    afv_akaze_plan plan;
    int rc = afv_akaze_plan_for(prm, prm->max_width, prm->max_height, &plan);
    if (rc) return rc;
    afv_akaze *a = new (std::nothrow) afv_akaze();
    if (!a) return AFV_ENOMEM;
    a->device = device;
    a->prm = *prm;
    a->plan = plan;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess) {
        delete a;
        return AFV_EHIP;
    }
    rc = guarded(a, [&]() -> int { return akz_create_buffers(a); });
    if (rc != AFV_OK) {
        afv_akaze_destroy(a);
        return rc;
    }
    *out = a;
    return AFV_OK;
}

static int akz_enqueue(afv_akaze *a, const uint8_t *d_gray, int nframes, int w, int h, int stride, size_t frame_stride) {
    if (w != a->cur_w || h != a->cur_h) {
        afv_akaze_plan plan;
        const int rc = afv_akaze_plan_for(&a->prm, w, h, &plan);
        if (rc) return rc;
        a->plan = plan;
        a->cur_w = w;
        a->cur_h = h;
        float taps[40] = {};
        std::memcpy(taps, plan.gauss_soffset, sizeof(float) * 32);
        std::memcpy(taps + 32, plan.gauss_one, sizeof(float) * 8);
        HIPCHK(a, hipMemcpyAsync(a->d_taps, taps, sizeof taps, hipMemcpyHostToDevice, a->stream));
        HIPCHK(a, hipStreamSynchronize(a->stream));  // `taps` is a stack buffer
    }
    a->cur_frames = nframes;
    a->have_scale_space = true;
    a->have_keypoints = false;
    a->detect_fallback = false;
    const afv_akaze_plan &P = a->plan;
    hipStream_t st = a->stream;
    const int nb = a->prm.kcontrast_nbins;
    if (a->profiling) HIPCHK(a, hipEventRecord(a->ev[0], st));
    // level 0: Lt = GaussianBlur(convert(gray), soffset); contrast factor from the sigma = 1 smoothed image
    if (afv_akz_launch_gauss(d_gray, 1, stride, frame_stride, w, h, nframes, a->d_taps, P.ksize_soffset, a->lt[0], st)) return AFV_EUNSUPPORTED;
    // the sigma = 1 image only feeds the gradient magnitude: with the usual 5-tap Gaussian it is formed inside that kernel
    const bool fused_contrast = !a->step_by_step && P.ksize_one == 5;
    if (!fused_contrast && afv_akz_launch_gauss(d_gray, 1, stride, frame_stride, w, h, nframes, a->d_taps + 32, P.ksize_one, a->pong, st))
        return AFV_EUNSUPPORTED;
    HIPCHK(a, hipMemsetAsync(a->d_hmax, 0, ((size_t)a->prm.max_batch + (size_t)nframes * (nb + 1)) * sizeof(int), st));  // d_hist follows d_hmax
    afv_akz_launch_kcontrast(fused_contrast ? nullptr : a->pong, d_gray, stride, (size_t)frame_stride, a->d_taps + 32, w, h, nframes, a->flow, a->d_hmax,
                             a->d_hist, nb, a->prm.kcontrast_percentile, a->d_kcontrast, st);
    for (int i = 1; i < P.nlevels; ++i) {
        const afv_akaze_level &L = P.lv[i], &Q = P.lv[i - 1];
        const float *src = a->lt[i - 1];
        if (L.octave > Q.octave) {
            afv_akz_launch_halfsample(a->lt[i - 1], Q.w, Q.h, a->half, L.w, L.h, nframes, st);
            src = a->half;
        }
        // Lsmooth + conductivity + the whole FED cycle of this level in one kernel (the usual case: 5-tap Gaussian, <= AKZ_FED_MAX steps)
        if (!a->step_by_step && P.ksize_one == 5 &&
            afv_akz_launch_fed_gauss(src, a->lsm[i], a->d_taps + 32, L.w, L.h, nframes, a->d_kcontrast, L.octave, L.nsteps, L.tau, a->lt[i], st))
            continue;
        // step by step (the test reference, longer FED cycles, degenerate sizes): Gaussian, conductivity, one kernel per FED step
        if (afv_akz_launch_gauss(src, 0, L.w, (size_t)L.w * L.h, L.w, L.h, nframes, a->d_taps + 32, P.ksize_one, a->lsm[i], st))
            return AFV_EUNSUPPORTED;
        afv_akz_launch_flow(a->lsm[i], L.w, L.h, nframes, a->d_kcontrast, L.octave, a->flow, st);
        // FED cycle, ping-pong so that the last step lands in Lt of this level
        const float *cur = src;
        for (int j = 0; j < L.nsteps; ++j) {
            float *dst = ((L.nsteps - 1 - j) % 2 == 0) ? a->lt[i] : a->pong;
            afv_akz_launch_nld_step(cur, a->flow, L.w, L.h, nframes, L.tau[j], dst, st);
            cur = dst;
        }
        if (L.nsteps == 0) HIPCHK(a, hipMemcpyAsync(a->lt[i], src, (size_t)L.w * L.h * nframes * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (a->profiling) HIPCHK(a, hipEventRecord(a->ev[1], st));
    for (int i = 0; i < P.nlevels; ++i) {
        const afv_akaze_level &L = P.lv[i];
        // the first derivatives stay in the kernel's registers; the two-kernel form (test reference, other sigma sizes) hands them over
        // through the scratch planes, which are free once the scale space is built
        const bool fused = !a->step_by_step && L.sigma_size >= 2 && L.sigma_size <= 4;
        if (afv_akz_launch_hessian(a->lsm[i], L.w, L.h, nframes, L.sigma_size, fused ? 0 : 1, fused ? nullptr : a->pong, fused ? nullptr : a->flow,
                                   a->ldet[i], st))
            return AFV_EUNSUPPORTED;
    }
    if (a->profiling) {
        HIPCHK(a, hipEventRecord(a->ev[2], st));
        HIPCHK(a, hipEventSynchronize(a->ev[2]));
        float m0 = 0, m1 = 0;
        HIPCHK(a, hipEventElapsedTime(&m0, a->ev[0], a->ev[1]));
        HIPCHK(a, hipEventElapsedTime(&m1, a->ev[1], a->ev[2]));
        a->ms_ss += m0;
        a->ms_hess += m1;
        a->launches += 1;
    }
    HIPCHK(a, hipGetLastError());
    return AFV_OK;
}

static bool akz_frames_ok(const afv_akaze *a, const uint8_t *gray, int nframes, int w, int h, int stride, size_t frame_stride) {
    return a && gray && nframes >= 1 && nframes <= a->prm.max_batch && w >= 80 && h >= 40 && w <= a->prm.max_width && h <= a->prm.max_height &&
           stride >= w && !(nframes > 1 && frame_stride < (size_t)stride * (h - 1) + w) &&
           (size_t)w * h <= (size_t)a->prm.max_width * a->prm.max_height;
}

// The frames of a host-pointer call into d_gray, tightly packed (row pitch w, frame pitch w * h), for afv_akaze_scale_space and
// afv_akaze_extract alike.  d_gray and the pinned arena grow as needed; page-locked caller frames are DMA'd in place, pageable ones are
// gathered into the arena (a pageable 1280 x 720 image costs one memcpy, not a staged 2-D copy) and sent in one transfer.  Asynchronous:
// the caller waits for the stream before the arena is used again.
static int akz_stage_frames(afv_akaze *a, const uint8_t *gray, int nframes, int w, int h, int stride, size_t frame_stride, const AkzArena &A) {
    hipStream_t st = a->stream;
    const size_t img = (size_t)w * h;
    if (A.in_bytes > a->gray_bytes) {
        HIPCHK(a, hipStreamSynchronize(st));
        if (a->d_gray) (void)hipFree(a->d_gray);
        a->d_gray = nullptr;
        a->gray_bytes = 0;
        HIPCHK(a, hipMalloc(reinterpret_cast<void **>(&a->d_gray), A.in_bytes));
        a->gray_bytes = A.in_bytes;
    }
    if (A.total > a->pin_bytes) {
        HIPCHK(a, hipStreamSynchronize(st));
        if (a->h_pin) (void)hipHostFree(a->h_pin);
        a->h_pin = nullptr;
        a->pin_bytes = 0;
        HIPCHK(a, hipHostMalloc(reinterpret_cast<void **>(&a->h_pin), A.total, hipHostMallocDefault));
        a->pin_bytes = A.total;
    }
    if (is_pinned_range(gray, (size_t)(nframes - 1) * frame_stride + (size_t)(h - 1) * stride + w)) {
        for (int f = 0; f < nframes; ++f)
            HIPCHK(a, hipMemcpy2DAsync(a->d_gray + (size_t)f * img, (size_t)w, gray + (size_t)f * frame_stride, (size_t)stride, (size_t)w, (size_t)h,
                                       hipMemcpyHostToDevice, st));
        return AFV_OK;
    }
    for (int f = 0; f < nframes; ++f) {
        const uint8_t *src = gray + (size_t)f * frame_stride;
        uint8_t *dst = a->h_pin + (size_t)f * img;
        if (stride == w) std::memcpy(dst, src, img);
        else
            for (int y = 0; y < h; ++y) std::memcpy(dst + (size_t)y * w, src + (size_t)y * stride, (size_t)w);
    }
    HIPCHK(a, hipMemcpyAsync(a->d_gray, a->h_pin, A.in_bytes, hipMemcpyHostToDevice, st));
    return AFV_OK;
}

extern "C" int afv_akaze_scale_space_device(afv_akaze *a, const uint8_t *d_gray, int nframes, int w, int h, int stride, size_t frame_stride) {
    return akz_call(a, akz_frames_ok(a, d_gray, nframes, w, h, stride, frame_stride),
                    [&]() -> int { return akz_enqueue(a, d_gray, nframes, w, h, stride, frame_stride); });
}

extern "C" int afv_akaze_scale_space(afv_akaze *a, const uint8_t *gray, int nframes, int w, int h, int stride, size_t frame_stride) {
    return akz_call(a, akz_frames_ok(a, gray, nframes, w, h, stride, frame_stride), [&]() -> int {
        int rc = akz_stage_frames(a, gray, nframes, w, h, stride, frame_stride, AkzArena(nframes, (size_t)w * h, (size_t)a->out_cap));
        if (rc == AFV_OK) rc = akz_enqueue(a, a->d_gray, nframes, w, h, w, (size_t)w * h);
        if (rc) return rc;
        HIPCHK(a, hipStreamSynchronize(a->stream));
        return AFV_OK;
    });
}

extern "C" int afv_akaze_synchronize(afv_akaze *a) {
    return akz_call(a, true, [&]() -> int { HIPCHK(a, hipStreamSynchronize(a->stream)); return AFV_OK; });
}

extern "C" int afv_akaze_get_plane(afv_akaze *a, int frame, int level, int which, float *out) {
    return akz_call(a, a && out && frame >= 0 && frame < a->cur_frames && level >= 0 && level < a->plan.nlevels && a->cur_w != 0 &&
                           which >= AFV_AKZ_LT && which <= AFV_AKZ_LDET, [&]() -> int {
        const afv_akaze_level &L = a->plan.lv[level];
        const float *base = which == AFV_AKZ_LT ? a->lt[level] : which == AFV_AKZ_LSMOOTH ? a->lsm[level] : which == AFV_AKZ_LDET ? a->ldet[level]
                            : which == AFV_AKZ_LX ? a->pong : a->flow;  // LX / LY: evaluated below
        size_t off = (size_t)frame * L.w * L.h;
        if (which == AFV_AKZ_LX || which == AFV_AKZ_LY) {
            // no derivative planes exist: this frame's are produced now, by the kernel the pipeline ran (with its first-derivative stores
            // switched on; the determinant it rewrites is the one that is there), into the scratch planes
            if (afv_akz_launch_hessian(a->lsm[level] + off, L.w, L.h, 1, L.sigma_size, a->step_by_step ? 1 : 0, a->pong, a->flow, a->ldet[level] + off,
                                       a->stream))
                return AFV_EUNSUPPORTED;
            off = 0;
        }
        HIPCHK(a, hipStreamSynchronize(a->stream));
        HIPCHK(a, hipMemcpy(out, base + off, (size_t)L.w * L.h * sizeof(float), hipMemcpyDeviceToHost));
        if (which == AFV_AKZ_LX || which == AFV_AKZ_LY) {  // the device planes are unscaled: Lx *= sigma_size as upstream does in place
            const float fs = (float)L.sigma_size;
            for (size_t i = 0, n = (size_t)L.w * L.h; i < n; ++i) out[i] = out[i] * fs;
        }
        return AFV_OK;
    });
}

extern "C" int afv_akaze_get_kcontrast(afv_akaze *a, int frame, float *out) {
    return akz_call(a, a && out && frame >= 0 && frame < a->cur_frames, [&]() -> int {
        HIPCHK(a, hipStreamSynchronize(a->stream));
        HIPCHK(a, hipMemcpy(out, a->d_kcontrast + frame, sizeof(float), hipMemcpyDeviceToHost));
        return AFV_OK;
    });
}

extern "C" int afv_akaze_profile_enable(afv_akaze *a, int on) {
    if (!a) return AFV_EINVAL;
    a->profiling = on != 0;
    a->ms_ss = a->ms_hess = 0;
    a->launches = 0;
    return AFV_OK;
}

extern "C" int afv_akaze_profile_read(afv_akaze *a, float *ms_scale_space, float *ms_hessian, int *launches) {
    if (!a) return AFV_EINVAL;
    if (ms_scale_space) *ms_scale_space = a->ms_ss;
    if (ms_hessian) *ms_hessian = a->ms_hess;
    if (launches) *launches = a->launches;
    return AFV_OK;
}

// ---- Feature_Detection ----
static int akz_detect_enqueue(afv_akaze *a) {
    if (!a->have_scale_space) return AFV_EINVAL;
    const afv_akaze_plan &P = a->plan;
    AkdParams &D = a->dp;
    D = AkdParams{};
    const int grid_rc = akz_detect_layout(P, a->prm.derivative_factor, D);
    D.dthreshold = a->prm.dthreshold; D.min_dthreshold = a->prm.min_dthreshold;
    for (int i = 0; i < P.nlevels; ++i) D.lv[i].ldet = a->ldet[i];
    if ((size_t)D.cand_stride > a->cand_stride_max || (size_t)D.rows_stride > a->rows_stride_max) return AFV_EINVAL;
    if (P.w > 2048) return AFV_EUNSUPPORTED;
    if (grid_rc) return grid_rc;
    if ((size_t)D.gcells > a->grid_cells_max || (size_t)D.gelems > a->grid_elems_max || D.lds_bytes > 52 * 1024) return AFV_EUNSUPPORTED;  // + ~10 KB of static LDS in k_akz_suppress (256-candidate rounds): 64 KB in all
    D.entry_cap = AKD_SLOT_CAP; D.kp_cap = AKD_ENTRY_CAP;
    hipStream_t st = a->stream;
    HIPCHK(a, hipMemsetAsync(a->ds.fp_ctl, 0, ((size_t)AKF_CTL * a->prm.max_batch + 1) * sizeof(int), st));  // fixed-point control block + d_status
    // list elements carry a 14-bit launch epoch (k_akaze_detect.hip); the grids are wiped whenever it starts over
    if (a->ds.epoch == 0 || a->ds.epoch >= 0x3fffu) {
        HIPCHK(a, hipMemsetAsync(a->ds.cells, 0, a->cells_bytes, st));
        a->ds.epoch = 0;
    }
    ++a->ds.epoch;
    const int engine = (a->suppress_mode == 0 || a->detect_fallback) ? 0 : 1;
    afv_akz_launch_candidates(&D, a->cur_frames, a->d_mask, a->d_row_start, a->ds.wpre, a->d_cand, a->d_cand_resp, a->d_cand_count, a->d_status, st);
    afv_akz_launch_suppress(&D, &a->ds, a->cur_frames, engine, a->d_mask, a->d_cand, a->d_cand_resp, a->d_cand_count, a->d_row_start, a->d_kps,
                            a->d_kp_count, a->d_status, st);
    HIPCHK(a, hipGetLastError());
    a->have_keypoints = true;
    a->have_descriptors = false;
    return AFV_OK;
}

extern "C" int afv_akaze_detect(afv_akaze *a) {
    return akz_call(a, true, [&]() -> int { return akz_detect_enqueue(a); });
}

// ---- the status rule: what the device status word of a detection / description run means ----
// ACCEPT: the run's results stand.  ACCEPT_CAPACITY: the run is final, AFV_ECAPACITY with `text`.  RERUN_ROUNDS: the fixed-point engine
// gave up on this batch, the same scale space goes through the ordered rounds.  STALLED: not a capacity problem - an earlier ticket holder
// of the level pipeline did not move for ~1 s (k_akaze_detect.hip)
enum AkzVerdict { AKZ_ACCEPT, AKZ_ACCEPT_CAPACITY, AKZ_RERUN_ROUNDS, AKZ_STALLED };
struct AkzRule {
    AkzVerdict verdict;
    const char *text;  // what afv_akaze_last_error says (null: accepted)
};
// Status 5 = stalled level pipeline, 6 / 7 = the fixed point gave up, anything else non-zero = a capacity.  With the fallback allowed
// (suppress mode 2) and not yet used on this scale space, 6 / 7 ask for the re-run.  With engine 1 forced they are final like every other
// capacity, and there the two consumers differ, by history rather than design: the getters (akz_status) return AFV_ECAPACITY before they
// read any data, afv_akaze_extract returns AFV_ECAPACITY AND copies that run's counts and rows out.  Both are kept as they were; a change
// of behaviour has to decide it here.
static AkzRule akz_status_rule(int st, int suppress_mode, bool fallback_used) {
    if (st == 0) return {AKZ_ACCEPT, nullptr};
    if (st == 5) return {AKZ_STALLED, "level pipeline stalled (suppression): the device was preempted or is being profiled; repeat the call"};
    const char *text = st == 1 ? "candidate capacity exceeded" : st == 2 ? "grid cell capacity exceeded" : st == 3 ? "keypoint list capacity exceeded"
                       : st == 6 ? "fixed-point suppression: more than AKF_K earlier in-range candidates" : st == 7 ? "fixed-point suppression: pass bound hit"
                       : "output capacity exceeded";
    return {(st == 6 || st == 7) && suppress_mode == 2 && !fallback_used ? AKZ_RERUN_ROUNDS : AKZ_ACCEPT_CAPACITY, text};
}
// the rule as a return code, its text in last_error (a run that is about to be repeated reports why until the repeat settles)
static int akz_rule_rc(afv_akaze *a, const AkzRule &r) {
    if (r.verdict == AKZ_ACCEPT) return AFV_OK;
    a->last_error = r.text;
    return r.verdict == AKZ_STALLED ? AFV_ETIMEOUT : AFV_ECAPACITY;
}

static int akz_describe_enqueue(afv_akaze *a);
// the getters' policy: wait, read the status word, re-run once through the ordered rounds when the rule asks for it, never repeat a stall
static int akz_status(afv_akaze *a) {
    int st = 0;
    HIPCHK(a, hipStreamSynchronize(a->stream));
    HIPCHK(a, hipMemcpy(&st, a->d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (akz_status_rule(st, a->suppress_mode, a->detect_fallback).verdict == AKZ_RERUN_ROUNDS) {
        const bool desc = a->have_descriptors;
        a->detect_fallback = true;
        int rc = akz_detect_enqueue(a);
        if (rc == AFV_OK && desc) rc = akz_describe_enqueue(a);
        if (rc) return rc;
        HIPCHK(a, hipStreamSynchronize(a->stream));
        HIPCHK(a, hipMemcpy(&st, a->d_status, sizeof(int), hipMemcpyDeviceToHost));
    }
    return akz_rule_rc(a, akz_status_rule(st, a->suppress_mode, a->detect_fallback));
}

extern "C" int afv_akaze_get_candidates(afv_akaze *a, int frame, int level, int32_t *out_idx, int cap, int *n_out) {
    return akz_call(a, a && n_out && frame >= 0 && frame < a->cur_frames && level >= 0 && level < a->plan.nlevels && a->have_keypoints, [&]() -> int {
        const int rc = akz_status(a);
        if (rc) return rc;
        int n = 0;
        HIPCHK(a, hipMemcpy(&n, a->d_cand_count + frame * 16 + level, sizeof(int), hipMemcpyDeviceToHost));  // 16: the kernels' stride
        *n_out = n;
        if (out_idx && n > 0) {
            if (n > cap) return AFV_ECAPACITY;
            HIPCHK(a, hipMemcpy(out_idx, a->d_cand + (size_t)frame * a->dp.cand_stride + a->dp.lv[level].cand_off, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
        return AFV_OK;
    });
}

extern "C" int afv_akaze_get_keypoints(afv_akaze *a, int frame, afv_keypoint *out, int cap, int *n_out) {
    return akz_call(a, a && n_out && frame >= 0 && frame < a->cur_frames && a->have_keypoints, [&]() -> int {
        const int rc = akz_status(a);
        if (rc) return rc;
        int n = 0;
        HIPCHK(a, hipMemcpy(&n, a->d_kp_count + frame, sizeof(int), hipMemcpyDeviceToHost));
        *n_out = n;
        if (out && n > 0) {
            if (n > cap) return AFV_ECAPACITY;
            HIPCHK(a, hipMemcpy(out, a->d_kps + (size_t)frame * AKD_ENTRY_CAP, (size_t)n * sizeof(afv_keypoint), hipMemcpyDeviceToHost));
        }
        return AFV_OK;
    });
}

// ---- plugin tail: filterKeypoints (quadtree per level) + computeDescriptors + mergeKeypointLevels ----
static int akz_describe_enqueue(afv_akaze *a) {
    if (!a->have_keypoints) return AFV_EINVAL;
    const afv_akaze_plan &P = a->plan;
    AksParams S{};
    S.nlevels = P.nlevels; S.W = P.w; S.H = P.h;
    S.n_ini = (int)roundf((float)P.w / (float)P.h);  // ORBextractor.cc:243
    if (S.n_ini < 1 || S.n_ini > 16) return AFV_EUNSUPPORTED;
    S.h_x = (float)P.w / (float)S.n_ini;
    for (int l = 0; l < P.nlevels; ++l) S.quota[l] = a->quota[l];
    S.kp_cap = AKD_ENTRY_CAP; S.sel_cap = a->sel_cap; S.out_cap = a->out_cap; S.M = a->qt_M;
    AkdDescParams D{};
    D.nlevels = P.nlevels; D.kp_cap = AKD_ENTRY_CAP; D.sel_cap = a->sel_cap; D.out_cap = a->out_cap; D.desc_pitch = 64;
    for (int l = 0; l < P.nlevels; ++l) D.lv[l] = AkdLevelPlanes{a->lt[l], a->lsm[l], P.lv[l].w, P.lv[l].h, P.lv[l].octave, P.lv[l].sigma_size, (float)P.lv[l].sigma_size};
    hipStream_t st = a->stream;
    afv_akz_launch_select(&S, a->cur_frames, a->d_kps, a->d_kp_count, a->d_lvl_idx, a->d_lvl_node, a->d_sel, a->d_sel_count, st);
    afv_akz_launch_describe(&D, a->cur_frames, a->out_cap, a->d_kps, a->d_sel, a->d_sel_count, a->d_out_kps, a->d_out_desc, a->d_out_count,
                            a->d_status, st);
    HIPCHK(a, hipGetLastError());
    a->have_descriptors = true;
    return AFV_OK;
}

extern "C" int afv_akaze_describe(afv_akaze *a) {
    return akz_call(a, true, [&]() -> int { return akz_describe_enqueue(a); });
}

extern "C" int afv_akaze_get_features(afv_akaze *a, int frame, afv_keypoint *kps, uint8_t *desc61, int cap, int *n_out) {
    return akz_call(a, a && n_out && frame >= 0 && frame < a->cur_frames && a->have_descriptors, [&]() -> int {
        const int rc = akz_status(a);
        if (rc) return rc;
        int n = 0;
        HIPCHK(a, hipMemcpy(&n, a->d_out_count + frame, sizeof(int), hipMemcpyDeviceToHost));
        *n_out = n;
        if (n > 0 && (kps || desc61)) {
            if (n > cap) return AFV_ECAPACITY;
            if (kps) HIPCHK(a, hipMemcpy(kps, a->d_out_kps + (size_t)frame * a->out_cap, (size_t)n * sizeof(afv_keypoint), hipMemcpyDeviceToHost));
            if (desc61)
                HIPCHK(a, hipMemcpy2D(desc61, 61, a->d_out_desc + (size_t)frame * a->out_cap * 64, 64, 61, (size_t)n, hipMemcpyDeviceToHost));
        }
        return AFV_OK;
    });
}

// FeatureExtractor_akaze61::detectAndCompute for a batch of host frames (Feature_akaze61.cpp:17-24 after initializeExtractor).
// The plugin calls it with ONE frame (FeatureExtractor.cpp:111-121): the whole call is one upload, the kernel chain, four read-backs and ONE
// wait - frames go through the pinned arena (akz_stage_frames), the results (status, counts, keypoints, 64-byte descriptor rows) come back
// into it asynchronously and are unpacked on the host (four blocking read-backs cost 6.7 ms per frame around 1.2 ms of kernels).
extern "C" int afv_akaze_extract(afv_akaze *a, const uint8_t *gray, int nframes, int w, int h, int stride, size_t frame_stride,
                                 afv_keypoint *kps, uint8_t *desc61, int cap_per_frame, int32_t *n_out) {
    return akz_call(a, n_out && kps && desc61 && cap_per_frame >= 1 && akz_frames_ok(a, gray, nframes, w, h, stride, frame_stride), [&]() -> int {
        hipStream_t st = a->stream;
        const size_t oc = (size_t)a->out_cap;
        const AkzArena A(nframes, (size_t)w * h, oc);
        int rc = akz_stage_frames(a, gray, nframes, w, h, stride, frame_stride, A);
        if (rc == AFV_OK) rc = akz_enqueue(a, a->d_gray, nframes, w, h, w, (size_t)w * h);
        if (rc) return rc;
        // This caller's policy: a stalled level pipeline is repeated, twice at most (the scale space is still there); the re-run through the
        // ordered rounds is NOT one of those repeats and has a budget of its own (they once shared one budget of three, and a loop that ended on
        // a `continue` copied the rejected run's results out).  Only a run the rule accepts is `settled`.
        bool settled = false;
        for (int timeouts = 0, fallbacks = 0; timeouts < 3 && fallbacks < 2 && !settled;) {
            rc = akz_detect_enqueue(a);
            if (rc == AFV_OK) rc = akz_describe_enqueue(a);
            if (rc) return rc;
            HIPCHK(a, hipMemcpyAsync(a->h_pin + A.off_status, a->d_status, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(a, hipMemcpyAsync(a->h_pin + A.off_count, a->d_out_count, (size_t)nframes * sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(a, hipMemcpyAsync(a->h_pin + A.off_kps, a->d_out_kps, (size_t)nframes * oc * sizeof(afv_keypoint), hipMemcpyDeviceToHost, st));
            HIPCHK(a, hipMemcpyAsync(a->h_pin + A.off_desc, a->d_out_desc, (size_t)nframes * oc * 64, hipMemcpyDeviceToHost, st));
            HIPCHK(a, hipStreamSynchronize(st));
            const AkzRule r = akz_status_rule(*reinterpret_cast<const int *>(a->h_pin + A.off_status), a->suppress_mode, a->detect_fallback);
            rc = akz_rule_rc(a, r);
            if (r.verdict == AKZ_STALLED) {
                ++timeouts;
            } else if (r.verdict == AKZ_RERUN_ROUNDS) {
                a->detect_fallback = true;
                ++fallbacks;
            } else {
                settled = true;
            }
        }
        if (!settled) {  // no run was accepted: nothing of the arena is a result
            for (int f = 0; f < nframes; ++f) n_out[f] = 0;
            return rc;
        }
        const int *cnt = reinterpret_cast<const int *>(a->h_pin + A.off_count);
        for (int f = 0; f < nframes; ++f) {
            int n = std::min(std::max(cnt[f], 0), (int)oc);
            n_out[f] = n;
            if (n > cap_per_frame) {
                n = cap_per_frame;
                if (rc == AFV_OK) rc = AFV_ECAPACITY;
            }
            std::memcpy(kps + (size_t)f * cap_per_frame, a->h_pin + A.off_kps + (size_t)f * oc * sizeof(afv_keypoint), (size_t)n * sizeof(afv_keypoint));
            const uint8_t *rows = a->h_pin + A.off_desc + (size_t)f * oc * 64;
            uint8_t *out = desc61 + (size_t)f * cap_per_frame * 61;
            for (int i = 0; i < n; ++i) std::memcpy(out + (size_t)i * 61, rows + (size_t)i * 64, 61);
        }
        return rc;
    });
}

extern "C" int afv_akaze_extract_device(afv_akaze *a, const uint8_t *d_gray, int nframes, int w, int h, int stride, size_t frame_stride) {
    return akz_call(a, akz_frames_ok(a, d_gray, nframes, w, h, stride, frame_stride), [&]() -> int {
        int rc = akz_enqueue(a, d_gray, nframes, w, h, stride, frame_stride);
        if (rc == AFV_OK) rc = akz_detect_enqueue(a);
        if (rc == AFV_OK) rc = akz_describe_enqueue(a);
        return rc;
    });
}

extern "C" int afv_akaze_get_quotas(const afv_akaze *a, int32_t *quota16) {
    if (!a || !quota16) return AFV_EINVAL;
    for (int l = 0; l < AFV_AKZ_MAX_LEVELS; ++l) quota16[l] = a->quota[l];
    return AFV_OK;
}

// 0 = ordered speculative rounds (k_akz_suppress), 1 = fixed point (k_akz_fp_*), 2 = fixed point with fallback (default); pass_cap > 0
// bounds the fixed point's passes (test hook: 1 forces the fallback / the error)
extern "C" int afv_akaze_set_suppress_engine(afv_akaze *a, int mode, int pass_cap) {
    if (!a || mode < 0 || mode > 2) return AFV_EINVAL;
    a->suppress_mode = mode;
    a->ds.fp_pass_cap = pass_cap > 0 ? pass_cap : 0;
    return AFV_OK;
}

// test hook: the fixed-point engine gives up (status 6) on a candidate with more than `cap` earlier in-range candidates (0: the built-in 16)
extern "C" int afv_akaze_debug_neighbour_cap(afv_akaze *a, int cap) {
    if (!a || cap < 0) return AFV_EINVAL;
    a->ds.fp_nbr_cap = cap;
    return AFV_OK;
}

// test hook: 1 = run pm_g2 and every FED step as its own kernel (the reference structure), 0 = fused level kernel (default)
extern "C" int afv_akaze_set_step_by_step(afv_akaze *a, int on) {
    if (!a) return AFV_EINVAL;
    a->step_by_step = on != 0;
    return AFV_OK;
}
