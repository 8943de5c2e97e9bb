// afv_api.hip — host runtime behind the C-ABI of include/afv_hip.h: the context and what does not belong to one pipeline.
// Owns the HIP streams and the device scratch of one context (create / destroy), its settings and the stage profile; the brute-force pair
// and L2 matchers, ComputeDistinctiveDescriptors and the vocabulary.  The ORB32 extractor's host side (geometry, staging, the kernel
// pipeline, its entry points) is afv_extract.hip; the BoW-guided matchers are afv_match_jobs.hip; the projection searches are
// afv_project.hip.
// No CPU fallback exists: without a HIP device afv_create fails with AFV_ENODEV.
#include <algorithm>

#include "afv_runtime.h"

static const char *k_errors[] = {"ok", "invalid argument", "no usable HIP device", "out of memory", "HIP runtime error",
                                 "output capacity too small", "unsupported", "device-side wait timed out"};


extern "C" void afv_default_orb_params(afv_orb_params *p) {
    if (!p) return;
    p->nfeatures = 1000;
    p->nlevels = 8;
    p->scale_factor = 1.2f;
    p->fast_threshold = 20;
    p->max_width = 640;
    p->max_height = 480;
    p->max_batch = 1;
}

extern "C" int afv_abi_version(void) { return AFV_ABI_VERSION; }

extern "C" const char *afv_strerror(int code) {
    const int i = -code;
    if (i < 0 || i > 7) return "unknown error";
    return k_errors[i];
}
extern "C" const char *afv_last_error(const afv_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }
extern "C" void *afv_stream(afv_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" void afv_destroy(afv_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    afv_table_release_all(c);
    afv_frame_release_all(c);
    afv_points_release_all(c);
    void *ptrs[] = {c->d_geo, c->d_tab, c->d_pyr, c->d_cand_packed, c->d_kept_xy, c->d_l1, c->d_l1_resp, c->d_l1_count, c->d_hq, c->d_hq_n, c->d_kept_resp,
                    c->d_kept_node, c->d_cand_count, c->d_sel_count, c->d_sel, c->d_frames, c->d_out_block,
                    c->d_status, c->d_match, c->d_topk, c->d_slice, c->d_tickets, c->d_pf_blob, c->d_l2_scratch, c->d_proj_ticket, c->d_points_count};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (c->h_stage) {
        if (c->stage_pinned) (void)hipHostFree(c->h_stage);
        else std::free(c->h_stage);
    }
    for (auto &v : c->prof_ev)
        for (hipEvent_t e : v) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->pipe_ev) (void)hipEventDestroy(e);
    if (c->stream_copy) (void)hipStreamDestroy(c->stream_copy);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int afv_create(int device, const afv_orb_params *params, afv_ctx **out) {
    if (!params || !out) return AFV_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AFV_ENODEV;
    if (device < 0 || device >= ndev) return AFV_ENODEV;
    if (params->nfeatures < 1 || params->nfeatures > 4000 || params->max_batch < 1 || params->max_batch > 65535 ||
        params->scale_factor <= 1.0f)
        return AFV_EINVAL;
    afv_ctx *c = new (std::nothrow) afv_ctx();
    if (!c) return AFV_ENOMEM;
    c->device = device;
    c->p = *params;
    int rc = afv_build_geometry(c->p, params->max_width, params->max_height, params->max_batch, c->cap_geo);
    if (rc) {
        delete c;
        return rc;
    }
    const Geo &g = c->cap_geo;
    const int B = params->max_batch;
#define CREATE_CHK(call)                                                         \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) {                                                  \
            fprintf(stderr, "afv_create: %s: %s\n", #call, hipGetErrorString(e_)); \
            afv_destroy(c);                                                      \
            return e_ == hipErrorOutOfMemory ? AFV_ENOMEM : AFV_EHIP;            \
        }                                                                        \
    } while (0)
    CREATE_CHK(hipSetDevice(device));
    CREATE_CHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CREATE_CHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    CREATE_CHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    CREATE_CHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    CREATE_CHK(hipMalloc(&c->d_geo, sizeof(Geo)));
    c->tab_elems = 0;
    for (int l = 1; l < g.nlevels; ++l) c->tab_elems += (size_t)g.lv[l].w + (size_t)g.lv[l].h;
    CREATE_CHK(hipMalloc(&c->d_tab, std::max<size_t>(c->tab_elems, 1) * sizeof(short2)));
    CREATE_CHK(hipMalloc(&c->d_pyr, afv_geo_pyr_bytes(g, B)));
    const size_t ce = afv_geo_cand_elems(g, B);
    CREATE_CHK(hipMalloc(&c->d_cand_packed, ce * 4));
    CREATE_CHK(hipMalloc(&c->d_l1, ce * 4));
    CREATE_CHK(hipMalloc(&c->d_l1_resp, ce * 4));
    CREATE_CHK(hipMalloc(&c->d_l1_count, (size_t)B * AFV_MAX_LEVELS * sizeof(int)));
    c->hq_per_frame = afv_harris_queue_per_frame(&g);
    CREATE_CHK(hipMalloc(&c->d_hq, c->hq_per_frame * (size_t)B * sizeof(uint2)));
    CREATE_CHK(hipMalloc(&c->d_hq_n, (size_t)B * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->d_kept_xy, ce * 4));
    CREATE_CHK(hipMalloc(&c->d_kept_resp, ce * 4));
    CREATE_CHK(hipMalloc(&c->d_kept_node, ce * 2));
    CREATE_CHK(hipMalloc(&c->d_cand_count, (size_t)B * AFV_MAX_LEVELS * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->d_sel_count, (size_t)B * AFV_MAX_LEVELS * sizeof(int)));
    CREATE_CHK(hipMalloc(&c->d_sel, (size_t)B * g.sel_per_frame * sizeof(SelPoint)));
    CREATE_CHK(afv_fill(c, c->d_sel_count, 0, (size_t)B * AFV_MAX_LEVELS * sizeof(int)));
    // staging for host-pointer calls
    c->frames_pitch = align_up((size_t)params->max_width, 64);
    c->frames_stride = align_up(c->frames_pitch * (size_t)params->max_height, 256);
    CREATE_CHK(hipMalloc(&c->d_frames, c->frames_stride * (size_t)B + 256));  // frames back to back, one guard at the very end
    c->stage_cap = afv_max_keypoints_per_frame(c);
    {   // counts, keypoints and descriptors of the host-pointer calls in ONE block: [n][kps][desc] - with max_batch 1 (the plugin
        // context) the results of a frame are one contiguous range, i.e. one device-to-host copy
        c->out_kps_off = align_up((size_t)B * sizeof(int), 256);
        c->out_desc_off = c->out_kps_off + align_up((size_t)B * c->stage_cap * sizeof(afv_keypoint), 256);
        c->out_bytes = c->out_desc_off + (size_t)B * c->stage_cap * AFV_DESC_BYTES;
        CREATE_CHK(hipMalloc(&c->d_out_block, c->out_bytes));
        c->d_n = reinterpret_cast<int *>(c->d_out_block);
        c->d_kps = reinterpret_cast<afv_keypoint *>(c->d_out_block + c->out_kps_off);
        c->d_desc = c->d_out_block + c->out_desc_off;
    }
    CREATE_CHK(hipMalloc(&c->d_status, sizeof(int)));
    // quadtree node capacity: alive nodes <= max(quota + 3, 4 * n_ini)
    int M = 64;
    for (int l = 0; l < g.nlevels; ++l) M = std::max(M, g.lv[l].quota + 8);
    M = std::max(M, 4 * 16 + 8);
    M = (int)align_up((size_t)M, 64);
    c->select_M = M;
    if (afv_select_lds_bytes(M) > 160 * 1024) {
        afv_destroy(c);
        return AFV_EUNSUPPORTED;
    }
#undef CREATE_CHK
    // kernels that ask for more dynamic LDS than the default: raised once per context, on its device, checked
    if (hipMalloc(reinterpret_cast<void **>(&c->d_proj_ticket), 256) != hipSuccess || afv_fill(c, c->d_proj_ticket, 0, 256) != hipSuccess) {
        (void)hipGetLastError();
        if (c->d_proj_ticket) (void)hipFree(c->d_proj_ticket);
        c->d_proj_ticket = nullptr;  // the searches then take two launches
    }
    c->proj_wg_lds_max = afv_project_prepare();
    c->frame_lds_max = afv_frame_prepare();
    (void)afv_match_prepare();
    c->select_wide_ok = afv_select_prepare(c->select_M) != 0;
    *out = c;
    return AFV_OK;
}

static void profile_drain(afv_ctx *c) {
    for (int st = 0; st < AFV_NUM_STAGES; ++st) {
        for (size_t i = 0; i + 1 < c->prof_used[st]; i += 2) {
            float ms = 0.f;
            if (hipEventSynchronize(c->prof_ev[st][i + 1]) == hipSuccess &&
                hipEventElapsedTime(&ms, c->prof_ev[st][i], c->prof_ev[st][i + 1]) == hipSuccess) {
                c->prof_ms[st] += ms;
                c->prof_launches[st] += 1;
            }
        }
        c->prof_used[st] = 0;
    }
}

extern "C" int afv_set_split_threshold(afv_ctx *c, int min_frames) {
    if (!c || min_frames < 2) return AFV_EINVAL;
    c->split_min_frames = min_frames;
    return AFV_OK;
}
extern "C" int afv_set_pipeline_chunk(afv_ctx *c, int frames, int chunks_ahead) {
    if (!c || frames < 1 || chunks_ahead < 1 || chunks_ahead > 64) return AFV_EINVAL;
    c->pipe_chunk = frames;
    c->pipe_ahead = chunks_ahead;
    return AFV_OK;
}
extern "C" int afv_set_match_engine(afv_ctx *c, int engine) {
    if (!c || (engine != AFV_MATCH_ENGINE_POPCOUNT && engine != AFV_MATCH_ENGINE_MFMA)) return AFV_EINVAL;
    c->match_engine = engine;
    return AFV_OK;
}

extern "C" int afv_set_l2_chunk_pairs(afv_ctx *c, int pairs) {
    if (!c || pairs < 1 || pairs > 65535) return AFV_EINVAL;
    c->l2_chunk_pairs = pairs;
    return AFV_OK;
}

extern "C" int afv_set_match_resolve(afv_ctx *c, int engine) {
    if (!c || engine < 0 || engine > 2) return AFV_EINVAL;
    c->resolve_engine = engine;
    return AFV_OK;
}

extern "C" int afv_set_small_batch_path(afv_ctx *c, int mode, int max_frames) {
    if (!c || mode < 0 || mode > 2 || max_frames < 0) return AFV_EINVAL;
    c->small_mode = mode;
    if (max_frames > 0) c->small_max_frames = max_frames;
    return AFV_OK;
}

extern "C" int afv_set_split_chunks(afv_ctx *c, int chunks) {
    if (!c || (chunks != 0 && chunks < 2) || chunks > 64) return AFV_EINVAL;
    c->split_chunks = chunks;
    return AFV_OK;
}

extern "C" int afv_set_split_schedule(afv_ctx *c, int mode) {
    if (!c || (mode != 0 && mode != 1)) return AFV_EINVAL;
    c->split_schedule = mode;
    return AFV_OK;
}

extern "C" int afv_profile_enable(afv_ctx *c, int enable) {
    if (!c) return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    profile_drain(c);
    c->prof = false;
    c->prof_every = enable > 0 ? enable : 0;
    c->prof_tick_extract = c->prof_tick_match = 0;
    if (enable)
        for (int st = 0; st < AFV_NUM_STAGES; ++st) {
            c->prof_ms[st] = 0.f;
            c->prof_launches[st] = 0;
            c->prof_units[st] = 0;
        }
    return AFV_OK;
}

extern "C" int afv_num_stages(void) { return AFV_NUM_STAGES; }

extern "C" int afv_profile_read(afv_ctx *c, int32_t *launches, float *total_ms, int64_t *units) {
    if (!c || !launches || !total_ms) return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    profile_drain(c);
    for (int st = 0; st < AFV_NUM_STAGES; ++st) {
        launches[st] = c->prof_launches[st];
        total_ms[st] = c->prof_ms[st];
        if (units) units[st] = c->prof_units[st];
    }
    return AFV_OK;
}

// ---- test hooks for the per-call scratch (include/afv_hip.h, "test hooks for the per-call scratch"): sizes, a fill, the zero-at-rest
// words.  The list of buffers is the header comment's; nothing in the product calls these ----
static int scratch_quiesce(afv_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
    return AFV_OK;
}

// slot -> the buffers it stands for, in a fixed order; host: they are host memory (memset / memcpy), else device memory
static void scratch_segments(afv_ctx *c, std::vector<ScratchSeg> seg[AFV_SCRATCH_SLOTS]) {
    seg[AFV_SCRATCH_D_MATCH].push_back(ScratchSeg{c->d_match, c->match_bytes});
    seg[AFV_SCRATCH_H_STAGE].push_back(ScratchSeg{c->h_stage, c->stage_bytes});
    seg[AFV_SCRATCH_D_TOPK].push_back(ScratchSeg{c->d_topk, c->topk_bytes});
    seg[AFV_SCRATCH_D_SLICE].push_back(ScratchSeg{c->d_slice, c->slice_bytes});
    seg[AFV_SCRATCH_D_L2].push_back(ScratchSeg{c->d_l2_scratch, c->l2_bytes});
    for (const afv_points *p : c->points) {
        seg[AFV_SCRATCH_POINTS_STAGE].push_back(ScratchSeg{p->d_stage, p->stage_bytes});
        seg[AFV_SCRATCH_POINTS_PIN].push_back(ScratchSeg{p->h_pin, p->pin_bytes});
    }
    afv_tables_pair_scratch(c, seg[AFV_SCRATCH_TABLE_PAIRS], seg[AFV_SCRATCH_TABLE_PIN]);
    for (int i = 0; i < AFV_SCRATCH_SLOTS; ++i) {  // a buffer that was never made counts as empty
        auto &v = seg[i];
        v.erase(std::remove_if(v.begin(), v.end(), [](const ScratchSeg &s) { return !s.p || !s.n; }), v.end());
    }
}
static inline bool scratch_on_host(int slot) { return slot == AFV_SCRATCH_H_STAGE || slot == AFV_SCRATCH_POINTS_PIN || slot == AFV_SCRATCH_TABLE_PIN; }

extern "C" int afv_debug_scratch_bytes(afv_ctx *c, size_t *out, int n) {
    if (!c || !out || n < 1) return AFV_EINVAL;
    std::vector<ScratchSeg> seg[AFV_SCRATCH_SLOTS];
    scratch_segments(c, seg);
    for (int i = 0; i < n && i < AFV_SCRATCH_SLOTS; ++i) {
        out[i] = 0;
        for (const ScratchSeg &s : seg[i]) out[i] += s.n;
    }
    return AFV_OK;
}

extern "C" int afv_debug_paint_scratch(afv_ctx *c, int byte) {
    if (!c || byte < 0 || byte > 255) return AFV_EINVAL;
    int rc = scratch_quiesce(c);
    if (rc) return rc;
    for (afv_points *p : c->points)
        if (p->ev_armed) HIPCHK(c, hipEventSynchronize(p->ev));  // the stream was waited for: the upload out of h_pin is over
    std::vector<ScratchSeg> seg[AFV_SCRATCH_SLOTS];
    scratch_segments(c, seg);
    for (int i = 0; i < AFV_SCRATCH_SLOTS; ++i)
        for (const ScratchSeg &s : seg[i]) {
            if (scratch_on_host(i)) std::memset(s.p, byte, s.n);
            else HIPCHK(c, afv_fill(c, s.p, byte, s.n));
        }
    return AFV_OK;
}

extern "C" int afv_debug_rest_words(afv_ctx *c, int32_t *nonzero) {
    if (!c || !nonzero) return AFV_EINVAL;
    *nonzero = -1;
    int rc = scratch_quiesce(c);
    if (rc) return rc;
    std::vector<int32_t> w(3 + c->tickets_n, 0);
    if (c->d_proj_ticket) HIPCHK(c, hipMemcpyAsync(w.data(), c->d_proj_ticket, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (c->d_points_count) HIPCHK(c, hipMemcpyAsync(w.data() + 1, c->d_points_count, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (c->d_tickets && c->tickets_n)
        HIPCHK(c, hipMemcpyAsync(w.data() + 3, c->d_tickets, c->tickets_n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int32_t n = 0;
    for (int32_t v : w) n += v != 0;
    *nonzero = n;
    return AFV_OK;
}

extern "C" int afv_debug_scratch_read(afv_ctx *c, int which, size_t offset, void *out, size_t bytes) {
    if (!c || !out || which < 0 || which >= AFV_SCRATCH_SLOTS) return AFV_EINVAL;
    std::vector<ScratchSeg> seg[AFV_SCRATCH_SLOTS];
    scratch_segments(c, seg);
    size_t total = 0;
    for (const ScratchSeg &s : seg[which]) total += s.n;
    if (offset > total || bytes > total - offset) return AFV_EINVAL;
    int rc = scratch_quiesce(c);
    if (rc) return rc;
    uint8_t *dst = static_cast<uint8_t *>(out);
    size_t base = 0;  // the slot's buffers read as one run of bytes, in the order of scratch_segments
    for (const ScratchSeg &s : seg[which]) {
        const size_t lo = std::max(offset, base), hi = std::min(offset + bytes, base + s.n);
        if (lo < hi) {
            const uint8_t *src = static_cast<const uint8_t *>(s.p) + (lo - base);
            if (scratch_on_host(which)) std::memcpy(dst + (lo - offset), src, hi - lo);
            else HIPCHK(c, hipMemcpyAsync(dst + (lo - offset), src, hi - lo, hipMemcpyDeviceToHost, c->stream));
        }
        base += s.n;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AFV_OK;
}

extern "C" int afv_hamming256(const uint8_t *a, const uint8_t *b) {
    int d = 0;
    for (int i = 0; i < 8; ++i) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * i, 4);
        std::memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

// ---- SearchByBoW / SearchForTriangulation over host arrays: argument checks and the jobs' sides; afv_match_jobs.hip stages and launches ----
static int validate_job(const afv_match_job &j, bool need_angles) {
    if (j.n1 < 0 || j.n2 < 0 || j.n1 > AFV_MAX_SIDE || j.n2 > AFV_MAX_SIDE) return AFV_EINVAL;
    if ((j.n1 > 0 && !j.desc1) || (j.n2 > 0 && !j.desc2)) return AFV_EINVAL;
    if (j.mode & AFV_MATCH_FLOAT32) {  // float rows: desc_bytes = 4 * dim, rows 16-byte aligned in the staging blob
        if (j.desc_bytes < 16 || j.desc_bytes > 4096 || (j.desc_bytes & 15)) return AFV_EINVAL;
    } else if (j.desc_bytes < 1 || j.desc_bytes > 64) {
        return AFV_EINVAL;
    }
    if (j.nnodes1 < 0 || j.nnodes2 < 0) return AFV_EINVAL;
    if (j.nnodes1 > 0 && (!j.node_id1 || !j.seg_ptr1 || !j.seg_idx1)) return AFV_EINVAL;
    if (j.nnodes2 > 0 && (!j.node_id2 || !j.seg_ptr2 || !j.seg_idx2)) return AFV_EINVAL;
    if (need_angles && j.check_orientation && (!j.angle1 || !j.angle2)) return AFV_EINVAL;
    // the CSR FeatureVectors size host copies and index descriptors on the device
    const int rc = afv_featvec_check(j.node_id1, j.seg_ptr1, j.seg_idx1, j.nnodes1, j.n1);
    return rc ? rc : afv_featvec_check(j.node_id2, j.seg_ptr2, j.seg_idx2, j.nnodes2, j.n2);
}

// the two sides of a host-array job, appended to B.sides
static void push_job_sides(MatchBatch &B, const afv_match_job &j, bool tri) {
    const bool guided = j.nnodes1 > 0 && j.nnodes2 > 0;  // else brute force: no node structure, no index arrays on either side
    const bool frame2 = !tri && (j.mode & ~AFV_MATCH_FLOAT32) == AFV_MATCH_KF_FRAME;
    MatchSide s[2];
    for (int k = 0; k < 2; ++k) {
        s[k].desc_bytes = j.desc_bytes;
        s[k].fdim = (j.mode & AFV_MATCH_FLOAT32) ? j.desc_bytes / 4 : 0;
        s[k].words = s[k].fdim ? s[k].fdim : (j.desc_bytes <= 32 ? 8 : 16);
        s[k].n = k ? j.n2 : j.n1;
        s[k].rows = k ? j.desc2 : j.desc1;
        if (guided) {
            s[k].node_id = k ? j.node_id2 : j.node_id1;
            s[k].seg_ptr = k ? j.seg_ptr2 : j.seg_ptr1;
            s[k].idx = k ? j.seg_idx2 : j.seg_idx1;
            s[k].nnodes = k ? j.nnodes2 : j.nnodes1;
        }
        if (!tri && j.check_orientation) s[k].angle = k ? j.angle2 : j.angle1;
    }
    s[0].valid = j.valid1;
    s[1].valid = frame2 ? nullptr : j.valid2;  // KF-Frame: validity on the keyframe side only (FeatureMatcher.cc:216-232)
    B.sides.push_back(s[0]);
    B.sides.push_back(s[1]);
}

static int afv_match_bow_impl(afv_ctx *c, const afv_match_job *jobs, int njobs, int32_t *out, int32_t *nmatches) {
    if (!c || !jobs || njobs < 1 || !out || !nmatches) return AFV_EINVAL;
    for (int i = 0; i < njobs; ++i) {
        const int rc = validate_job(jobs[i], true);
        if (rc) return rc;
        const int kind = jobs[i].mode & ~AFV_MATCH_FLOAT32;
        if (kind != AFV_MATCH_KF_KF && kind != AFV_MATCH_KF_FRAME) return AFV_EINVAL;
    }
    bool taken = false;
    const int rc = afv_match_bow_plain32(c, jobs, njobs, out, nmatches, &taken);
    if (taken) return rc;
    MatchBatch B;
    B.whole_range = true;
    for (int i = 0; i < njobs; ++i) {
        const afv_match_job &j = jobs[i];
        push_job_sides(B, j, false);
        B.jobs.push_back(MatchJobSpec{2 * i, 2 * i + 1, j.th_low, j.nnratio, j.check_orientation, j.mode & ~AFV_MATCH_FLOAT32});
    }
    return afv_match_jobs_run(c, B, out, nmatches);
}
extern "C" int afv_match_bow(afv_ctx *c, const afv_match_job *jobs, int njobs, int32_t *out, int32_t *nmatches) {
    return guarded(c, [&] { return afv_match_bow_impl(c, jobs, njobs, out, nmatches); });
}

static int afv_match_triangulation_impl(afv_ctx *c, const afv_tri_job *caller_jobs, int njobs, int32_t *match12, int32_t *nmatches) {
    if (!c || !caller_jobs || njobs < 1 || !match12 || !nmatches) return AFV_EINVAL;
    std::vector<afv_tri_job> loaded;
    if (!afv_load_jobs(caller_jobs, njobs, offsetof(afv_tri_job, u_right1), loaded)) return AFV_EINVAL;
    MatchBatch B;
    B.tri = B.whole_range = true;
    for (int i = 0; i < njobs; ++i) {
        const afv_tri_job &t = loaded[i];
        const int rc = validate_job(t.bow, false);
        if (rc) return rc;
        if ((t.bow.n1 > 0 && (!t.x1 || !t.y1)) || (t.bow.n2 > 0 && (!t.x2 || !t.y2 || !t.sigma2_2))) return AFV_EINVAL;
        if (t.only_stereo != 0 && t.only_stereo != 1) return AFV_EINVAL;
        push_job_sides(B, t.bow, true);
        MatchSide &s1 = B.sides[2 * i], &s2 = B.sides[2 * i + 1];
        s1.x = t.x1, s1.y = t.y1, s1.u_right = t.u_right1;  // u_right: stereo keyframes (FeatureMatcher.cc:705, :727), null = monocular
        s2.x = t.x2, s2.y = t.y2, s2.sigma2 = t.sigma2_2, s2.u_right = t.u_right2;
        B.jobs.push_back(MatchJobSpec{2 * i, 2 * i + 1, t.bow.th_low, t.bow.nnratio, 0, AFV_MATCH_KF_KF, t.F12, t.ex, t.ey, t.only_stereo});
    }
    return afv_match_jobs_run(c, B, match12, nmatches);
}
extern "C" int afv_match_triangulation(afv_ctx *c, const afv_tri_job *jobs, int njobs, int32_t *match12, int32_t *nmatches) {
    return guarded(c, [&] { return afv_match_triangulation_impl(c, jobs, njobs, match12, nmatches); });
}

// a pair whose fixed point hit its pass guard carries nmatches = AFV_PASS_GUARD (k_match_resolve_wg): entry points that hand results to the
// host report it (never observed outside the test hook afv_debug_pass_cap)
int afv_check_resolve_guard(afv_ctx *c, const int32_t *nmatches, int n) {
    for (int i = 0; i < n; ++i)
        if (nmatches[i] == AFV_PASS_GUARD) {
            c->last_error = "pair matcher: the fixed point of pair " + std::to_string(i) + " hit its pass guard; afv_set_match_resolve(ctx, 0) selects the ordered walk";
            return AFV_EHIP;
        }
    return AFV_OK;
}

// core of the device-resident brute-force batch; angles as a strided float array (see afv_launch_match_resolve); words = dwords per row of
// d_desc (8: descriptors of up to 32 bytes, 16: 33 to 64 bytes, zero padded)
int afv_match_pairs_core(afv_ctx *c, const uint8_t *d_desc, const float *d_ang, int ang_stride, const int32_t *d_n, int cap,
                         const int32_t *d_pair_a, const int32_t *d_pair_b, int npairs, float th_low, float nnratio,
                         int check_orientation, int32_t *d_match, int32_t *d_nmatches, hipStream_t s, int words) {
    c->prof = c->prof_every && (c->prof_tick_match++ % (unsigned)c->prof_every) == 0;
    // the small-batch path deals the column tiles of phase 1 to several workgroups per row tile (two 64-column tiles each): a single
    // pair then runs on 32 workgroups instead of 4, and the resolve kernel merges the slices' key records
    const int nslices = small_batch_path(c, npairs) ? afv_match_topk_slices(cap, c->match_engine, ((cap + 63) / 64 + 1) / 2) : 1;
    {
        const int rc = ensure_slice_scratch(c, npairs, cap, nslices);
        if (rc) return rc;
    }
    const size_t need = (size_t)npairs * cap * 32;  // one 2 x int4 key record per row
    if (need > c->topk_bytes) {  // grow-only scratch (first call / larger batch): implies a device sync
        HIPCHK(c, hipDeviceSynchronize());
        if (c->d_topk) (void)hipFree(c->d_topk);
        c->d_topk = nullptr;
        c->topk_bytes = 0;
        HIPCHK(c, hipMalloc(&c->d_topk, need));
        c->topk_bytes = need;
    }
    // Schedule 1 keeps a call of up to 4096 pairs on the caller's stream.  Split over the two streams, the two top-k launches run side by
    // side at half speed each and so do the two resolves: nothing is hidden, and the fork and the join each leave the chip idle for 10 to
    // 20 us (kernel trace: profiles/r09/overlap_parent.txt).  Unsplit, the step of bench.py is 0.4 % (512 frames) to 7.6 % (64 frames)
    // shorter, 0.3 % at 1024 frames, 0.8 % on frames that really overlap (DESIGN_LOG, round 9); a call of 10 000 pairs, where two
    // hand-offs are nothing beside 3 ms of kernels, was no faster unsplit (3.10 against 3.07 ms, inside its spread) and keeps the split.  All top-k launches on one stream
    // with the resolves behind events on the other - so that a resolve runs beside the next top-k - was measured too: 2.8 % slower on
    // unrelated frames, 4 to 6 % on overlapping ones (the lone last resolve and the event hops cost more than the overlap wins).
    const bool split = npairs >= c->split_min_frames && (c->split_schedule == 0 || npairs > 4096);
    if (split) {
        // grid.y carries the pair index (<= 65535 per launch); chunk k, top-k and resolve, on stream k % 2 (more, smaller chunks were
        // measured and are slower: 256 frames, 4 / 6 / 8 chunks: -4 / -9 / -13 %)
        HIPCHK(c, hipEventRecord(c->ev_fork, s));
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
        const int K = std::max(2, (npairs + 32767) / 32768 * 2);
        for (int k = 0; k < K; ++k) {
            const int b0 = (int)((long)npairs * k / K), e0 = (int)((long)npairs * (k + 1) / K);
            if (e0 <= b0) continue;
            hipStream_t ks = (k & 1) ? c->stream2 : s;
            {
                StageTimer t_(c, AFV_STAGE_MATCH, ks, e0 - b0);
                afv_launch_match_topk(d_desc, d_n, cap, d_pair_a, d_pair_b, e0 - b0, c->d_topk, b0, c->match_engine, nslices, c->d_slice, c->d_tickets, words, ks);
            }
            StageTimer t_(c, AFV_STAGE_MATCH_RESOLVE, ks, e0 - b0);
            afv_launch_match_resolve(d_desc, d_ang, ang_stride, d_n, cap, d_pair_a, d_pair_b, e0 - b0, th_low, nnratio, check_orientation,
                                     d_match, d_nmatches, c->d_topk, b0, resolve_engine_for(c, npairs), words, ks);
        }
        HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
        HIPCHK(c, hipStreamWaitEvent(s, c->ev_join, 0));
    } else {
        {
            StageTimer t_(c, AFV_STAGE_MATCH, s, npairs);
            afv_launch_match_topk(d_desc, d_n, cap, d_pair_a, d_pair_b, npairs, c->d_topk, 0, c->match_engine, nslices, c->d_slice, c->d_tickets, words, s);
        }
        StageTimer t_(c, AFV_STAGE_MATCH_RESOLVE, s, npairs);
        afv_launch_match_resolve(d_desc, d_ang, ang_stride, d_n, cap, d_pair_a, d_pair_b, npairs, th_low, nnratio, check_orientation, d_match,
                                 d_nmatches, c->d_topk, 0, resolve_engine_for(c, npairs), words, s);
    }
    {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            // a sliced launch that did not go out (or went out half) may leave row-tile tickets behind: zero them, so that the next
            // small-batch call on this context starts from rest instead of merging early or never
            if (nslices > 1 && c->d_tickets) (void)hipMemsetAsync(c->d_tickets, 0, c->tickets_n * sizeof(int), s);
            c->last_error = std::string("pair matcher launch: ") + hipGetErrorString(e);
            return AFV_EHIP;
        }
    }
    return AFV_OK;
}

extern "C" int afv_match_bruteforce_pairs_device(afv_ctx *c, const uint8_t *d_desc, const afv_keypoint *d_kps,
                                                 const int32_t *d_n, int nsets, int cap, const int32_t *d_pair_a,
                                                 const int32_t *d_pair_b, int npairs, float th_low, float nnratio,
                                                 int check_orientation, int32_t *d_match, int32_t *d_nmatches, void *stream) {
    if (!c || !d_desc || !d_n || !d_pair_a || !d_pair_b || !d_match || !d_nmatches) return AFV_EINVAL;
    if (nsets < 1 || npairs < 1 || cap < 1 || cap > 4096) return AFV_EINVAL;  // PAIR_MAX_SIDE in k_match.hip
    if (check_orientation && !d_kps) return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    return afv_match_pairs_core(c, d_desc, d_kps ? &d_kps->angle : nullptr, (int)(sizeof(afv_keypoint) / sizeof(float)), d_n, cap,
                                d_pair_a, d_pair_b, npairs, th_low, nnratio, check_orientation, d_match, d_nmatches,
                                stream ? (hipStream_t)stream : c->stream, 8);
}

static int afv_match_l2_impl(afv_ctx *c, const float *desc1, int n1, const float *desc2, int n2, int dim, const uint8_t *valid1,
                            const uint8_t *valid2, float th_low, float nnratio, int32_t *match12, int32_t *nmatches) {
    if (!c || !match12 || !nmatches || n1 < 0 || n2 < 0 || n1 > AFV_MAX_SIDE || n2 > AFV_MAX_SIDE || dim < 1 || dim > 1024)
        return AFV_EINVAL;
    if ((n1 > 0 && !desc1) || (n2 > 0 && !desc2)) return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    Blob b(c);
    const size_t o1 = b.put(desc1, (size_t)n1 * dim * 4), o2 = b.put(desc2, (size_t)n2 * dim * 4);
    const size_t ov1 = valid1 ? b.put(valid1, (size_t)n1) : 0, ov2 = valid2 ? b.put(valid2, (size_t)n2) : 0;
    const size_t in_bytes = b.h.size();
    const size_t oo = b.reserve((size_t)std::max(n1, 1) * 4), on = b.reserve(4);
    int ntiles = 1, cols_per_tile = 32;
    const size_t ok = b.reserve_scratch(afv_match_l2_scratch_bytes(n1, n2, &ntiles, &cols_per_tile));
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    HIPCHK(c, b.upload(in_bytes));
    const float *p1 = reinterpret_cast<const float *>(c->d_match + o1), *p2 = reinterpret_cast<const float *>(c->d_match + o2);
    const uint8_t *pv1 = valid1 ? c->d_match + ov1 : nullptr, *pv2 = valid2 ? c->d_match + ov2 : nullptr;
    int *pout = reinterpret_cast<int *>(c->d_match + oo), *pn = reinterpret_cast<int *>(c->d_match + on);
    if (!afv_launch_match_l2_tiled(p1, n1, p2, n2, dim, pv1, pv2, th_low, nnratio, pout, pn, c->d_match + ok, ntiles, cols_per_tile, c->stream))
        afv_launch_match_l2(p1, n1, p2, n2, dim, pv1, pv2, th_low, nnratio, pout, pn, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, b.fetch(match12, oo, (size_t)n1 * 4, c->stream));
    HIPCHK(c, b.fetch(nmatches, on, 4, c->stream));
    HIPCHK(c, b.wait());
    return AFV_OK;
}
extern "C" int afv_match_l2(afv_ctx *c, const float *desc1, int n1, const float *desc2, int n2, int dim, const uint8_t *valid1,
                            const uint8_t *valid2, float th_low, float nnratio, int32_t *match12, int32_t *nmatches) {
    return guarded(c, [&] { return afv_match_l2_impl(c, desc1, n1, desc2, n2, dim, valid1, valid2, th_low, nnratio, match12, nmatches); });
}

// device-resident batch of the float-descriptor matcher (config #3 as a throughput path, like afv_match_bruteforce_pairs_device for
// ORB32): the key scratch is the Hamming path's grow-only buffer (32 B per row there as well)
int afv_match_l2_pairs_core(afv_ctx *c, const float *d_desc, const float *d_ang, const int32_t *d_n, int cap, int dim, const int32_t *d_pair_a,
                            const int32_t *d_pair_b, int npairs, float th_low, float nnratio, int32_t *d_match, int32_t *d_nmatches, hipStream_t s) {
    const int chunk = std::min(npairs, c->l2_chunk_pairs);  // pairs per launch: grid.y and the scratch stay bounded
    // the float matcher's own key scratch: the Hamming pair calls keep theirs (d_topk) busy on the context's streams, and a caller
    // may run the two kinds on different streams of one context
    const size_t need = (size_t)chunk * cap * 32;
    if (need > c->l2_bytes) {  // grow-only (first call / larger batch): implies a device sync
        HIPCHK(c, hipDeviceSynchronize());
        if (c->d_l2_scratch) (void)hipFree(c->d_l2_scratch);
        c->d_l2_scratch = nullptr;
        c->l2_bytes = 0;
        HIPCHK(c, hipMalloc(&c->d_l2_scratch, need));
        c->l2_bytes = need;
    }
    // chunks reuse the scratch one after the other: same stream, so chunk k + 1 starts after chunk k has read its keys
    for (int b0 = 0; b0 < npairs; b0 += chunk)
        if (!afv_launch_match_l2_pairs(d_desc, d_n, cap, dim, d_pair_a, d_pair_b, std::min(chunk, npairs - b0), b0, th_low, nnratio, d_ang, d_match,
                                       d_nmatches, c->d_l2_scratch, s))
            return AFV_EUNSUPPORTED;
    HIPCHK(c, hipGetLastError());
    return AFV_OK;
}

extern "C" int afv_match_l2_pairs_device(afv_ctx *c, const float *d_desc, const int32_t *d_n, int cap, int dim, const int32_t *d_pair_a,
                                         const int32_t *d_pair_b, int npairs, float th_low, float nnratio, int32_t *d_match,
                                         int32_t *d_nmatches, void *stream) {
    return guarded(c, [&]() -> int {
        if (!c || !d_desc || !d_n || !d_pair_a || !d_pair_b || !d_match || !d_nmatches || npairs < 0 || cap < 1 || cap > AFV_MAX_SIDE)
            return AFV_EINVAL;
        if (dim != 64 && dim != 128) return AFV_EUNSUPPORTED;
        if (npairs == 0) return AFV_OK;
        HIPCHK(c, hipSetDevice(c->device));
        return afv_match_l2_pairs_core(c, d_desc, nullptr, d_n, cap, dim, d_pair_a, d_pair_b, npairs, th_low, nnratio, d_match, d_nmatches,
                                       stream ? (hipStream_t)stream : c->stream);
    });
}

// ---- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:279-349) for a batch of map points ----
extern "C" int afv_distinctive_descriptors(afv_ctx *c, const uint8_t *desc, int desc_bytes, const int32_t *set_ptr, int nsets, int32_t *best_idx,
                                           int32_t *best_median) {
    if (!c || !set_ptr || nsets < 0 || desc_bytes < 1 || desc_bytes > 64 || (nsets > 0 && !best_idx)) return AFV_EINVAL;
    if (nsets == 0) return AFV_OK;
    if (set_ptr[0] != 0) return AFV_EINVAL;
    for (int s = 0; s < nsets; ++s)
        if (set_ptr[s + 1] < set_ptr[s] || set_ptr[s + 1] - set_ptr[s] > 65535) return AFV_EINVAL;  // (the kernel's key holds the row in 16 bits)
    const int total = set_ptr[nsets];
    if (total > 0 && !desc) return AFV_EINVAL;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        Blob b(c);
        const int words = desc_bytes <= 32 ? 8 : 16;
        const size_t d_off = put_desc(b, desc, total, desc_bytes, words);
        const size_t p_off = b.put(set_ptr, (size_t)(nsets + 1) * 4);
        const size_t in_bytes = b.h.size();
        const size_t bi_off = b.reserve((size_t)nsets * 4), bm_off = b.reserve((size_t)nsets * 4);
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        HIPCHK(c, b.upload(in_bytes));
        afv_launch_distinctive(reinterpret_cast<const uint32_t *>(c->d_match + d_off), reinterpret_cast<const int *>(c->d_match + p_off), nsets, words,
                               desc_bytes, reinterpret_cast<int *>(c->d_match + bi_off), reinterpret_cast<int *>(c->d_match + bm_off), c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, b.fetch(best_idx, bi_off, (size_t)nsets * 4, c->stream));
        if (best_median) HIPCHK(c, b.fetch(best_median, bm_off, (size_t)nsets * 4, c->stream));
        HIPCHK(c, b.wait());
        return AFV_OK;
    });
}

extern "C" int afv_distinctive_descriptors_f32(afv_ctx *c, const float *desc, int dim, const int32_t *set_ptr, int nsets, int32_t *best_idx,
                                               float *best_median) {
    if (!c || !set_ptr || nsets < 0 || dim < 1 || dim > 1024 || (nsets > 0 && !best_idx)) return AFV_EINVAL;
    if (nsets == 0) return AFV_OK;
    if (set_ptr[0] != 0) return AFV_EINVAL;
    for (int s = 0; s < nsets; ++s)
        if (set_ptr[s + 1] < set_ptr[s] || set_ptr[s + 1] - set_ptr[s] > 65535) return AFV_EINVAL;
    const int total = set_ptr[nsets];
    if (total > 0 && !desc) return AFV_EINVAL;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        Blob b(c);
        const size_t d_off = b.put(desc, (size_t)total * dim * 4);
        const size_t p_off = b.put(set_ptr, (size_t)(nsets + 1) * 4);
        const size_t in_bytes = b.h.size();
        const size_t bi_off = b.reserve((size_t)nsets * 4), bm_off = b.reserve((size_t)nsets * 4);
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        HIPCHK(c, b.upload(in_bytes));
        afv_launch_distinctive_f32(reinterpret_cast<const float *>(c->d_match + d_off), dim, reinterpret_cast<const int *>(c->d_match + p_off), nsets,
                                   reinterpret_cast<int *>(c->d_match + bi_off), reinterpret_cast<float *>(c->d_match + bm_off), c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, b.fetch(best_idx, bi_off, (size_t)nsets * 4, c->stream));
        if (best_median) HIPCHK(c, b.fetch(best_median, bm_off, (size_t)nsets * 4, c->stream));
        HIPCHK(c, b.wait());
        return AFV_OK;
    });
}

// ---- BoW quantisation ----
// the tree image of k_bow.hip for node descriptors of `words` dwords each (binary: 8 or 16, zero-padded; float: the dimension)
static int vocab_create_impl(afv_ctx *c, int k, int L, int nnodes, const int32_t *child_ptr, const int32_t *child_idx, const uint8_t *desc, int desc_bytes,
                             int words, int float_dim, afv_vocab **out);

extern "C" int afv_vocab_create(afv_ctx *c, int k, int L, int nnodes, const int32_t *child_ptr, const int32_t *child_idx,
                                const uint8_t *desc, int desc_bytes, afv_vocab **out) {
    if (!c || !out || !child_ptr || !child_idx || !desc || k < 1 || L < 1 || nnodes < 1 || desc_bytes < 1 || desc_bytes > 64)
        return AFV_EINVAL;
    return vocab_create_impl(c, k, L, nnodes, child_ptr, child_idx, desc, desc_bytes, desc_bytes <= 32 ? 8 : 16, 0, out);
}

// float node descriptors (the non-binary cases of Vocabulary::transform, Vocabulary.cpp:158-187): dim = 64 (SURF64 / KAZE64), 128 (SIFT128 / R2D2) or 256
extern "C" int afv_vocab_create_f32(afv_ctx *c, int k, int L, int nnodes, const int32_t *child_ptr, const int32_t *child_idx, const float *desc, int dim,
                                    afv_vocab **out) {
    if (!c || !out || !child_ptr || !child_idx || !desc || k < 1 || L < 1 || nnodes < 1 || (dim != 64 && dim != 128 && dim != 256)) return AFV_EINVAL;
    return vocab_create_impl(c, k, L, nnodes, child_ptr, child_idx, reinterpret_cast<const uint8_t *>(desc), dim * 4, dim, dim, out);
}

static int vocab_create_impl(afv_ctx *c, int k, int L, int nnodes, const int32_t *child_ptr, const int32_t *child_idx, const uint8_t *desc, int desc_bytes,
                             int words, int float_dim, afv_vocab **out) {
    *out = nullptr;
    const int nchild = child_ptr[nnodes];
    if (child_ptr[0] != 0 || nchild < 0 || nchild > nnodes) return AFV_EINVAL;
    for (int i = 0; i < nnodes; ++i)
        if (child_ptr[i + 1] < child_ptr[i]) return AFV_EINVAL;
    {   // a tree: every non-root node is the child of exactly one node (no duplicates => no cycles reachable from the
        // root, so the descent of k_bow_transform terminates)
        std::vector<uint8_t> seen((size_t)nnodes, 0);
        for (int i = 0; i < nchild; ++i) {
            if (child_idx[i] <= 0 || child_idx[i] >= nnodes || seen[child_idx[i]]) return AFV_EINVAL;
            seen[child_idx[i]] = 1;
        }
        // ... and no node is its own ancestor: walk the levels from the root, at most L of them may have children
        std::vector<int> frontier{0}, next;
        for (int depth = 0; !frontier.empty(); ++depth) {
            next.clear();
            for (int nd : frontier)
                for (int q = child_ptr[nd]; q < child_ptr[nd + 1]; ++q) next.push_back(child_idx[q]);
            if (!next.empty() && depth >= L) return AFV_EINVAL;
            frontier.swap(next);
        }
    }
    for (int i = 0; i < nnodes; ++i)
        if (child_ptr[i + 1] - child_ptr[i] > 65535) return AFV_EINVAL;  // the descent's key carries the child position in 16 bits
    HIPCHK(c, hipSetDevice(c->device));
    afv_vocab *v = new (std::nothrow) afv_vocab();
    if (!v) return AFV_ENOMEM;
    v->desc_bytes = desc_bytes;
    v->float_dim = float_dim;
    const int RD = words + 4;
    // device image (k_bow.hip): nodes renumbered breadth first, the children of a node consecutive and in DBoW2 order; record =
    // descriptor | first child record | #children | DBoW2 id | 0.  Nodes the root does not reach keep no record.
    std::vector<int> order;  // record -> DBoW2 id
    order.reserve((size_t)nnodes);
    order.push_back(0);
    std::vector<uint32_t> rec((size_t)nnodes * RD, 0);
    std::vector<int> depth((size_t)nnodes, -1);  // by DBoW2 id; -1: not reachable from the root
    depth[0] = 0;
    for (size_t r = 0; r < order.size(); ++r) {
        const int id = order[r];
        for (int q = child_ptr[id]; q < child_ptr[id + 1]; ++q) depth[child_idx[q]] = depth[id] + 1;
        uint32_t *R = rec.data() + r * RD;
        std::memcpy(R, desc + (size_t)id * desc_bytes, (size_t)desc_bytes);
        const int nc = child_ptr[id + 1] - child_ptr[id];
        R[words] = (uint32_t)order.size();
        R[words + 1] = (uint32_t)nc;
        R[words + 2] = (uint32_t)id;
        for (int q = child_ptr[id]; q < child_ptr[id + 1]; ++q) order.push_back(child_idx[q]);
    }
    {   // rank of every node among the nodes of its depth, ascending DBoW2 id: the FeatureVector's sort key (k_featvec_build)
        std::vector<int> rank_of((size_t)nnodes, 0);
        v->depth_width.clear();
        for (int id = 0; id < nnodes; ++id) {
            if (depth[id] < 0) continue;
            if ((size_t)depth[id] >= v->depth_width.size()) v->depth_width.resize((size_t)depth[id] + 1, 0);
            rank_of[id] = v->depth_width[(size_t)depth[id]]++;
        }
        for (size_t r = 0; r < order.size(); ++r) rec[r * RD + words + 3] = (uint32_t)rank_of[order[r]];
    }
    hipError_t e = hipMalloc(&v->d_rec, rec.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(v->d_rec, rec.data(), rec.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        c->last_error = std::string("afv_vocab_create: ") + hipGetErrorString(e);
        afv_vocab_destroy(c, v);
        return e == hipErrorOutOfMemory ? AFV_ENOMEM : AFV_EHIP;
    }
    v->dev = DevVocab{k, L, nnodes, words, RD, (const uint32_t *)v->d_rec, nullptr};
    *out = v;
    return AFV_OK;
}

extern "C" int afv_vocab_set_stopped(afv_ctx *c, afv_vocab *v, const uint8_t *stopped) {
    if (!c || !v) return AFV_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!stopped) {
        v->dev.stopped = nullptr;
        v->h_stopped.clear();
        return AFV_OK;
    }
    try {
        v->h_stopped.assign(stopped, stopped + v->dev.nnodes);
    } catch (...) {
        return AFV_ENOMEM;
    }
    if (!v->d_stopped) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&v->d_stopped), (size_t)v->dev.nnodes));
    HIPCHK(c, hipMemcpy(v->d_stopped, stopped, (size_t)v->dev.nnodes, hipMemcpyHostToDevice));
    v->dev.stopped = v->d_stopped;
    return AFV_OK;
}

// word weights: what DBoW2 transform adds to the BowVector (k_bowvec.hip)
extern "C" int afv_vocab_set_weights(afv_ctx *c, afv_vocab *v, const double *weight, const int32_t *word_id) {
    if (!c || !v || (weight && !word_id)) return AFV_EINVAL;
    const int nn = v->dev.nnodes;
    int max_word = -1;
    if (weight) {  // a word id names one node
        for (int i = 0; i < nn; ++i) {
            if (word_id[i] < -1) return AFV_EINVAL;
            max_word = std::max(max_word, word_id[i]);
        }
        if (max_word >= nn) return AFV_EINVAL;
    }
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (void *p : {(void *)v->d_weight, (void *)v->d_word_id, (void *)v->d_word_weight})
            if (p) (void)hipFree(p);
        v->d_weight = v->d_word_weight = nullptr;
        v->d_word_id = nullptr;
        if (!weight) return AFV_OK;
        std::vector<double> by_word((size_t)max_word + 1, 0.0);
        std::vector<uint8_t> seen((size_t)max_word + 1, 0);
        for (int i = 0; i < nn; ++i)
            if (word_id[i] >= 0) {
                if (seen[(size_t)word_id[i]]) return AFV_EINVAL;
                seen[(size_t)word_id[i]] = 1;
                by_word[(size_t)word_id[i]] = weight[i];
            }
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&v->d_weight), (size_t)nn * sizeof(double));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&v->d_word_id), (size_t)nn * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&v->d_word_weight), std::max<size_t>(by_word.size(), 1) * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(v->d_weight, weight, (size_t)nn * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(v->d_word_id, word_id, (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess && !by_word.empty()) e = hipMemcpy(v->d_word_weight, by_word.data(), by_word.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            for (void *p : {(void *)v->d_weight, (void *)v->d_word_id, (void *)v->d_word_weight})
                if (p) (void)hipFree(p);
            v->d_weight = v->d_word_weight = nullptr;
            v->d_word_id = nullptr;
        }
        HIPCHK(c, e);
        return AFV_OK;
    });
}

extern "C" int afv_bow_vector(afv_ctx *c, const afv_vocab *v, const int32_t *leaf_node, int n, int32_t *word, double *value, int32_t *n_out) {
    if (!c || !v || !n_out || n < 0 || n > AFV_BOW_MAX_ENTRIES || (n > 0 && (!leaf_node || !word || !value))) return AFV_EINVAL;
    if (!v->d_weight) return AFV_EINVAL;  // afv_vocab_set_weights first
    for (int i = 0; i < n; ++i)
        if (leaf_node[i] < 0 || leaf_node[i] >= v->dev.nnodes) return AFV_EINVAL;
    *n_out = 0;
    if (n == 0) return AFV_OK;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        Blob b(c);
        const size_t leaf_off = b.put(leaf_node, (size_t)n * 4);
        const size_t in_bytes = b.h.size();
        const size_t n_off = b.reserve_scratch(16), word_off = b.reserve_scratch((size_t)n * 4), val_off = b.reserve_scratch((size_t)n * 8);
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        HIPCHK(c, b.upload(in_bytes));
        afv_launch_bowvec_build(reinterpret_cast<const int *>(c->d_match + leaf_off), n, v->d_weight, v->d_word_id, v->d_word_weight,
                                reinterpret_cast<int32_t *>(c->d_match + word_off), reinterpret_cast<double *>(c->d_match + val_off),
                                reinterpret_cast<int *>(c->d_match + n_off), c->stream);
        HIPCHK(c, hipGetLastError());
        // the entries land in the arena first: the caller's arrays hold n entries, the kernel wrote at most that many
        HIPCHK(c, b.fetch(n_out, n_off, 4, c->stream));
        HIPCHK(c, b.fetch(word, word_off, (size_t)n * 4, c->stream));
        HIPCHK(c, b.fetch(value, val_off, (size_t)n * 8, c->stream));
        HIPCHK(c, b.wait());
        return AFV_OK;
    });
}

extern "C" void afv_vocab_destroy(afv_ctx *c, afv_vocab *v) {
    if (!v) return;
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    if (v->d_rec) (void)hipFree(v->d_rec);
    if (v->d_stopped) (void)hipFree(v->d_stopped);
    if (v->d_weight) (void)hipFree(v->d_weight);
    if (v->d_word_id) (void)hipFree(v->d_word_id);
    if (v->d_word_weight) (void)hipFree(v->d_word_weight);
    delete v;
}

static int afv_bow_transform_impl(afv_ctx *c, const afv_vocab *v, const uint8_t *desc, int n, int levelsup, int32_t *leaf_node,
                                 int32_t *node_at_level) {
    if (!c || !v || n < 0 || (n > 0 && (!desc || !leaf_node || !node_at_level))) return AFV_EINVAL;
    if (v->float_dim) return AFV_EINVAL;  // a float vocabulary: afv_bow_transform_f32
    if (n == 0) return AFV_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Blob b(c);
    const size_t d_off = put_desc(b, desc, n, v->desc_bytes, v->dev.words);
    const size_t in_bytes = b.h.size();
    const size_t leaf_off = b.reserve((size_t)n * 4), nid_off = b.reserve((size_t)n * 4);
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    HIPCHK(c, b.upload(in_bytes));
    afv_launch_bow_transform(&v->dev, reinterpret_cast<const uint32_t *>(c->d_match + d_off), n, levelsup,
                             reinterpret_cast<int *>(c->d_match + leaf_off), reinterpret_cast<int *>(c->d_match + nid_off), nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, b.fetch(leaf_node, leaf_off, (size_t)n * 4, c->stream));
    HIPCHK(c, b.fetch(node_at_level, nid_off, (size_t)n * 4, c->stream));
    HIPCHK(c, b.wait());
    return AFV_OK;
}
extern "C" int afv_bow_transform(afv_ctx *c, const afv_vocab *v, const uint8_t *desc, int n, int levelsup, int32_t *leaf_node,
                                 int32_t *node_at_level) {
    return guarded(c, [&] { return afv_bow_transform_impl(c, v, desc, n, levelsup, leaf_node, node_at_level); });
}

extern "C" int afv_bow_transform_f32(afv_ctx *c, const afv_vocab *v, const float *desc, int n, int levelsup, int32_t *leaf_node, int32_t *node_at_level) {
    if (!c || !v || n < 0 || (n > 0 && (!desc || !leaf_node || !node_at_level))) return AFV_EINVAL;
    if (!v->float_dim) return AFV_EINVAL;  // a binary vocabulary: afv_bow_transform
    if (n == 0) return AFV_OK;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        Blob b(c);
        const size_t d_off = b.put(desc, (size_t)n * v->float_dim * 4);
        const size_t in_bytes = b.h.size();
        const size_t leaf_off = b.reserve((size_t)n * 4), nid_off = b.reserve((size_t)n * 4);
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        HIPCHK(c, b.upload(in_bytes));
        if (!afv_launch_bow_transform_f32(&v->dev, reinterpret_cast<const float *>(c->d_match + d_off), n, v->float_dim, levelsup,
                                          reinterpret_cast<int *>(c->d_match + leaf_off), reinterpret_cast<int *>(c->d_match + nid_off), nullptr, c->stream))
            return AFV_EUNSUPPORTED;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, b.fetch(leaf_node, leaf_off, (size_t)n * 4, c->stream));
        HIPCHK(c, b.fetch(node_at_level, nid_off, (size_t)n * 4, c->stream));
        HIPCHK(c, b.wait());
        return AFV_OK;
    });
}
