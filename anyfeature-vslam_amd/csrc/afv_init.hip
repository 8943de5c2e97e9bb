// afv_init.hip — host side of afv_frame_initializer (include/afv_hip.h, "Initializer"; kernels: k_init.hip).
//
// Reference call shape: Tracking::MonocularInitialization (src/Tracking.cc:473-487) hands the matches of SearchForInitialization to
// Initializer::Initialize, which spends two host threads on the H and F RANSAC and repeats the whole job for every frame until it
// succeeds.  Here matches12 goes up in one copy, three launches run on the context's stream and the host waits once; the two frames'
// mvKeysUn planes are read where they live.
#include <cmath>

#include "afv_runtime.h"

static bool init_frame_ready(const afv_frame *f) { return f->has_features && (!f->p.distorted || f->has_grid); }

static int init_impl(afv_frame *f1, afv_frame *f2, const afv_init_job &job, const int32_t *matches12, int N, int32_t *ok, int32_t *route,
                     float *R21, float *t21, float *p3d, uint8_t *triangulated, afv_init_trace *trace, float *hyp_score, float *hyp_model,
                     uint8_t *hyp_degenerate, uint32_t *hyp_inliers, int mask_words) {
    afv_ctx *c = f1->c;
    HIPCHK(c, hipSetDevice(c->device));
    const int n1 = f1->n, it = job.iterations;
    const size_t rows = (size_t)std::max(n1, 1), hyps = 2 * (size_t)it;
    const int mw = std::max((N + 31) / 32, 1);  // the device's row width; the caller's rows are padded or cut to mask_words below
    Blob b(c);
    const size_t o_m = b.put(matches12, (size_t)n1 * 4);
    const size_t in_bytes = b.h.size();
    const size_t o_n = b.reserve_scratch(4), o_pairs = b.reserve_scratch(rows * 8), o_norm = b.reserve_scratch(32);
    const size_t o_sets = b.reserve_scratch((size_t)it * 32), o_score = b.reserve_scratch(hyps * 4), o_model = b.reserve_scratch(hyps * 36);
    const size_t o_deg = b.reserve_scratch(hyps), o_inl = b.reserve_scratch(hyps * mw * 4);
    const size_t o_cos = b.reserve_scratch(AFV_INIT_MAX_MOTIONS * rows * 4), o_p3dk = b.reserve_scratch(AFV_INIT_MAX_MOTIONS * rows * 12);
    const size_t o_status = b.reserve_scratch(AFV_INIT_MAX_MOTIONS * rows), o_trace = b.reserve_scratch(sizeof(afv_init_trace));
    const size_t o_answer = b.reserve_scratch(8), o_rt = b.reserve_scratch(48), o_p3d = b.reserve_scratch(rows * 12), o_tri = b.reserve_scratch(rows);
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    uint8_t *B = c->d_match;
    HIPCHK(c, b.upload(in_bytes));
    DevInitArgs A{};
    A.x1 = f1->d_x; A.y1 = f1->d_y; A.x2 = f2->d_x; A.y2 = f2->d_y;
    A.n1 = n1; A.n2 = f2->n;
    A.matches12 = reinterpret_cast<const int *>(B + o_m);
    A.iterations = it; A.mask_words = mw;
    A.seed = ((unsigned long long)job.seed_hi << 32) | job.seed_lo;
    A.fx = job.fx; A.fy = job.fy; A.cx = job.cx; A.cy = job.cy; A.sigma = job.sigma;
    A.n = reinterpret_cast<int *>(B + o_n); A.pairs = reinterpret_cast<int *>(B + o_pairs); A.norm = reinterpret_cast<float *>(B + o_norm);
    A.sets = reinterpret_cast<int *>(B + o_sets); A.score = reinterpret_cast<float *>(B + o_score);
    A.model = reinterpret_cast<float *>(B + o_model); A.degenerate = B + o_deg; A.inliers = reinterpret_cast<uint32_t *>(B + o_inl);
    A.cosv = reinterpret_cast<float *>(B + o_cos); A.p3dk = reinterpret_cast<float *>(B + o_p3dk); A.status = B + o_status;
    A.trace = reinterpret_cast<afv_init_trace *>(B + o_trace); A.answer = reinterpret_cast<int *>(B + o_answer);
    A.Rt = reinterpret_cast<float *>(B + o_rt); A.p3d = reinterpret_cast<float *>(B + o_p3d); A.triangulated = B + o_tri;
    afv_launch_init(&A, c->stream);
    HIPCHK(c, hipGetLastError());
    int32_t answer[2];
    float Rt[12];
    afv_init_trace tr;
    std::vector<uint32_t> words;
    HIPCHK(c, b.fetch(answer, o_answer, 8, c->stream));
    HIPCHK(c, b.fetch(Rt, o_rt, 48, c->stream));
    HIPCHK(c, b.fetch(p3d, o_p3d, (size_t)n1 * 12, c->stream));
    HIPCHK(c, b.fetch(triangulated, o_tri, (size_t)n1, c->stream));
    if (trace) HIPCHK(c, b.fetch(&tr, o_trace, sizeof(tr), c->stream));
    if (hyp_score) HIPCHK(c, b.fetch(hyp_score, o_score, hyps * 4, c->stream));
    if (hyp_model) HIPCHK(c, b.fetch(hyp_model, o_model, hyps * 36, c->stream));
    if (hyp_degenerate) HIPCHK(c, b.fetch(hyp_degenerate, o_deg, hyps, c->stream));
    if (hyp_inliers && mask_words > 0) {
        words.resize(hyps * mw);
        HIPCHK(c, b.fetch(words.data(), o_inl, hyps * mw * 4, c->stream));
    }
    HIPCHK(c, b.wait());  // the call's one wait
    *ok = answer[0];
    *route = answer[1];
    std::memcpy(R21, Rt, 36);
    std::memcpy(t21, Rt + 9, 12);
    if (trace) {
        tr.struct_size = (uint32_t)sizeof(afv_init_trace);
        *trace = tr;
    }
    if (hyp_inliers && mask_words > 0)
        for (size_t h = 0; h < hyps; ++h) {
            uint32_t *dst = hyp_inliers + h * (size_t)mask_words;
            const int copy = std::min(mw, mask_words);
            std::memcpy(dst, words.data() + h * mw, (size_t)copy * 4);
            if (mask_words > copy) std::memset(dst + copy, 0, (size_t)(mask_words - copy) * 4);
        }
    return AFV_OK;
}

extern "C" int afv_frame_initializer(afv_frame *f1, afv_frame *f2, const afv_init_job *caller_job, const int32_t *matches12, int32_t *ok,
                                     int32_t *route, float *R21, float *t21, float *p3d, uint8_t *triangulated, afv_init_trace *trace,
                                     float *hyp_score, float *hyp_model, uint8_t *hyp_degenerate, uint32_t *hyp_inliers, int mask_words) {
    if (!f1 || !f2 || !caller_job || !ok || !route || !R21 || !t21) return AFV_EINVAL;
    if (!afv_frame_is_live(f1) || !afv_frame_is_live(f2) || f1->c != f2->c) return AFV_EINVAL;
    if (!init_frame_ready(f1) || !init_frame_ready(f2)) return AFV_EINVAL;
    if (f1->n > 0 && (!matches12 || !p3d || !triangulated)) return AFV_EINVAL;
    if (mask_words < 0 || mask_words > AFV_INIT_MAX_MASK_WORDS) return AFV_EINVAL;
    if (trace && trace->struct_size != sizeof(afv_init_trace)) return AFV_EINVAL;
    std::vector<afv_init_job> jobs;
    if (!afv_load_jobs(caller_job, 1, sizeof(afv_init_job), jobs)) return AFV_EINVAL;
    const afv_init_job &job = jobs[0];
    if (job.iterations < 1 || job.iterations > AFV_INIT_MAX_ITERATIONS) return AFV_EINVAL;
    if (!(std::isfinite(job.sigma) && job.sigma > 0) || !(std::isfinite(job.fx) && job.fx > 0) || !(std::isfinite(job.fy) && job.fy > 0) ||
        !std::isfinite(job.cx) || !std::isfinite(job.cy))
        return AFV_EINVAL;
    int N = 0;
    for (int i = 0; i < f1->n; ++i) {
        if (matches12[i] < -1 || matches12[i] >= f2->n) return AFV_EINVAL;
        N += matches12[i] >= 0;
    }
    if (hyp_inliers && (long long)mask_words * 32 < N) return AFV_EINVAL;
    return guarded(f1->c, [&] {
        return init_impl(f1, f2, job, matches12, N, ok, route, R21, t21, p3d, triangulated, trace, hyp_score, hyp_model, hyp_degenerate,
                         hyp_inliers, mask_words);
    });
}
