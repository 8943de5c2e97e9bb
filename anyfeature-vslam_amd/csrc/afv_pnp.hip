// afv_pnp.hip — host side of afv_frame_pnp_hypotheses (include/afv_hip.h, "PnPsolver"; kernels: k_pnp.hip).
//
// Reference call shape: Tracking::Relocalization (src/Tracking.cc:1190-1216) builds one PnPsolver per candidate keyframe on the host and
// iterates them round-robin, five RANSAC hypotheses at a time.  Here the rows of up to 64 candidates go up in one copy, three launches run
// on the context's stream and the host waits once: k_pnp_gather is every solver's constructor, k_pnp_hypotheses evaluates every
// hypothesis of every candidate, k_pnp_refine the Refine of every record.  The scan of PnPsolver::iterate over the counts is the caller's.
// The staging follows afv_sim3.hip.
#include <cmath>

#include "afv_runtime.h"

static int pnp_impl(afv_frame *f, afv_points *points, const afv_pnp_job *caller_jobs, int nc, const int32_t *pts, int nhyp, int mask_words,
                    int32_t *n, int32_t *min_inliers, int32_t *index, int32_t *count, uint8_t *degenerate, float *pose, uint32_t *inliers,
                    uint8_t *refined, int32_t *refined_count, float *refined_pose, uint32_t *refined_inliers, float *max_err, float *p3dw) {
    afv_ctx *c = f->c;
    std::vector<afv_pnp_job> jobs;
    if (!afv_load_jobs(caller_jobs, nc, sizeof(afv_pnp_job), jobs)) return AFV_EINVAL;
    const int nf = f->n;
    long long most = 0;
    for (int k = 0; k < nc; ++k) {
        const afv_pnp_job &j = jobs[(size_t)k];
        if (j.min_inliers < 4 || !std::isfinite(j.epsilon) || !(j.epsilon > 0.0f) || !std::isfinite(j.th2) || !(j.th2 > 0.0f)) {
            c->last_error = "afv_frame_pnp_hypotheses: candidate " + std::to_string(k) + " wants min_inliers >= 4 and finite epsilon, th2 > 0";
            return AFV_EINVAL;
        }
        long long countable = 0;
        for (int i = 0; i < nf; ++i) {
            const int p = pts[(size_t)k * nf + i];
            if (p < -1 || p >= points->cap) {
                c->last_error = "afv_frame_pnp_hypotheses: candidate " + std::to_string(k) + " names a map-point id outside the store";
                return AFV_EINVAL;
            }
            countable += p >= 0;
        }
        most = std::max(most, countable);
    }
    if ((long long)mask_words * 32 < most) {
        c->last_error = "afv_frame_pnp_hypotheses: mask_words " + std::to_string(mask_words) + " cannot hold " + std::to_string(most) + " correspondences";
        return AFV_EINVAL;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)nc * nf, hyps = (size_t)nc * nhyp;
    std::vector<DevPnpCand> dc((size_t)nc);
    for (int k = 0; k < nc; ++k) {
        const afv_pnp_job &j = jobs[(size_t)k];
        DevPnpCand &D = dc[(size_t)k];
        D = DevPnpCand{};
        D.seed = ((unsigned long long)j.seed_hi << 32) | j.seed_lo;
        D.min_inliers = j.min_inliers;
        D.epsilon = j.epsilon;
        D.th2 = j.th2;
    }
    Blob b(c);
    const size_t o_cands = b.put(dc.data(), dc.size() * sizeof(DevPnpCand));
    const size_t o_pts = b.put(pts, cells * 4);
    const size_t in_bytes = b.h.size();
    const size_t words = std::max<size_t>(hyps * (size_t)mask_words * 4, 4);
    const size_t o_n = b.reserve_scratch((size_t)nc * 4), o_min = b.reserve_scratch((size_t)nc * 4), o_index = b.reserve_scratch(cells * 4);
    const size_t o_p2d = b.reserve_scratch(cells * 8), o_p3d = b.reserve_scratch(cells * 12), o_err = b.reserve_scratch(cells * 4);
    const size_t o_count = b.reserve_scratch(hyps * 4), o_deg = b.reserve_scratch(hyps), o_pose = b.reserve_scratch(hyps * 48);
    const size_t o_inl = b.reserve_scratch(words);
    const size_t o_ref = b.reserve_scratch(hyps), o_rcount = b.reserve_scratch(hyps * 4), o_rpose = b.reserve_scratch(hyps * 48);
    const size_t o_rinl = b.reserve_scratch(words);
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    uint8_t *B = c->d_match;
    HIPCHK(c, b.upload(in_bytes));
    DevPnpArgs A{};
    A.cands = reinterpret_cast<const DevPnpCand *>(B + o_cands);
    A.pts = reinterpret_cast<const int *>(B + o_pts);
    A.nc = nc; A.nf = nf; A.nhyp = nhyp; A.mask_words = mask_words;
    A.x = f->d_x; A.y = f->d_y; A.sigma2 = f->d_sigma2;
    A.fx = f->fx; A.fy = f->fy; A.cx = f->cx; A.cy = f->cy;
    for (int k = 0; k < 3; ++k) A.pos[k] = points->P.pos[k];
    A.flags = points->P.flags;
    A.pcap = points->cap;
    A.n = reinterpret_cast<int *>(B + o_n); A.min_inliers = reinterpret_cast<int *>(B + o_min); A.index = reinterpret_cast<int *>(B + o_index);
    A.p2d = reinterpret_cast<float *>(B + o_p2d); A.p3dw = reinterpret_cast<float *>(B + o_p3d); A.max_err = reinterpret_cast<float *>(B + o_err);
    A.count = reinterpret_cast<int *>(B + o_count); A.degenerate = B + o_deg;
    A.pose = reinterpret_cast<float *>(B + o_pose); A.inliers = reinterpret_cast<uint32_t *>(B + o_inl);
    A.refined = B + o_ref; A.refined_count = reinterpret_cast<int *>(B + o_rcount);
    A.refined_pose = reinterpret_cast<float *>(B + o_rpose); A.refined_inliers = reinterpret_cast<uint32_t *>(B + o_rinl);
    afv_launch_pnp(&A, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, b.fetch(n, o_n, (size_t)nc * 4, c->stream));
    HIPCHK(c, b.fetch(min_inliers, o_min, (size_t)nc * 4, c->stream));
    HIPCHK(c, b.fetch(index, o_index, cells * 4, c->stream));
    HIPCHK(c, b.fetch(count, o_count, hyps * 4, c->stream));
    HIPCHK(c, b.fetch(degenerate, o_deg, hyps, c->stream));
    HIPCHK(c, b.fetch(pose, o_pose, hyps * 48, c->stream));
    HIPCHK(c, b.fetch(inliers, o_inl, hyps * (size_t)mask_words * 4, c->stream));
    HIPCHK(c, b.fetch(refined, o_ref, hyps, c->stream));
    HIPCHK(c, b.fetch(refined_count, o_rcount, hyps * 4, c->stream));
    HIPCHK(c, b.fetch(refined_pose, o_rpose, hyps * 48, c->stream));
    HIPCHK(c, b.fetch(refined_inliers, o_rinl, hyps * (size_t)mask_words * 4, c->stream));
    if (max_err) HIPCHK(c, b.fetch(max_err, o_err, cells * 4, c->stream));
    if (p3dw) HIPCHK(c, b.fetch(p3dw, o_p3d, cells * 12, c->stream));
    HIPCHK(c, b.wait());  // the call's one wait
    return AFV_OK;
}

extern "C" int afv_frame_pnp_hypotheses(afv_frame *f, afv_points *points, const afv_pnp_job *jobs, int nc, const int32_t *pts, int nhyp,
                                        int mask_words, int32_t *n, int32_t *min_inliers, int32_t *index, int32_t *count, uint8_t *degenerate,
                                        float *pose, uint32_t *inliers, uint8_t *refined, int32_t *refined_count, float *refined_pose,
                                        uint32_t *refined_inliers, float *max_err, float *p3dw) {
    if (!f || !points || !jobs || !pts || !n || !min_inliers || !index || !count || !degenerate || !pose || !inliers || !refined || !refined_count ||
        !refined_pose || !refined_inliers)
        return AFV_EINVAL;
    if (nc < 1 || nc > AFV_PNP_MAX_CANDIDATES || nhyp < 1 || nhyp > AFV_PNP_MAX_HYPOTHESES || mask_words < 0 || mask_words > AFV_PNP_MAX_MASK_WORDS)
        return AFV_EINVAL;
    if (!afv_frame_is_live(f) || !afv_points_is_live(points) || points->c != f->c) return AFV_EINVAL;
    if (!f->has_features || !f->has_grid || f->n < 1 || !f->has_pose) return AFV_EINVAL;
    return guarded(f->c, [&] {
        return pnp_impl(f, points, jobs, nc, pts, nhyp, mask_words, n, min_inliers, index, count, degenerate, pose, inliers, refined, refined_count,
                        refined_pose, refined_inliers, max_err, p3dw);
    });
}
