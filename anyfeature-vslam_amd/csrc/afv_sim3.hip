// afv_sim3.hip — host side of afv_table_sim3_hypotheses (include/afv_hip.h, "Sim3Solver"; kernels: k_sim3.hip).
//
// Reference call shape: LoopClosing::ComputeSim3 (src/LoopClosing.cc:247-416) builds one Sim3Solver per candidate keyframe on the host and
// iterates them round-robin, five RANSAC hypotheses at a time.  Here the rows of up to 64 candidates go up in one copy, two launches run
// on the context's stream and the host waits once: k_sim3_gather is every solver's constructor, k_sim3_hypotheses evaluates every
// hypothesis of every candidate.  The scan of Sim3Solver::iterate over the counts is the caller's (the adapters).
#include "afv_runtime.h"

static int sim3_impl(afv_table *t, afv_points *points, const int32_t *slot_a, const int32_t *slot_b, const afv_sim3_job *caller_jobs, int nc,
                     const int32_t *mp1, const int32_t *mp2, const int32_t *idx1, const int32_t *idx2, int nhyp, int mask_words, int32_t *n,
                     int32_t *index1, int32_t *count, uint8_t *degenerate, float *sim3, uint32_t *inliers, float *x3dc1, float *x3dc2,
                     float *max_err) {
    afv_ctx *c = t->c;
    std::vector<afv_sim3_job> jobs;
    if (!afv_load_jobs(caller_jobs, nc, sizeof(afv_sim3_job), jobs)) return AFV_EINVAL;
    const int cap = t->cap;
    long long most = 0;
    for (int k = 0; k < nc; ++k) {
        const int a = slot_a[k], b = slot_b[k];
        if (a < 0 || a >= t->nsets || b < 0 || b >= t->nsets) return AFV_EINVAL;
        if (jobs[(size_t)k].fix_scale != 0 && jobs[(size_t)k].fix_scale != 1) return AFV_EINVAL;
        for (int s : {a, b})
            if (t->h_n[s] > 0 && !t->has_geo[s]) {
                c->last_error = "afv_table_sim3_hypotheses: set " + std::to_string(s) + " lacks its geometry (afv_table_set_geometry)";
                return AFV_EINVAL;
            }
        const int n1 = t->h_n[a], n2 = t->h_n[b];
        const size_t row0 = (size_t)k * cap;
        long long countable = 0;
        for (int i = 0; i < n1; ++i) {
            const int p1 = mp1[row0 + i], p2 = mp2[row0 + i], k1 = idx1 ? idx1[row0 + i] : i, k2 = idx2[row0 + i];
            if (p1 < -1 || p1 >= points->cap || p2 < -1 || p2 >= points->cap) {
                c->last_error = "afv_table_sim3_hypotheses: candidate " + std::to_string(k) + " names a map-point id outside the store";
                return AFV_EINVAL;
            }
            if (k1 < -1 || k1 >= n1 || k2 < -1 || k2 >= n2) {
                c->last_error = "afv_table_sim3_hypotheses: candidate " + std::to_string(k) + " names a feature that does not exist";
                return AFV_EINVAL;
            }
            countable += p1 >= 0 && p2 >= 0 && k1 >= 0 && k2 >= 0;
        }
        most = std::max(most, countable);
    }
    if ((long long)mask_words * 32 < most) {
        c->last_error = "afv_table_sim3_hypotheses: mask_words " + std::to_string(mask_words) + " cannot hold " + std::to_string(most) + " correspondences";
        return AFV_EINVAL;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)nc * cap, hyps = (size_t)nc * nhyp, plane = (size_t)t->nsets * cap;
    std::vector<DevSim3Cand> dc((size_t)nc);
    for (int k = 0; k < nc; ++k) {
        const afv_sim3_job &j = jobs[(size_t)k];
        DevSim3Cand &D = dc[(size_t)k];
        D = DevSim3Cand{};
        std::memcpy(D.R1, j.Rcw1, sizeof(D.R1)); std::memcpy(D.t1, j.tcw1, sizeof(D.t1));
        std::memcpy(D.R2, j.Rcw2, sizeof(D.R2)); std::memcpy(D.t2, j.tcw2, sizeof(D.t2));
        D.fx1 = j.fx1; D.fy1 = j.fy1; D.cx1 = j.cx1; D.cy1 = j.cy1; D.fx2 = j.fx2; D.fy2 = j.fy2; D.cx2 = j.cx2; D.cy2 = j.cy2;
        D.seed = ((unsigned long long)j.seed_hi << 32) | j.seed_lo;
        D.fix_scale = j.fix_scale;
        D.n1 = t->d_geo ? t->h_n[slot_a[k]] : 0;  // no geometry plane at all: every slot is empty
        if (t->d_geo) {
            D.sigma2_1 = t->d_geo + 2 * plane + (size_t)slot_a[k] * cap;
            D.sigma2_2 = t->d_geo + 2 * plane + (size_t)slot_b[k] * cap;
        }
    }
    Blob b(c);
    const size_t o_cands = b.put(dc.data(), dc.size() * sizeof(DevSim3Cand));
    const size_t o_mp1 = b.put(mp1, cells * 4), o_mp2 = b.put(mp2, cells * 4), o_idx2 = b.put(idx2, cells * 4);
    const size_t o_idx1 = idx1 ? b.put(idx1, cells * 4) : 0;
    const size_t in_bytes = b.h.size();
    const size_t o_n = b.reserve_scratch((size_t)nc * 4), o_index1 = b.reserve_scratch(cells * 4);
    const size_t o_x1 = b.reserve_scratch(cells * 12), o_x2 = b.reserve_scratch(cells * 12);
    const size_t o_im1 = b.reserve_scratch(cells * 8), o_im2 = b.reserve_scratch(cells * 8), o_err = b.reserve_scratch(cells * 8);
    const size_t o_count = b.reserve_scratch(hyps * 4), o_deg = b.reserve_scratch(hyps), o_sim3 = b.reserve_scratch(hyps * 13 * 4);
    const size_t o_inl = b.reserve_scratch(std::max<size_t>(hyps * (size_t)mask_words * 4, 4));
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    uint8_t *B = c->d_match;
    HIPCHK(c, b.upload(in_bytes));
    DevSim3Args A{};
    A.cands = reinterpret_cast<const DevSim3Cand *>(B + o_cands);
    A.mp1 = reinterpret_cast<const int *>(B + o_mp1); A.mp2 = reinterpret_cast<const int *>(B + o_mp2);
    A.idx1 = idx1 ? reinterpret_cast<const int *>(B + o_idx1) : nullptr; A.idx2 = reinterpret_cast<const int *>(B + o_idx2);
    A.nc = nc; A.cap = cap; A.nhyp = nhyp; A.mask_words = mask_words;
    for (int k = 0; k < 3; ++k) A.pos[k] = points->P.pos[k];
    A.flags = points->P.flags;
    A.pcap = points->cap;
    A.n = reinterpret_cast<int *>(B + o_n); A.index1 = reinterpret_cast<int *>(B + o_index1);
    A.x1 = reinterpret_cast<float *>(B + o_x1); A.x2 = reinterpret_cast<float *>(B + o_x2);
    A.im1 = reinterpret_cast<float *>(B + o_im1); A.im2 = reinterpret_cast<float *>(B + o_im2);
    A.max_err = reinterpret_cast<float *>(B + o_err);
    A.count = reinterpret_cast<int *>(B + o_count); A.degenerate = B + o_deg;
    A.sim3 = reinterpret_cast<float *>(B + o_sim3); A.inliers = reinterpret_cast<uint32_t *>(B + o_inl);
    afv_launch_sim3_gather(&A, c->stream);
    afv_launch_sim3_hypotheses(&A, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, b.fetch(n, o_n, (size_t)nc * 4, c->stream));
    HIPCHK(c, b.fetch(index1, o_index1, cells * 4, c->stream));
    HIPCHK(c, b.fetch(count, o_count, hyps * 4, c->stream));
    HIPCHK(c, b.fetch(degenerate, o_deg, hyps, c->stream));
    HIPCHK(c, b.fetch(sim3, o_sim3, hyps * 13 * 4, c->stream));
    HIPCHK(c, b.fetch(inliers, o_inl, hyps * (size_t)mask_words * 4, c->stream));
    if (x3dc1) HIPCHK(c, b.fetch(x3dc1, o_x1, cells * 12, c->stream));
    if (x3dc2) HIPCHK(c, b.fetch(x3dc2, o_x2, cells * 12, c->stream));
    if (max_err) HIPCHK(c, b.fetch(max_err, o_err, cells * 8, c->stream));
    HIPCHK(c, b.wait());  // the call's one wait
    return AFV_OK;
}

extern "C" int afv_table_sim3_hypotheses(afv_table *t, afv_points *points, const int32_t *slot_a, const int32_t *slot_b, const afv_sim3_job *jobs,
                                         int nc, const int32_t *mp1, const int32_t *mp2, const int32_t *idx1, const int32_t *idx2, int nhyp,
                                         int mask_words, int32_t *n, int32_t *index1, int32_t *count, uint8_t *degenerate, float *sim3,
                                         uint32_t *inliers, float *x3dc1, float *x3dc2, float *max_err) {
    if (!t || !points || !slot_a || !slot_b || !jobs || !mp1 || !mp2 || !idx2 || !n || !index1 || !count || !degenerate || !sim3 || !inliers)
        return AFV_EINVAL;
    if (nc < 1 || nc > AFV_SIM3_MAX_CANDIDATES || nhyp < 1 || nhyp > AFV_SIM3_MAX_HYPOTHESES || mask_words < 0 || mask_words > AFV_SIM3_MAX_MASK_WORDS)
        return AFV_EINVAL;
    if (!afv_points_is_live(points) || points->c != t->c) return AFV_EINVAL;
    return guarded(t->c, [&] {
        return sim3_impl(t, points, slot_a, slot_b, jobs, nc, mp1, mp2, idx1, idx2, nhyp, mask_words, n, index1, count, degenerate, sim3, inliers,
                         x3dc1, x3dc2, max_err);
    });
}
