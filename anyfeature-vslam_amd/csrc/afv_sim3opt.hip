// afv_sim3opt.hip — host side of afv_table_optimize_sim3 (include/afv_hip.h, "OptimizeSim3"; kernels: k_sim3opt.hip).
//
// Reference call shape: LoopClosing::ComputeSim3 (src/LoopClosing.cc:279-371) calls Optimizer::OptimizeSim3 once per candidate whose
// Sim3Solver found a transform, on the host, through g2o.  Here the rows of up to 64 candidates go up in one copy, two launches run on
// the context's stream and the host waits once: k_sim3opt_gather builds every job's edge set, k_sim3opt_solve runs every job's two
// optimize() calls and classifications, one wavefront per job.
#include "afv_runtime.h"

static int sim3opt_impl(afv_table *t, afv_points *points, const int32_t *slot_a, const int32_t *slot_b, const afv_sim3opt_job *caller_jobs, int nc,
                        const int32_t *mp1, const int32_t *mp2, const int32_t *idx2, afv_sim3opt_result *results, uint8_t *state) {
    afv_ctx *c = t->c;
    std::vector<afv_sim3opt_job> jobs;
    if (!afv_load_jobs(caller_jobs, nc, sizeof(afv_sim3opt_job), jobs)) return AFV_EINVAL;
    const int cap = t->cap;
    for (int k = 0; k < nc; ++k) {
        const int a = slot_a[k], b = slot_b[k];
        if (a < 0 || a >= t->nsets || b < 0 || b >= t->nsets) return AFV_EINVAL;
        if (jobs[(size_t)k].fix_scale != 0 && jobs[(size_t)k].fix_scale != 1) return AFV_EINVAL;
        for (int s : {a, b}) {
            if (t->h_n[s] > 0 && !t->has_geo[s]) {
                c->last_error = "afv_table_optimize_sim3: set " + std::to_string(s) + " lacks its geometry (afv_table_set_geometry)";
                return AFV_EINVAL;
            }
            if (t->h_n[s] > 0 && !t->has_inf[s]) {
                c->last_error = "afv_table_optimize_sim3: set " + std::to_string(s) + " lacks its information plane (afv_table_set_inf)";
                return AFV_EINVAL;
            }
        }
        const int n1 = t->h_n[a], n2 = t->h_n[b];
        const size_t row0 = (size_t)k * cap;
        for (int i = 0; i < n1; ++i) {
            const int p1 = mp1[row0 + i], p2 = mp2[row0 + i], k2 = idx2[row0 + i];
            if (p1 < -1 || p1 >= points->cap || p2 < -1 || p2 >= points->cap) {
                c->last_error = "afv_table_optimize_sim3: job " + std::to_string(k) + " names a map-point id outside the store";
                return AFV_EINVAL;
            }
            if (k2 < -1 || k2 >= n2) {
                c->last_error = "afv_table_optimize_sim3: job " + std::to_string(k) + " names a feature that does not exist";
                return AFV_EINVAL;
            }
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)nc * cap, plane = (size_t)t->nsets * cap;
    const bool planes = t->d_geo && t->d_inf;  // without them every slot is empty (checked above)
    std::vector<DevSim3OptJob> dj((size_t)nc);
    for (int k = 0; k < nc; ++k) {
        const afv_sim3opt_job &j = jobs[(size_t)k];
        DevSim3OptJob &D = dj[(size_t)k];
        D = DevSim3OptJob{};
        std::memcpy(D.R1, j.Rcw1, sizeof(D.R1)); std::memcpy(D.t1, j.tcw1, sizeof(D.t1));
        std::memcpy(D.R2, j.Rcw2, sizeof(D.R2)); std::memcpy(D.t2, j.tcw2, sizeof(D.t2));
        D.fx1 = j.fx1; D.fy1 = j.fy1; D.cx1 = j.cx1; D.cy1 = j.cy1; D.fx2 = j.fx2; D.fy2 = j.fy2; D.cx2 = j.cx2; D.cy2 = j.cy2;
        std::memcpy(D.R12, j.R12, sizeof(D.R12)); std::memcpy(D.t12, j.t12, sizeof(D.t12));
        D.s12 = j.s12; D.th2 = j.th2;
        D.fix_scale = j.fix_scale;
        D.n1 = planes ? t->h_n[slot_a[k]] : 0;
        if (planes) {
            const size_t ra = (size_t)slot_a[k] * cap, rb = (size_t)slot_b[k] * cap;
            D.x1 = t->d_geo + ra; D.y1 = t->d_geo + plane + ra; D.inf1 = t->d_inf + ra;
            D.x2 = t->d_geo + rb; D.y2 = t->d_geo + plane + rb; D.inf2 = t->d_inf + rb;
        }
    }
    Blob b(c);
    const size_t o_jobs = b.put(dj.data(), dj.size() * sizeof(DevSim3OptJob));
    const size_t o_mp1 = b.put(mp1, cells * 4), o_mp2 = b.put(mp2, cells * 4), o_idx2 = b.put(idx2, cells * 4);
    const size_t in_bytes = b.h.size();
    const size_t o_n = b.reserve_scratch((size_t)nc * 4), o_index1 = b.reserve_scratch(cells * 4);
    const size_t o_edges = b.reserve_scratch(cells * sizeof(DevSim3OptEdge)), o_active = b.reserve_scratch(cells);
    const size_t o_res = b.reserve_scratch((size_t)nc * sizeof(afv_sim3opt_result)), o_state = b.reserve_scratch(cells);
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    uint8_t *B = c->d_match;
    HIPCHK(c, b.upload(in_bytes));
    DevSim3OptArgs A{};
    A.jobs = reinterpret_cast<const DevSim3OptJob *>(B + o_jobs);
    A.mp1 = reinterpret_cast<const int *>(B + o_mp1); A.mp2 = reinterpret_cast<const int *>(B + o_mp2);
    A.idx2 = reinterpret_cast<const int *>(B + o_idx2);
    A.nc = nc; A.cap = cap;
    for (int k = 0; k < 3; ++k) A.pos[k] = points->P.pos[k];
    A.flags = points->P.flags;
    A.pcap = points->cap;
    A.n = reinterpret_cast<int *>(B + o_n); A.index1 = reinterpret_cast<int *>(B + o_index1);
    A.edges = reinterpret_cast<DevSim3OptEdge *>(B + o_edges); A.active = B + o_active;
    A.results = reinterpret_cast<afv_sim3opt_result *>(B + o_res); A.state = B + o_state;
    afv_launch_sim3opt_gather(&A, c->stream);
    afv_launch_sim3opt_solve(&A, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, b.fetch(results, o_res, (size_t)nc * sizeof(afv_sim3opt_result), c->stream));
    HIPCHK(c, b.fetch(state, o_state, cells, c->stream));
    HIPCHK(c, b.wait());  // the call's one wait
    return AFV_OK;
}

extern "C" int afv_table_optimize_sim3(afv_table *t, afv_points *points, const int32_t *slot_a, const int32_t *slot_b, const afv_sim3opt_job *jobs,
                                       int nc, const int32_t *mp1, const int32_t *mp2, const int32_t *idx2, afv_sim3opt_result *results,
                                       uint8_t *state) {
    if (!t || !points || !slot_a || !slot_b || !jobs || !mp1 || !mp2 || !idx2 || !results || !state) return AFV_EINVAL;
    if (nc < 1 || nc > AFV_SIM3_MAX_CANDIDATES) return AFV_EINVAL;
    if (!afv_points_is_live(points) || points->c != t->c) return AFV_EINVAL;
    return guarded(t->c, [&] { return sim3opt_impl(t, points, slot_a, slot_b, jobs, nc, mp1, mp2, idx2, results, state); });
}
