// afv_lba.hip — host side of afv_table_bundle_adjust (include/afv_hip.h, "Bundle adjustment"; kernels: k_lba.hip).
//
// Reference call shape: LocalMapping::Run calls Optimizer::LocalBundleAdjustment after every keyframe (src/LocalMapping.cc:84), on the
// host, through g2o; Tracking::CreateInitialMapMonocular and loop closing call Optimizer::BundleAdjustment.  Here the edge lists go up in
// one copy, a gather reads everything else from the table and the store, and the host drives the Levenberg loop: per trial it enqueues
// the trial's launches, waits once, reads the status record and the stop flag - where g2o's terminate() stands - and follows what the
// device decided.  The by-keyframe order of the edges depends on obs_kf alone, so it is built here during the argument check.
//
// afv_table_global_bundle_adjust (LoopClosing::RunGlobalBundleAdjustment's call, and any problem beyond AFV_LBA_MAX_FREE) is the same
// driver with another solve: the host also derives the block-sparse plan of the reduced system from the edge list (afv_gba_plan.h), the
// plan goes up in the same copy, and per trial k_gba_schur / k_gba_factor (k_gba.hip) stand where k_lba_schur / k_lba_solve stood.  The
// dense n x n matrix is not allocated on that route.  afv_points_correct_se3 is the float point correction that follows a global BA.
#include "afv_runtime.h"
#include "afv_lba_math.h"
#include "afv_gba_math.h"
#include "afv_gba_plan.h"

static_assert(sizeof(afv_lba_cam) == 72 && sizeof(afv_lba_params) == 32 && sizeof(afv_lba_result) == 64, "afv_lba records");

namespace {

struct LbaCall {
    afv_table *t;
    afv_points *points;
    const int32_t *slots, *point_ids, *obs_point, *obs_kf, *obs_idx;
    int nk, nf, np, ne;
    std::vector<afv_lba_cam> cams;
    afv_lba_params prm;
    const volatile int32_t *stop_flag;
    int total_trials = 0;
    bool sparse = false;  // afv_table_global_bundle_adjust: the block-sparse solve (k_gba.hip), no dense n x n matrix
    long long max_blocks = AFV_GBA_MAX_L_BLOCKS;
    const char *fn = "afv_table_bundle_adjust";
    bool flag() const { return (stop_flag && *stop_flag != 0) || (prm.trial_budget > 0 && total_trials >= prm.trial_budget); }
};

int lba_refuse(afv_ctx *c, const char *why, const char *fn = "afv_table_bundle_adjust", int rc = AFV_EINVAL) {
    c->last_error = std::string(fn) + ": " + why;
    return rc;
}

// everything that is malformed is refused here, before any launch; builds pt_ptr [np + 1] and the by-keyframe order (kf_ptr [nf + 1], kf_edge)
int lba_check(const LbaCall &K, std::vector<int> &pt_ptr, std::vector<int> &kf_ptr, std::vector<int> &kf_edge) {
    const afv_table *t = K.t;
    afv_ctx *c = t->c;
    for (int k = 0; k < K.nk; ++k) {
        const int s = K.slots[k];
        if (s < 0 || s >= t->nsets) return lba_refuse(c, "a slot is out of range", K.fn);
        if (t->h_n[s] > 0 && !t->has_geo[s]) return lba_refuse(c, "a slot lacks its geometry (afv_table_set_geometry)", K.fn);
        if (t->h_n[s] > 0 && !t->has_inf[s]) return lba_refuse(c, "a slot lacks its information plane (afv_table_set_inf)", K.fn);
    }
    {
        std::vector<uint8_t> seen((size_t)K.points->cap, 0);
        for (int p = 0; p < K.np; ++p) {
            const int id = K.point_ids[p];
            if (id < 0 || id >= K.points->cap) return lba_refuse(c, "a map-point id lies outside the store", K.fn);
            if (seen[(size_t)id]) return lba_refuse(c, "a map-point id is named twice", K.fn);
            seen[(size_t)id] = 1;
        }
    }
    pt_ptr.assign((size_t)K.np + 1, 0);
    kf_ptr.assign((size_t)K.nf + 1, 0);
    std::vector<int> last((size_t)K.nk, -1);  // the last point that keyframe k observed: edges come by point, so a repeat is a duplicate
    for (int e = 0; e < K.ne; ++e) {
        const int p = K.obs_point[e], k = K.obs_kf[e];
        if (p < 0 || p >= K.np) return lba_refuse(c, "obs_point is out of range", K.fn);
        if (e > 0 && p < K.obs_point[e - 1]) return lba_refuse(c, "the edges are not grouped by point", K.fn);
        if (k < 0 || k >= K.nk) return lba_refuse(c, "obs_kf is out of range", K.fn);
        if (K.obs_idx[e] < 0 || K.obs_idx[e] >= t->h_n[K.slots[k]]) return lba_refuse(c, "obs_idx names a feature that does not exist", K.fn);
        if (last[(size_t)k] == p) return lba_refuse(c, "a point is observed twice by one keyframe", K.fn);
        last[(size_t)k] = p;
        pt_ptr[(size_t)p + 1] = e + 1;
        if (k < K.nf) ++kf_ptr[(size_t)k + 1];
    }
    for (int p = 0; p < K.np; ++p)
        if (pt_ptr[(size_t)p + 1] < pt_ptr[(size_t)p]) pt_ptr[(size_t)p + 1] = pt_ptr[(size_t)p];  // a point without edges
    for (int i = 0; i < K.nf; ++i) kf_ptr[(size_t)i + 1] += kf_ptr[(size_t)i];
    kf_edge.assign((size_t)kf_ptr[(size_t)K.nf] + 1, 0);
    std::vector<int> at(kf_ptr.begin(), kf_ptr.end());
    for (int e = 0; e < K.ne; ++e)
        if (K.obs_kf[e] < K.nf) kf_edge[(size_t)at[(size_t)K.obs_kf[e]]++] = e;
    return AFV_OK;
}

int lba_impl(LbaCall &K, afv_lba_result *results, double *kf_out, double *xyz_out, uint8_t *edge_state) {
    afv_table *t = K.t;
    afv_ctx *c = t->c;
    std::vector<int> pt_ptr, kf_ptr, kf_edge;
    const int rc0 = lba_check(K, pt_ptr, kf_ptr, kf_edge);
    if (rc0) return rc0;
    GbPlan plan;  // L7': derived from the edge list as given, before anything is dropped or removed
    if (K.sparse && gb_plan(K.nf, K.np, pt_ptr.data(), K.obs_kf, K.max_blocks, plan) == GB_PLAN_BLOCKS)
        return lba_refuse(c, "the fill of the keyframe order exceeds AFV_GBA_MAX_L_BLOCKS", K.fn, AFV_ECAPACITY);
    afv_lba_result R{};
    if (K.prm.checks && K.flag()) {  // :645-647
        R.stopped = 1;
        *results = R;
        return AFV_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int nk = K.nk, nf = K.nf, np = K.np, ne = K.ne;
    const size_t E = (size_t)std::max(ne, 1), P = (size_t)std::max(np, 1), KF = (size_t)std::max(nk, 1), n = 6 * (size_t)nf;
    std::vector<float> cams(17 * KF, 0.0f);
    for (int k = 0; k < nk; ++k) {
        const afv_lba_cam &a = K.cams[(size_t)k];
        float *o = cams.data() + 17 * (size_t)k;
        std::memcpy(o, a.Rcw, 9 * sizeof(float));
        std::memcpy(o + 9, a.tcw, 3 * sizeof(float));
        o[12] = a.fx; o[13] = a.fy; o[14] = a.cx; o[15] = a.cy; o[16] = a.bf;
    }
    // the image: inputs first (one upload), then what the host reads back, then device-only scratch beyond the image
    Blob b(c);
    const size_t o_cams = b.put(cams.data(), cams.size() * sizeof(float));
    const size_t o_slots = b.put(K.slots, KF * 4 * (nk > 0)), o_ids = b.put(K.point_ids, P * 4 * (np > 0));
    const size_t o_ept = b.put(K.obs_point, E * 4 * (ne > 0)), o_ekf = b.put(K.obs_kf, E * 4 * (ne > 0)), o_eidx = b.put(K.obs_idx, E * 4 * (ne > 0));
    const size_t o_ptp = b.put(pt_ptr.data(), pt_ptr.size() * 4), o_kfp = b.put(kf_ptr.data(), kf_ptr.size() * 4);
    const size_t o_kfe = b.put(kf_edge.data(), kf_edge.size() * 4);
    size_t o_colp = 0, o_brow = 0, o_bcol = 0, o_bkind = 0;
    if (K.sparse) {
        o_colp = b.put(plan.col_ptr.data(), plan.col_ptr.size() * 4); o_brow = b.put(plan.blk_row.data(), plan.blk_row.size() * 4);
        o_bcol = b.put(plan.blk_col.data(), plan.blk_col.size() * 4); o_bkind = b.put(plan.blk_kind.data(), plan.blk_kind.size());
    }
    const size_t o_status = b.reserve(sizeof(LbStatus));  // zero: buffer 0 holds the estimate
    const size_t in_bytes = b.h.size();
    const size_t o_state = b.reserve_scratch(E), o_kfout = b.reserve_scratch(std::max<size_t>(nf, 1) * 12 * 8), o_xyzout = b.reserve_scratch(P * 3 * 8);
    size_t cur = align_up(b.h.size(), 256);
    auto take = [&](size_t bytes) {
        const size_t o = cur;
        cur = align_up(cur + std::max<size_t>(bytes, 8), 256);
        return o;
    };
    const size_t o_cam = take(KF * sizeof(LbCam)), o_obs = take(5 * E * 8), o_stereo = take(E), o_eon = take(E), o_echi = take(E * 8);
    const size_t o_pon = take(P), o_pose = take(2 * KF * 12 * 8), o_xyz = take(2 * P * 3 * 8), o_term = take((size_t)LB_NT * E * 8), o_rho = take(E * 8);
    const size_t o_hll = take(P * 9 * 8), o_hinv = take(P * 9 * 8), o_hpp = take(std::max<size_t>(nf, 1) * 27 * 8);
    const size_t o_m = take(K.sparse ? ((size_t)plan.nb + 1) * 36 * 8 : n * n * 8);  // the dense M, or the blocks of L
    const size_t o_bs = take(n * 8), o_dx = take((n + 3 * P) * 8), o_pfail = take(P), o_kfail = take(KF), o_sfail = take(4);
    const int rc = ensure_match_buffer(c, cur);
    if (rc) return rc;
    uint8_t *B = c->d_match;
    HIPCHK(c, b.upload(in_bytes));
    LbView V{};
    V.nk = nk; V.nf = nf; V.np = np; V.ne = ne;
    V.cam = reinterpret_cast<const LbCam *>(B + o_cam);
    V.e_pt = reinterpret_cast<const int *>(B + o_ept); V.e_kf = reinterpret_cast<const int *>(B + o_ekf);
    V.e_obs = reinterpret_cast<const double *>(B + o_obs); V.e_stereo = B + o_stereo; V.e_on = B + o_eon; V.e_state = B + o_state;
    V.e_chi2 = reinterpret_cast<double *>(B + o_echi);
    V.pt_ptr = reinterpret_cast<const int *>(B + o_ptp); V.kf_ptr = reinterpret_cast<const int *>(B + o_kfp);
    V.kf_edge = reinterpret_cast<const int *>(B + o_kfe);
    V.p_on = B + o_pon; V.pose = reinterpret_cast<double *>(B + o_pose); V.xyz = reinterpret_cast<double *>(B + o_xyz);
    V.term = reinterpret_cast<double *>(B + o_term); V.rho_trial = reinterpret_cast<double *>(B + o_rho);
    V.Hll = reinterpret_cast<double *>(B + o_hll); V.Hinv = reinterpret_cast<double *>(B + o_hinv); V.Hpp = reinterpret_cast<double *>(B + o_hpp);
    V.M = K.sparse ? nullptr : reinterpret_cast<double *>(B + o_m); V.bS = reinterpret_cast<double *>(B + o_bs); V.dx = reinterpret_cast<double *>(B + o_dx);
    V.p_fail = B + o_pfail; V.k_fail = B + o_kfail; V.solve_fail = reinterpret_cast<int32_t *>(B + o_sfail);
    V.st = reinterpret_cast<LbStatus *>(B + o_status);
    GbView S{};
    if (K.sparse) {
        S.nf = nf; S.nb = plan.nb;
        S.col_ptr = reinterpret_cast<const int *>(B + o_colp); S.blk_row = reinterpret_cast<const int *>(B + o_brow);
        S.blk_col = reinterpret_cast<const int *>(B + o_bcol); S.blk_kind = B + o_bkind; S.L = reinterpret_cast<double *>(B + o_m);
    }
    DevLbaGather G{};
    G.geo = t->d_geo; G.inf = t->d_inf; G.plane = (size_t)t->nsets * t->cap; G.cap = t->cap;
    G.slots = reinterpret_cast<const int *>(B + o_slots); G.obs_idx = reinterpret_cast<const int *>(B + o_eidx);
    G.point_ids = reinterpret_cast<const int *>(B + o_ids); G.cams = reinterpret_cast<const float *>(B + o_cams);
    for (int k = 0; k < 3; ++k) G.pos[k] = K.points->P.pos[k];
    G.flags = K.points->P.flags;
    G.obs = reinterpret_cast<double *>(B + o_obs); G.stereo = B + o_stereo; G.p_on = B + o_pon; G.cam = reinterpret_cast<LbCam *>(B + o_cam);
    HIPCHK(c, hipMemsetAsync(B + o_sfail, 0, 4, c->stream));
    afv_launch_lba_gather(&V, &G, c->stream);
    HIPCHK(c, hipGetLastError());

    uint8_t *h_state = b.h.data() + o_state;
    const LbStatus *h_status = reinterpret_cast<const LbStatus *>(b.h.data() + o_status);
    // the edge states after the gather / the first check: the host counts the active edges (L8) where it waits anyway
    auto count_state = [&](int which, int *n_out) -> int {
        int cnt = 0;
        if (ne > 0) {
            HIPCHK(c, hipMemcpyAsync(h_state, B + o_state, (size_t)ne, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (int e = 0; e < ne; ++e) cnt += h_state[e] == which;
        }
        *n_out = cnt;
        return AFV_OK;
    };
    // SparseOptimizer::optimize(iterations): the flag is read before every iteration and after every trial
    auto optimize = [&](int r, int active) -> int {
        if (active == 0 || nf == 0 || K.prm.iterations[r] <= 0 || K.flag()) return AFV_OK;  // L8
        afv_launch_lba_round(&V, K.prm.iterations[r], K.prm.robust[r], c->stream);
        int next = LB_NEXT_ITERATION;
        while (next != LB_NEXT_DONE) {
            if (next == LB_NEXT_ITERATION) afv_launch_lba_iteration(&V, c->stream);
            if (K.sparse) {
                afv_launch_lba_trial_head(&V, c->stream);
                afv_launch_gba_solve(&V, &S, c->stream);
                afv_launch_lba_trial_tail(&V, c->stream);
            } else {
                afv_launch_lba_trial(&V, c->stream);
            }
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(b.h.data() + o_status, B + o_status, sizeof(LbStatus), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // the trial's one wait
            next = h_status->next;
            ++K.total_trials;
            if (K.flag()) next = LB_NEXT_DONE;
        }
        R.iterations[r] = h_status->iterations; R.trials[r] = h_status->trials; R.chi2[r] = h_status->cur; R.lambda[r] = h_status->lam;
        return AFV_OK;
    };
    int active = 0, rcx;
    if ((rcx = count_state(LB_KEPT, &active))) return rcx;
    R.n_edges = active;
    if ((rcx = optimize(0, active))) return rcx;
    const bool stopped = K.flag();
    if (stopped) R.stopped = 2;
    if (K.prm.checks) {
        if (!stopped) {
            afv_launch_lba_check(&V, 0, c->stream);
            int kept = 0;
            if ((rcx = count_state(LB_KEPT, &kept))) return rcx;
            R.n_removed_first = active - kept;
            if ((rcx = optimize(1, kept))) return rcx;
            if (K.flag()) R.stopped = 3;
        }
        afv_launch_lba_check(&V, 1, c->stream);
    }
    DevLbaFinish F{};
    F.kf_out = reinterpret_cast<double *>(B + o_kfout); F.xyz_out = reinterpret_cast<double *>(B + o_xyzout);
    for (int k = 0; k < 3; ++k) F.pos[k] = K.points->P.pos[k];
    F.point_ids = G.point_ids;
    F.write_points = K.prm.write_points;
    afv_launch_lba_finish(&V, &F, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, b.fetch(kf_out, o_kfout, (size_t)nf * 12 * 8, c->stream));
    HIPCHK(c, b.fetch(xyz_out, o_xyzout, (size_t)np * 3 * 8, c->stream));
    HIPCHK(c, b.fetch(edge_state, o_state, (size_t)ne, c->stream));
    HIPCHK(c, b.wait());
    for (int e = 0; e < ne; ++e) R.n_erase += edge_state[e] == LB_ERASE;
    *results = R;
    return AFV_OK;
}

int lba_entry(bool sparse, afv_table *t, afv_points *points, const int32_t *slots, int nk, int n_free, const afv_lba_cam *cams, const int32_t *point_ids,
              int np, const int32_t *obs_point, const int32_t *obs_kf, const int32_t *obs_idx, int ne, const afv_lba_params *params,
              const volatile int32_t *stop_flag, afv_lba_result *results, double *kf_out, double *xyz_out, uint8_t *edge_state) {
    if (!t || !points || !slots || !cams || !point_ids || !obs_point || !obs_kf || !obs_idx || !params || !results || !kf_out || !xyz_out || !edge_state)
        return AFV_EINVAL;
    const int max_kf = sparse ? AFV_GBA_MAX_KF : AFV_LBA_MAX_KF, max_free = sparse ? AFV_GBA_MAX_KF : AFV_LBA_MAX_FREE;
    const int max_np = sparse ? AFV_GBA_MAX_POINTS : AFV_LBA_MAX_POINTS, max_ne = sparse ? AFV_GBA_MAX_EDGES : AFV_LBA_MAX_EDGES;
    if (nk < 0 || nk > max_kf || n_free < 0 || n_free > nk || n_free > max_free || np < 0 || np > max_np || ne < 0 || ne > max_ne) return AFV_EINVAL;
    if (!afv_points_is_live(points) || points->c != t->c) return AFV_EINVAL;
    return guarded(t->c, [&] {
        LbaCall K{};
        K.t = t; K.points = points; K.slots = slots; K.point_ids = point_ids; K.obs_point = obs_point; K.obs_kf = obs_kf; K.obs_idx = obs_idx;
        K.nk = nk; K.nf = n_free; K.np = np; K.ne = ne; K.stop_flag = stop_flag;
        K.sparse = sparse;
        if (sparse) K.fn = "afv_table_global_bundle_adjust";
        std::vector<afv_lba_params> prm;
        if (!afv_load_jobs(params, 1, sizeof(afv_lba_params), prm)) return (int)AFV_EINVAL;
        K.prm = prm[0];
        if (nk > 0 && !afv_load_jobs(cams, nk, sizeof(afv_lba_cam), K.cams)) return (int)AFV_EINVAL;
        const afv_lba_params &p = K.prm;
        for (int r = 0; r < 2; ++r)
            if (p.iterations[r] < 0 || (p.robust[r] != 0 && p.robust[r] != 1)) return (int)AFV_EINVAL;
        if ((p.checks != 0 && p.checks != 1) || (p.write_points != 0 && p.write_points != 1) || p.trial_budget < 0) return (int)AFV_EINVAL;
        return lba_impl(K, results, kf_out, xyz_out, edge_state);
    });
}

bool se3_ok(const float *T, int m) {
    for (size_t q = 0; q < 12 * (size_t)m; ++q)
        if (!(fabsf(T[q]) <= 3.402823466e38f)) return false;
    return true;
}

}  // namespace

extern "C" int afv_table_bundle_adjust(afv_table *t, afv_points *points, const int32_t *slots, int nk, int n_free, const afv_lba_cam *cams,
                                       const int32_t *point_ids, int np, const int32_t *obs_point, const int32_t *obs_kf, const int32_t *obs_idx, int ne,
                                       const afv_lba_params *params, const volatile int32_t *stop_flag, afv_lba_result *results, double *kf_out,
                                       double *xyz_out, uint8_t *edge_state) {
    return lba_entry(false, t, points, slots, nk, n_free, cams, point_ids, np, obs_point, obs_kf, obs_idx, ne, params, stop_flag, results, kf_out, xyz_out,
                     edge_state);
}

extern "C" int afv_table_global_bundle_adjust(afv_table *t, afv_points *points, const int32_t *slots, int nk, int n_free, const afv_lba_cam *cams,
                                              const int32_t *point_ids, int np, const int32_t *obs_point, const int32_t *obs_kf, const int32_t *obs_idx,
                                              int ne, const afv_lba_params *params, const volatile int32_t *stop_flag, afv_lba_result *results,
                                              double *kf_out, double *xyz_out, uint8_t *edge_state) {
    return lba_entry(true, t, points, slots, nk, n_free, cams, point_ids, np, obs_point, obs_kf, obs_idx, ne, params, stop_flag, results, kf_out, xyz_out,
                     edge_state);
}

// internal, for the tests of the capacity answer: the plan of an edge list against a block cap of the caller's choice (the entry point
// itself always uses AFV_GBA_MAX_L_BLOCKS).  obs_point ascending, obs_kf < n_free: free.  Returns AFV_OK or AFV_ECAPACITY; counts[3]: the
// blocks of L, the structural blocks among them, the free keyframes.  No device is touched.
extern "C" int afv_gba_plan_probe(int n_free, int np, const int32_t *obs_point, const int32_t *obs_kf, int ne, long long max_blocks, int32_t *counts) {
    if (n_free < 0 || n_free > AFV_GBA_MAX_KF || np < 0 || ne < 0 || (ne > 0 && (!obs_point || !obs_kf)) || !counts) return AFV_EINVAL;
    std::vector<int> pt_ptr((size_t)np + 1, 0);
    for (int e = 0; e < ne; ++e) {
        if (obs_point[e] < 0 || obs_point[e] >= np || obs_kf[e] < 0 || (e > 0 && obs_point[e] < obs_point[e - 1])) return AFV_EINVAL;
        pt_ptr[(size_t)obs_point[e] + 1] = e + 1;
    }
    for (int p = 0; p < np; ++p)
        if (pt_ptr[(size_t)p + 1] < pt_ptr[(size_t)p]) pt_ptr[(size_t)p + 1] = pt_ptr[(size_t)p];
    GbPlan P;
    if (gb_plan(n_free, np, pt_ptr.data(), obs_kf, max_blocks, P) == GB_PLAN_BLOCKS) return AFV_ECAPACITY;
    counts[0] = P.nb; counts[1] = P.ns; counts[2] = P.nf;
    return AFV_OK;
}

extern "C" int afv_points_correct_se3(afv_points *points, const int32_t *ids, int n, const int32_t *pair_of_point, const float *T_before,
                                      const float *T_after, int m, uint8_t *status) {
    if (!points || !afv_points_is_live(points) || n < 0 || m < 0 || m > AFV_GBA_MAX_KF) return AFV_EINVAL;
    if (n > 0 && (!ids || !pair_of_point || !status)) return AFV_EINVAL;
    if (m > 0 && (!T_before || !T_after)) return AFV_EINVAL;
    if (n > points->cap) return AFV_EINVAL;
    afv_ctx *c = points->c;
    return guarded(c, [&]() -> int {
        static const char *fn = "afv_points_correct_se3";
        if (n == 0) return (int)AFV_OK;
        {
            std::vector<uint8_t> seen((size_t)points->cap, 0);
            for (int i = 0; i < n; ++i) {
                const int id = ids[i];
                if (id < 0 || id >= points->cap) return lba_refuse(c, "a map-point id lies outside the store", fn);
                if (seen[(size_t)id]) return lba_refuse(c, "a map-point id is named twice", fn);
                seen[(size_t)id] = 1;
                if (pair_of_point[i] < -1 || pair_of_point[i] >= m) return lba_refuse(c, "a point's reference is out of range", fn);
            }
        }
        if (m > 0 && (!se3_ok(T_before, m) || !se3_ok(T_after, m))) return lba_refuse(c, "a transform is not finite", fn);
        HIPCHK(c, hipSetDevice(c->device));
        const size_t M = (size_t)std::max(m, 1);
        Blob b(c);
        const size_t o_from = b.put(T_before, M * 48 * (m > 0)), o_to = b.put(T_after, M * 48 * (m > 0));
        const size_t o_ids = b.put(ids, (size_t)n * 4), o_pair = b.put(pair_of_point, (size_t)n * 4);
        const size_t in_bytes = b.h.size();
        const size_t o_pst = b.reserve_scratch((size_t)n);
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        uint8_t *B = c->d_match;
        HIPCHK(c, b.upload(in_bytes));
        DevGbaCorrect J{};
        for (int k = 0; k < 3; ++k) J.pos[k] = points->P.pos[k];
        J.flags = points->P.flags; J.ids = reinterpret_cast<const int *>(B + o_ids); J.pair = reinterpret_cast<const int *>(B + o_pair);
        J.T_before = reinterpret_cast<const float *>(B + o_from); J.T_after = reinterpret_cast<const float *>(B + o_to);
        J.status = B + o_pst; J.n = n;
        afv_launch_gba_correct_points(&J, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, b.fetch(status, o_pst, (size_t)n, c->stream));
        HIPCHK(c, b.wait());
        return (int)AFV_OK;
    });
}
