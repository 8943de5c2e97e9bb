// afv_essgraph.hip — host side of afv_essential_graph and afv_points_correct_sim3 (include/afv_hip.h, "Essential graph"; kernels:
// k_essgraph.hip).
//
// Reference call shape: LoopClosing::CorrectLoop calls Optimizer::OptimizeEssentialGraph (src/LoopClosing.cc:581) on the host, through g2o
// and Eigen's sparse Cholesky, and then walks every map point of the map.  Here the host derives the plan from the edge list while it
// checks the arguments (afv_essgraph_plan.h: the by-vertex order of the edges, the blocks of H, the symbolic factorisation in the order of
// the keyframe list, the update triples), everything goes up in one copy, and the host drives the Levenberg loop: per trial it enqueues
// the trial's launches, waits once, reads the status record and follows what the device decided.  The points are corrected where they
// live, with the inverses the recovery has just written on the device.
#include "afv_runtime.h"
#include "afv_essgraph.h"
#include "afv_essgraph_plan.h"

static_assert(sizeof(afv_sim3d) == 104 && sizeof(afv_ess_params) == 24 && sizeof(afv_ess_result) == 40, "afv_ess records");

namespace {

int ess_refuse(afv_ctx *c, const char *fn, const char *why, int rc = AFV_EINVAL) {
    c->last_error = std::string(fn) + ": " + why;
    return rc;
}

bool sim3_ok(const afv_sim3d *S, int n) {
    for (int i = 0; i < n; ++i) {
        const double *p = reinterpret_cast<const double *>(S + i);
        for (int q = 0; q < 13; ++q)
            if (!so_finite(p[q])) return false;
        if (!(S[i].s > 0.0)) return false;
    }
    return true;
}

// ids inside the store and distinct, pairs in [-1, m)
int points_ok(afv_ctx *c, const char *fn, const afv_points *points, const int32_t *ids, const int32_t *pair, int n, int m) {
    std::vector<uint8_t> seen((size_t)points->cap, 0);
    for (int i = 0; i < n; ++i) {
        const int id = ids[i];
        if (id < 0 || id >= points->cap) return ess_refuse(c, fn, "a map-point id lies outside the store");
        if (seen[(size_t)id]) return ess_refuse(c, fn, "a map-point id is named twice");
        seen[(size_t)id] = 1;
        if (pair[i] < -1 || pair[i] >= m) return ess_refuse(c, fn, "a point's reference is out of range");
    }
    return AFV_OK;
}

int ess_impl(afv_ctx *c, afv_points *points, const afv_sim3d *S_init, int nk, int fixed, const int32_t *v0, const int32_t *v1, const afv_sim3d *meas, int ne,
             const afv_ess_params &prm, const int32_t *ids, const int32_t *ref, int np, afv_ess_result *result, afv_sim3d *S_out, double *Tiw_out,
             double *xyz_out, uint8_t *point_status) {
    static const char *fn = "afv_essential_graph";
    if (fixed < 0 || fixed >= nk) return ess_refuse(c, fn, "fixed is out of range");
    for (int e = 0; e < ne; ++e) {
        if (v0[e] < 0 || v0[e] >= nk || v1[e] < 0 || v1[e] >= nk) return ess_refuse(c, fn, "an edge end is out of range");
        if (v0[e] == v1[e]) return ess_refuse(c, fn, "an edge joins a vertex with itself");
    }
    if (!sim3_ok(S_init, nk)) return ess_refuse(c, fn, "an initial Sim3 is not finite or has s <= 0");
    if (ne > 0 && !sim3_ok(meas, ne)) return ess_refuse(c, fn, "a measurement is not finite or has s <= 0");
    if (np > 0) {
        const int rc = points_ok(c, fn, points, ids, ref, np, nk);
        if (rc) return rc;
    }
    EgPlan P;
    const int prc = eg_plan(nk, fixed, ne, v0, v1, AFV_ESS_MAX_L_BLOCKS, AFV_ESS_MAX_UPDATES, P);
    if (prc == EG_PLAN_BLOCKS) return ess_refuse(c, fn, "the fill of the keyframe order exceeds AFV_ESS_MAX_L_BLOCKS", AFV_ECAPACITY);
    if (prc == EG_PLAN_UPDATES) return ess_refuse(c, fn, "the update triples of the keyframe order exceed AFV_ESS_MAX_UPDATES", AFV_ECAPACITY);
    HIPCHK(c, hipSetDevice(c->device));
    const int nf = P.nf;
    const size_t E = (size_t)std::max(ne, 1), F = (size_t)std::max(nf, 1), K = (size_t)nk, NP = (size_t)std::max(np, 1);
    const size_t NB = (size_t)std::max(P.nb, 1), NOB = (size_t)std::max(P.nob, 1);
    // the image: inputs first (one upload), then what the host reads back, then device-only scratch beyond the image
    Blob b(c);
    auto put_ints = [&](const std::vector<int> &v) { return b.put(v.data(), v.size() * 4); };
    const size_t o_init = b.put(S_init, K * 104), o_S = b.put(S_init, K * 104, 8);
    b.put(S_init, K * 104, 8);  // the second state buffer follows the first
    const size_t o_meas = b.put(meas, E * 104 * (ne > 0)), o_v0 = b.put(v0, E * 4 * (ne > 0)), o_v1 = b.put(v1, E * 4 * (ne > 0));
    const size_t o_vof = put_ints(P.vertex_of), o_sof = put_ints(P.sys_of), o_vep = put_ints(P.ve_ptr), o_vee = put_ints(P.ve_edge);
    const size_t o_obp = put_ints(P.ob_ptr), o_obe = put_ints(P.ob_edge), o_colp = put_ints(P.col_ptr), o_brow = put_ints(P.blk_row);
    const size_t o_bcol = put_ints(P.blk_col), o_bsrc = put_ints(P.blk_src), o_updp = put_ints(P.upd_ptr), o_upd = put_ints(P.upd);
    const size_t o_ids = b.put(ids, NP * 4 * (np > 0)), o_ref = b.put(ref, NP * 4 * (np > 0));
    const size_t o_status = b.reserve(sizeof(EgStatus));  // zero: buffer 0 holds the estimate
    const size_t in_bytes = b.h.size();
    const size_t o_Sout = b.reserve_scratch(K * 104), o_Tiw = b.reserve_scratch(K * 96), o_xyz = b.reserve_scratch(NP * 24), o_pst = b.reserve_scratch(NP);
    size_t cur = align_up(b.h.size(), 256);
    auto take = [&](size_t bytes) {
        const size_t o = cur;
        cur = align_up(cur + std::max<size_t>(bytes, 8), 256);
        return o;
    };
    const size_t o_Swc = take(K * 104), o_pert = take(K * 14 * 104), o_perr = take(E * EG_NP * 56), o_term = take(E * EG_NT * 8), o_Hd = take(F * 35 * 8);
    const size_t o_Aoff = take(NOB * 392), o_L = take(NB * 392), o_rhs = take(F * 56), o_chi = take(E * 8), o_ebad = take(E), o_vfail = take(F), o_sfail = take(4);
    const int rc = ensure_match_buffer(c, cur);
    if (rc) return rc;
    uint8_t *B = c->d_match;
    HIPCHK(c, b.upload(in_bytes));
    auto ints = [&](size_t o) { return reinterpret_cast<const int *>(B + o); };
    auto dbl = [&](size_t o) { return reinterpret_cast<double *>(B + o); };
    EgView V{};
    V.nk = nk; V.nf = nf; V.ne = ne; V.fixed = fixed; V.fix_scale = prm.fix_scale; V.nob = P.nob; V.nb = P.nb; V.nu = P.nu;
    V.v0 = ints(o_v0); V.v1 = ints(o_v1); V.meas = dbl(o_meas); V.S = dbl(o_S); V.vertex_of = ints(o_vof); V.sys_of = ints(o_sof);
    V.ve_ptr = ints(o_vep); V.ve_edge = ints(o_vee); V.ob_ptr = ints(o_obp); V.ob_edge = ints(o_obe); V.col_ptr = ints(o_colp);
    V.blk_row = ints(o_brow); V.blk_col = ints(o_bcol); V.blk_src = ints(o_bsrc); V.upd_ptr = ints(o_updp); V.upd = ints(o_upd);
    V.pert = dbl(o_pert); V.perr = dbl(o_perr); V.term = dbl(o_term); V.Hd = dbl(o_Hd); V.Aoff = dbl(o_Aoff); V.L = dbl(o_L); V.rhs = dbl(o_rhs);
    V.chi_trial = dbl(o_chi); V.e_bad = B + o_ebad; V.v_fail = B + o_vfail; V.solve_fail = reinterpret_cast<int32_t *>(B + o_sfail);
    V.st = reinterpret_cast<EgStatus *>(B + o_status);
    afv_ess_result R{};
    R.l_blocks = P.nb;
    const EgStatus *h_status = reinterpret_cast<const EgStatus *>(b.h.data() + o_status);
    if (nf == 0 || ne == 0 || prm.iterations <= 0) {  // G8
        R.status = AFV_ESS_EMPTY;
    } else {
        afv_launch_ess_round(&V, prm.iterations, c->stream);
        int next = EG_NEXT_ITERATION;
        for (int guard = 0; next != EG_NEXT_DONE && guard <= SO_MAX_TRIALS * prm.iterations; ++guard) {
            if (next == EG_NEXT_ITERATION) afv_launch_ess_iteration(&V, prm.lambda_init, c->stream);
            afv_launch_ess_trial(&V, c->stream);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(b.h.data() + o_status, B + o_status, sizeof(EgStatus), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // the trial's one wait
            next = h_status->next;
        }
        R.iterations = h_status->iterations; R.trials = h_status->trials; R.chi2_first = h_status->chi2_first; R.chi2_last = h_status->cur;
        R.lambda = h_status->lam; R.status = h_status->status;
    }
    afv_launch_ess_recover(&V, dbl(o_Sout), dbl(o_Tiw), dbl(o_Swc), c->stream);
    if (np > 0) {
        DevEssCorrect J{};
        for (int k = 0; k < 3; ++k) J.pos[k] = points->P.pos[k];
        J.flags = points->P.flags; J.ids = ints(o_ids); J.pair = ints(o_ref); J.S_from = dbl(o_init); J.S_to = dbl(o_Swc);
        J.xyz_out = dbl(o_xyz); J.status = B + o_pst; J.n = np; J.write_points = prm.write_points;
        afv_launch_ess_correct_points(&J, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, b.fetch(S_out, o_Sout, K * 104, c->stream));
    HIPCHK(c, b.fetch(Tiw_out, o_Tiw, K * 96, c->stream));
    if (np > 0) {
        HIPCHK(c, b.fetch(xyz_out, o_xyz, (size_t)np * 24, c->stream));
        HIPCHK(c, b.fetch(point_status, o_pst, (size_t)np, c->stream));
    }
    HIPCHK(c, b.wait());
    *result = R;
    return AFV_OK;
}

}  // namespace

extern "C" int afv_essential_graph(afv_ctx *ctx, afv_points *points, const afv_sim3d *S_init, int nk, int fixed, const int32_t *edge_v0,
                                   const int32_t *edge_v1, const afv_sim3d *edge_meas, int ne, const afv_ess_params *params, const int32_t *point_ids,
                                   const int32_t *point_ref, int np, afv_ess_result *result, afv_sim3d *S_out, double *Tiw_out, double *xyz_out,
                                   uint8_t *point_status) {
    if (!ctx || !S_init || !params || !result || !S_out || !Tiw_out) return AFV_EINVAL;
    if (nk < 1 || nk > AFV_ESS_MAX_KF || ne < 0 || ne > AFV_ESS_MAX_EDGES || np < 0) return AFV_EINVAL;
    if (ne > 0 && (!edge_v0 || !edge_v1 || !edge_meas)) return AFV_EINVAL;
    if (np > 0 && (!points || !point_ids || !point_ref || !xyz_out || !point_status)) return AFV_EINVAL;
    if (points && (!afv_points_is_live(points) || points->c != ctx)) return AFV_EINVAL;
    if (points && np > points->cap) return AFV_EINVAL;
    return guarded(ctx, [&]() -> int {
        std::vector<afv_ess_params> prm;
        if (!afv_load_jobs(params, 1, sizeof(afv_ess_params), prm)) return (int)AFV_EINVAL;
        const afv_ess_params &p = prm[0];
        if (p.iterations < 0 || (p.fix_scale != 0 && p.fix_scale != 1) || (p.write_points != 0 && p.write_points != 1) || !(p.lambda_init > 0.0) ||
            !so_finite(p.lambda_init))
            return (int)AFV_EINVAL;
        return ess_impl(ctx, points, S_init, nk, fixed, edge_v0, edge_v1, edge_meas, ne, p, point_ids, point_ref, np, result, S_out, Tiw_out, xyz_out,
                        point_status);
    });
}

extern "C" int afv_points_correct_sim3(afv_points *points, const int32_t *ids, int n, const int32_t *pair_of_point, const afv_sim3d *S_from,
                                       const afv_sim3d *S_to, int m, uint8_t *status) {
    if (!points || !afv_points_is_live(points) || n < 0 || m < 0 || m > AFV_ESS_MAX_KF) return AFV_EINVAL;
    if (n > 0 && (!ids || !pair_of_point || !status)) return AFV_EINVAL;
    if (m > 0 && (!S_from || !S_to)) return AFV_EINVAL;
    if (n > points->cap) return AFV_EINVAL;
    afv_ctx *c = points->c;
    return guarded(c, [&]() -> int {
        static const char *fn = "afv_points_correct_sim3";
        if (n == 0) return (int)AFV_OK;
        const int rc0 = points_ok(c, fn, points, ids, pair_of_point, n, m);
        if (rc0) return rc0;
        if (m > 0 && (!sim3_ok(S_from, m) || !sim3_ok(S_to, m))) return ess_refuse(c, fn, "a Sim3 is not finite or has s <= 0");
        HIPCHK(c, hipSetDevice(c->device));
        const size_t M = (size_t)std::max(m, 1);
        Blob b(c);
        const size_t o_from = b.put(S_from, M * 104 * (m > 0)), o_to = b.put(S_to, M * 104 * (m > 0));
        const size_t o_ids = b.put(ids, (size_t)n * 4), o_pair = b.put(pair_of_point, (size_t)n * 4);
        const size_t in_bytes = b.h.size();
        const size_t o_pst = b.reserve_scratch((size_t)n);
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        uint8_t *B = c->d_match;
        HIPCHK(c, b.upload(in_bytes));
        DevEssCorrect J{};
        for (int k = 0; k < 3; ++k) J.pos[k] = points->P.pos[k];
        J.flags = points->P.flags; J.ids = reinterpret_cast<const int *>(B + o_ids); J.pair = reinterpret_cast<const int *>(B + o_pair);
        J.S_from = reinterpret_cast<const double *>(B + o_from); J.S_to = reinterpret_cast<const double *>(B + o_to);
        J.xyz_out = nullptr; J.status = B + o_pst; J.n = n; J.write_points = 1;
        afv_launch_ess_correct_points(&J, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, b.fetch(status, o_pst, (size_t)n, c->stream));
        HIPCHK(c, b.wait());
        return (int)AFV_OK;
    });
}
