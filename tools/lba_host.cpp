// lba_host.cpp — LocalBundleAdjustment / BundleAdjustment as tests/_lba_ref.py restates them, as a scalar host program: the work of
// every lane of csrc/k_lba.hip (csrc/afv_lba_math.h, shared text) called in plain loops, the 64-partial trees, the dense L L^T and the
// two drivers written out.  tools/time_lba.py times it against the device and tests/test_lba_host_cpu.py holds it to the restatement bit
// for bit.  Build: g++ -O3 -ffp-contract=off -std=c++17 -I anyfeature-vslam_amd/csrc -shared -fPIC (the tests), or -DLBA_HOST_MAIN for a
// stand-alone program on a constructed scene.
#include <cstdio>
#include <cstring>
#include <vector>

#include "afv_lba_math.h"
#include "afv_gba_math.h"
#include "afv_gba_plan.h"

// gba_host (below) is the same program with the block-sparse solve of afv_table_global_bundle_adjust (L7' of tests/_gba_ref.py): the plan
// of csrc/afv_gba_plan.h, the block arithmetic of csrc/afv_gba_math.h in the loops that csrc/k_gba.hip spreads over lanes.  tools/
// time_gba.py times it, tests/test_gba_host_cpu.py holds it to the restatement; -DGBA_HOST_MAIN builds its stand-alone program.

namespace {

double tree64(double (&p)[64]) {  // L5: p[l] += p[l + s], s = 32 .. 1
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
    return p[0];
}

struct Host {
    LbView V{};
    LbStatus st{};
    std::vector<LbCam> cam;
    std::vector<double> obs, e_chi2, pose, xyz, term, rho_trial, Hll, Hinv, Hpp, M, bS, dx;
    std::vector<uint8_t> stereo, e_on, e_state, p_on, p_fail, k_fail;
    std::vector<int> pt_ptr, kf_ptr, kf_edge;
    int32_t solve_fail = 0;
    int stop_at = -1, total_trials = 0;
    bool flag() const { return stop_at >= 0 && total_trials >= stop_at; }
    bool sparse = false;   // gba_host: L7'
    GbPlan plan;
    GbView G{};
    std::vector<double> L;
    int solve_fails = 0;   // trials that ended on a bad pivot
};

// L7': the blocks of L column by column, then the two substitutions into dx
bool solve_sparse(const LbView &V, const GbView &G) {
    double *L = G.L;
    for (int j = 0; j < G.nf; ++j) {
        const int b0 = G.col_ptr[j], m = G.col_ptr[j + 1] - b0 - 1;
        if (!gb_chol6(L + (size_t)b0 * 36)) return false;
        for (int t = 0; t < 6 * m; ++t) gb_trsm_row(L + (size_t)b0 * 36, L + (size_t)(b0 + 1 + t / 6) * 36, t % 6);
        for (int qi = 0; qi < m; ++qi)
            for (int qk = 0; qk <= qi; ++qk) {
                const int bi = b0 + 1 + qi, bk = b0 + 1 + qk;
                double *dst = L + (size_t)(qi == qk ? G.col_ptr[G.blk_row[bi]] : gb_block_of(G, G.blk_row[bi], G.blk_row[bk])) * 36;
                for (int a = 0; a < 6; ++a)
                    for (int c = 0; c < (qi == qk ? a + 1 : 6); ++c) gb_update_entry(L + (size_t)bi * 36, L + (size_t)bk * 36, dst, a, c);
            }
    }
    double *x = V.dx;
    for (int t = 0; t < 6 * G.nf; ++t) x[t] = V.bS[t];
    for (int j = 0; j < G.nf; ++j) {
        const int b0 = G.col_ptr[j];
        gb_fwd_diag(L + (size_t)b0 * 36, x + (size_t)j * 6);
        for (int b = b0 + 1; b < G.col_ptr[j + 1]; ++b)
            for (int a = 0; a < 6; ++a) gb_fwd_row(L + (size_t)b * 36, x + (size_t)j * 6, x + (size_t)G.blk_row[b] * 6, a);
    }
    for (int j = G.nf - 1; j >= 0; --j) {
        double s[6];
        for (int a = 0; a < 6; ++a) s[a] = gb_back_gather(G, x, j, a);
        gb_back_diag(L + (size_t)G.col_ptr[j] * 36, s, x + (size_t)j * 6);
    }
    return true;
}

// L7: the dense, unpivoted L L^T of M's lower triangle in place, then the two substitutions (the back substitution subtracts in descending k)
bool solve_reduced(const LbView &V) {
    const int n = 6 * V.nf;
    double *M = V.M;
    for (int j = 0; j < n; ++j) {
        double s = M[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) s = s - M[(size_t)j * n + k] * M[(size_t)j * n + k];
        if (!(s > 0.0 && lb_finite(s))) return false;
        const double d = sqrt(s);
        M[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            s = M[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s = s - M[(size_t)i * n + k] * M[(size_t)j * n + k];
            M[(size_t)i * n + j] = s / d;
        }
    }
    for (int i = 0; i < n; ++i) {
        double s = V.bS[i];
        for (int k = 0; k < i; ++k) s = s - M[(size_t)i * n + k] * V.dx[k];
        V.dx[i] = s / M[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = V.dx[i];
        for (int k = n - 1; k > i; --k) s = s - M[(size_t)k * n + i] * V.dx[k];
        V.dx[i] = s / M[(size_t)i * n + i];
    }
    return true;
}

void linearise(Host &H) {
    const LbView &V = H.V;
    for (int e = 0; e < V.ne; ++e) lb_edge_linearise(V, e);
    for (int p = 0; p < V.np; ++p) lb_point_build(V, p);
    for (int i = 0; i < V.nf; ++i) {
        double part[27][64], acc[27];
        for (int l = 0; l < 64; ++l) {
            lb_pose_partials(V, i, l, acc);
            for (int q = 0; q < 27; ++q) part[q][l] = acc[q];
        }
        for (int q = 0; q < 27; ++q) V.Hpp[(size_t)i * 27 + q] = tree64(part[q]);
    }
    double c[64], m[64];
    for (int l = 0; l < 64; ++l) {
        c[l] = lb_edge_partial(V, V.term + (size_t)54 * V.ne, l);
        m[l] = lb_diag_partial(V, l);
    }
    double mx = 0.0;
    for (int l = 0; l < 64; ++l) mx = m[l] > mx ? m[l] : mx;
    lb_begin(*V.st, tree64(c), mx);
}

void trial(Host &H) {
    const LbView &V = H.V;
    bool failed = false;
    for (int p = 0; p < V.np; ++p) {
        lb_point_invert(V, p);
        if (V.p_on[p] && V.p_fail[p]) failed = true;
    }
    auto schur_block = [&](int i, int j, double *blk) {
        double part[42][64], acc[42], sum[42];
        for (int l = 0; l < 64; ++l) {
            lb_schur_partials(V, i, j, l, acc);
            for (int q = 0; q < 42; ++q) part[q][l] = acc[q];
        }
        for (int q = 0; q < 42; ++q) sum[q] = tree64(part[q]);
        if (blk) gb_schur_store(V, blk, i, j, sum); else lb_schur_store(V, i, j, sum);
    };
    if (H.sparse) {
        for (int b = 0; b < H.G.nb; ++b) {
            double *blk = H.G.L + (size_t)b * 36;
            if (H.G.blk_kind[b]) {
                schur_block(H.G.blk_col[b], H.G.blk_row[b], blk);
            } else {
                for (int q = 0; q < 36; ++q) blk[q] = 0.0;
            }
        }
    } else {
        for (int i = 0; i < V.nf; ++i)
            for (int j = i; j < V.nf; ++j) schur_block(i, j, nullptr);
    }
    double temp = 0.0, scale = 0.0;
    if (!failed) {
        failed = H.sparse ? !solve_sparse(V, H.G) : !solve_reduced(V);
        H.solve_fails += failed;
    }
    if (!failed) {
        for (int p = 0; p < V.np; ++p) lb_point_step(V, p);
        for (int k = 0; k < V.nk; ++k) {
            lb_pose_step(V, k);
            if (k < V.nf && V.k_fail[k]) failed = true;
        }
    }
    if (!failed) {
        const bool robust = V.st->robust != 0;
        for (int e = 0; e < V.ne; ++e)
            if (V.e_on[e]) V.rho_trial[e] = lb_edge_rho0(V, e, 1 - V.st->buf, robust);
        double c[64], s[64];
        for (int l = 0; l < 64; ++l) {
            c[l] = lb_edge_partial(V, V.rho_trial, l);
            s[l] = lb_scale_partial(V, l);
        }
        temp = tree64(c);
        scale = tree64(s);
    }
    lb_judge(*V.st, failed, temp, scale);
    ++H.total_trials;
}

// SparseOptimizer::optimize(iterations): the flag is read before every iteration and after every trial
void optimize(Host &H, int iterations, int robust, int *it_out, int *tr_out, double *chi2_out, double *lam_out) {
    LbStatus &S = H.st;
    S.lam = 0.0; S.ni = 2.0; S.cur = 0.0; S.it = 0; S.qmax = 0; S.iterations = 0; S.trials = 0; S.max_it = iterations; S.robust = robust;
    int active = 0;
    for (int e = 0; e < H.V.ne; ++e) active += H.e_on[e];
    if (active > 0 && H.V.nf > 0 && iterations > 0 && !H.flag()) {  // L8
        int next = LB_NEXT_ITERATION;
        while (next != LB_NEXT_DONE) {
            if (next == LB_NEXT_ITERATION) linearise(H);
            trial(H);
            next = S.next;
            if (H.flag()) next = LB_NEXT_DONE;
        }
    }
    *it_out = S.iterations; *tr_out = S.trials; *chi2_out = S.cur; *lam_out = S.lam;
}

}  // namespace

// cams [nk][17]: Rcw (9), tcw (3), fx, fy, cx, cy, bf; pos [np][3]; p_ok [np]; obs [ne][4]: x, y, u_right, inf;
// params: iterations[2], robust[2], checks, stop_at (-1: never; 0: raised before the call)
// ints [8]: iterations[2], trials[2], n_edges, n_removed_first, n_erase, stopped; doubles [4]: chi2[2], lambda[2]
// sparse: L7' with at most max_blocks blocks of L; extra [3] (or null): the blocks of L, the structural blocks among them, the trials that
// ended on a bad pivot.  false: the fill exceeds max_blocks, nothing is written
static bool host_run(bool sparse, long long max_blocks, int nk, int nf, int np, int ne, const float *cams, const float *pos, const uint8_t *p_ok,
                     const int *e_pt, const int *e_kf, const float *obs, const int *params, int *ints, double *doubles, double *kf_out, double *xyz_out,
                     uint8_t *edge_state, int *extra) {
    Host H;
    H.sparse = sparse;
    LbView &V = H.V;
    V.nk = nk; V.nf = nf; V.np = np; V.ne = ne;
    const size_t n = 6 * (size_t)nf, E = (size_t)(ne > 0 ? ne : 1), P = (size_t)(np > 0 ? np : 1), K = (size_t)(nk > 0 ? nk : 1);
    H.cam.resize(K); H.obs.assign(5 * E, 0.0); H.e_chi2.assign(E, 0.0); H.pose.assign(2 * K * 12, 0.0); H.xyz.assign(2 * P * 3, 0.0);
    H.term.assign((size_t)LB_NT * E, 0.0); H.rho_trial.assign(E, 0.0); H.Hll.assign(P * 9, 0.0); H.Hinv.assign(P * 9, 0.0);
    H.Hpp.assign((size_t)(nf > 0 ? nf : 1) * 27, 0.0); H.M.assign(sparse ? 1 : n * n + 1, 0.0); H.bS.assign(n + 1, 0.0); H.dx.assign(n + 3 * P, 0.0);
    H.stereo.assign(E, 0); H.e_on.assign(E, 0); H.e_state.assign(E, 0); H.p_on.assign(P, 0); H.p_fail.assign(P, 0); H.k_fail.assign(K, 0);
    H.pt_ptr.assign(np + 1, 0); H.kf_ptr.assign(nf + 1, 0);
    for (int k = 0; k < nk; ++k) {
        const float *c = cams + 17 * (size_t)k;
        for (int q = 0; q < 12; ++q) H.pose[(size_t)k * 12 + q] = H.pose[(K + k) * 12 + q] = (double)c[q];
        H.cam[k] = LbCam{(double)c[12], (double)c[13], (double)c[14], (double)c[15], (double)c[16]};
    }
    for (int p = 0; p < np; ++p) {
        H.p_on[p] = p_ok[p] ? 1 : 0;
        for (int c = 0; c < 3; ++c) H.xyz[(size_t)p * 3 + c] = H.xyz[(P + p) * 3 + c] = H.p_on[p] ? (double)pos[3 * (size_t)p + c] : 0.0;
    }
    int n_edges = 0;
    for (int e = 0; e < ne; ++e) {
        const float *o = obs + 4 * (size_t)e;
        H.obs[e] = (double)o[0]; H.obs[E + e] = (double)o[1]; H.obs[2 * E + e] = (double)o[2]; H.obs[3 * E + e] = (double)o[3];
        H.obs[4 * E + e] = (double)(0.5f * (o[3] + o[3]));  // GetKeyPt1DInf
        H.stereo[e] = o[2] >= 0.0f ? 1 : 0;
        H.e_on[e] = H.p_on[e_pt[e]];
        H.e_state[e] = H.e_on[e] ? LB_KEPT : LB_DROPPED;
        n_edges += H.e_on[e];
        H.pt_ptr[e_pt[e] + 1] = e + 1;
        if (e_kf[e] < nf) ++H.kf_ptr[e_kf[e] + 1];
    }
    for (int p = 0; p < np; ++p)
        if (H.pt_ptr[p + 1] < H.pt_ptr[p]) H.pt_ptr[p + 1] = H.pt_ptr[p];  // a point without edges
    for (int i = 0; i < nf; ++i) H.kf_ptr[i + 1] += H.kf_ptr[i];
    H.kf_edge.assign((size_t)H.kf_ptr[nf] + 1, 0);
    {
        std::vector<int> at(H.kf_ptr.begin(), H.kf_ptr.end());
        for (int e = 0; e < ne; ++e)
            if (e_kf[e] < nf) H.kf_edge[at[e_kf[e]]++] = e;
    }
    V.cam = H.cam.data(); V.e_pt = e_pt; V.e_kf = e_kf; V.e_obs = H.obs.data(); V.e_stereo = H.stereo.data(); V.e_on = H.e_on.data();
    V.e_state = H.e_state.data(); V.e_chi2 = H.e_chi2.data(); V.pt_ptr = H.pt_ptr.data(); V.kf_ptr = H.kf_ptr.data(); V.kf_edge = H.kf_edge.data();
    V.p_on = H.p_on.data(); V.pose = H.pose.data(); V.xyz = H.xyz.data(); V.term = H.term.data(); V.rho_trial = H.rho_trial.data();
    V.Hll = H.Hll.data(); V.Hinv = H.Hinv.data(); V.Hpp = H.Hpp.data(); V.M = H.M.data(); V.bS = H.bS.data(); V.dx = H.dx.data();
    V.p_fail = H.p_fail.data(); V.k_fail = H.k_fail.data(); V.solve_fail = &H.solve_fail; V.st = &H.st;
    if (sparse) {
        if (gb_plan(nf, np, H.pt_ptr.data(), e_kf, max_blocks, H.plan) == GB_PLAN_BLOCKS) return false;
        H.L.assign(((size_t)H.plan.nb + 1) * 36, 0.0);
        H.G.nf = nf; H.G.nb = H.plan.nb; H.G.col_ptr = H.plan.col_ptr.data(); H.G.blk_row = H.plan.blk_row.data();
        H.G.blk_col = H.plan.blk_col.data(); H.G.blk_kind = H.plan.blk_kind.data(); H.G.L = H.L.data();
        if (extra) {
            extra[0] = H.plan.nb;
            extra[1] = H.plan.ns;
            extra[2] = 0;
        }
    }
    H.stop_at = params[5];
    const int checks = params[4];
    std::memset(ints, 0, 8 * sizeof(int));
    std::memset(doubles, 0, 4 * sizeof(double));
    ints[4] = n_edges;
    if (checks && H.flag()) {  // :645-647: nothing is written
        ints[7] = 1;
        return true;
    }
    optimize(H, params[0], params[2], &ints[0], &ints[2], &doubles[0], &doubles[2]);
    bool stopped = H.flag();
    if (stopped) ints[7] = 2;
    if (checks) {
        if (!stopped) {  // the first check (:662-692), then optimize(10) without the kernel
            for (int e = 0; e < ne; ++e) {
                if (!H.e_on[e]) continue;
                if (lb_edge_outlier(V, e, H.st.buf, false, H.e_chi2[e])) {
                    H.e_on[e] = 0;
                    H.e_state[e] = LB_REMOVED_KEPT;
                    ++ints[5];
                }
            }
            optimize(H, params[1], params[3], &ints[1], &ints[3], &doubles[1], &doubles[3]);
            if (H.flag()) ints[7] = 3;
        }
        for (int e = 0; e < ne; ++e) {  // the final check (:705-733) visits the removed edges too (L-Q1)
            if (H.e_state[e] == LB_DROPPED) continue;
            if (lb_edge_outlier(V, e, H.st.buf, H.e_state[e] == LB_REMOVED_KEPT, H.e_chi2[e])) {
                H.e_state[e] = LB_ERASE;
                ++ints[6];
            }
        }
    }
    const size_t b = (size_t)H.st.buf;
    for (int i = 0; i < nf; ++i)
        for (int q = 0; q < 12; ++q) kf_out[(size_t)i * 12 + q] = H.pose[(b * K + i) * 12 + q];
    for (int p = 0; p < np; ++p)
        for (int c = 0; c < 3; ++c) xyz_out[(size_t)p * 3 + c] = H.p_on[p] ? H.xyz[(b * P + p) * 3 + c] : 0.0;  // L9
    for (int e = 0; e < ne; ++e) edge_state[e] = H.e_state[e];
    if (sparse && extra) extra[2] = H.solve_fails;
    return true;
}

extern "C" void lba_host(int nk, int nf, int np, int ne, const float *cams, const float *pos, const uint8_t *p_ok, const int *e_pt, const int *e_kf,
                         const float *obs, const int *params, int *ints, double *doubles, double *kf_out, double *xyz_out, uint8_t *edge_state) {
    host_run(false, 0, nk, nf, np, ne, cams, pos, p_ok, e_pt, e_kf, obs, params, ints, doubles, kf_out, xyz_out, edge_state, nullptr);
}

// the arguments of lba_host; max_blocks: the cap on the blocks of L (the library's is AFV_GBA_MAX_L_BLOCKS); extra [3]: the blocks of L,
// the structural blocks among them, the trials that ended on a bad pivot.  Returns 0, or 1 when the fill exceeds max_blocks (nothing written)
extern "C" int gba_host(int nk, int nf, int np, int ne, const float *cams, const float *pos, const uint8_t *p_ok, const int *e_pt, const int *e_kf,
                        const float *obs, const int *params, long long max_blocks, int *ints, double *doubles, double *kf_out, double *xyz_out,
                        uint8_t *edge_state, int *extra) {
    return host_run(true, max_blocks, nk, nf, np, ne, cams, pos, p_ok, e_pt, e_kf, obs, params, ints, doubles, kf_out, xyz_out, edge_state, extra) ? 0 : 1;
}

// the plan alone: col_ptr [nf + 1], blk_row / blk_col / blk_kind [cap_blocks] are filled when the plan fits cap_blocks.  counts [2]: nb, ns.
// Returns 0, or 1 when the fill exceeds max_blocks
extern "C" int gba_plan_host(int nf, int np, int ne, const int *e_pt, const int *e_kf, long long max_blocks, int *counts, int *col_ptr, int *blk_row,
                             int *blk_col, uint8_t *blk_kind, int cap_blocks) {
    std::vector<int> pt_ptr((size_t)np + 1, 0);
    for (int e = 0; e < ne; ++e) pt_ptr[(size_t)e_pt[e] + 1] = e + 1;
    for (int p = 0; p < np; ++p)
        if (pt_ptr[(size_t)p + 1] < pt_ptr[(size_t)p]) pt_ptr[(size_t)p + 1] = pt_ptr[(size_t)p];
    GbPlan P;
    if (gb_plan(nf, np, pt_ptr.data(), e_kf, max_blocks, P) == GB_PLAN_BLOCKS) return 1;
    counts[0] = P.nb;
    counts[1] = P.ns;
    if (P.nb <= cap_blocks) {
        for (int j = 0; j <= nf; ++j) col_ptr[j] = P.col_ptr[(size_t)j];
        for (int b = 0; b < P.nb; ++b) {
            blk_row[b] = P.blk_row[(size_t)b];
            blk_col[b] = P.blk_col[(size_t)b];
            blk_kind[b] = P.blk_kind[(size_t)b];
        }
    }
    return 0;
}

#ifdef GBA_HOST_MAIN
// a constructed map: 70 keyframes in a row (69 free, the last fixed), 8 points per keyframe, every point seen by three neighbours, and one
// point that joins the last free keyframe to the first (a loop: fill); the global BA of loop closing (10 iterations, no kernel, no checks)
int main() {
    const int nk = 70, nf = 69, per = 8, np = nk * per + 1;
    std::vector<float> cams(17 * nk), pos(3 * (size_t)np), obs;
    std::vector<uint8_t> ok(np, 1);
    std::vector<int> e_pt, e_kf;
    for (int k = 0; k < nk; ++k) {
        float *o = cams.data() + 17 * k;
        const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        for (int q = 0; q < 9; ++q) o[q] = R[q];
        o[9] = -0.2f * (float)k; o[10] = 0.0f; o[11] = 0.0f;
        o[12] = 500.0f; o[13] = 500.0f; o[14] = 320.0f; o[15] = 240.0f; o[16] = 40.0f;
    }
    unsigned seed = 4321u;
    auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.0f; };
    auto add = [&](int p, int k) {
        const float *c = cams.data() + 17 * k;
        const float x = pos[3 * p] + c[9], y = pos[3 * p + 1] + c[10], z = pos[3 * p + 2] + c[11];
        e_pt.push_back(p); e_kf.push_back(k);
        const float u = 500.0f * x / z + 320.0f + (rnd() - 0.5f), v = 500.0f * y / z + 240.0f + (rnd() - 0.5f);
        obs.push_back(u); obs.push_back(v); obs.push_back((k & 1) ? u - 40.0f / z : -1.0f); obs.push_back(1.0f);
    };
    for (int p = 0; p < np - 1; ++p) {
        const int k0 = p / per;
        pos[3 * p] = 0.2f * (float)k0 + 2.0f * rnd() - 1.0f; pos[3 * p + 1] = 2.0f * rnd() - 1.0f; pos[3 * p + 2] = 4.0f + 4.0f * rnd();
        for (int d = -1; d <= 1; ++d)
            if (k0 + d >= 0 && k0 + d < nk) add(p, k0 + d);
    }
    pos[3 * (np - 1)] = 7.0f; pos[3 * (np - 1) + 1] = 0.1f; pos[3 * (np - 1) + 2] = 30.0f;
    add(np - 1, 0);
    add(np - 1, nf - 1);
    for (int p = 0; p < np; ++p) pos[3 * p] += 0.02f;
    const int ne = (int)e_pt.size();
    const int params[6] = {10, 0, 0, 0, 0, -1};
    int ints[8], extra[3];
    double d[4];
    std::vector<double> kf(12 * nf), xyz(3 * (size_t)np);
    std::vector<uint8_t> state(ne);
    if (gba_host(nk, nf, np, ne, cams.data(), pos.data(), ok.data(), e_pt.data(), e_kf.data(), obs.data(), params, 8, ints, d, kf.data(), xyz.data(),
                 state.data(), extra) != 1)
        return 2;  // eight blocks cannot hold it
    const int rc = gba_host(nk, nf, np, ne, cams.data(), pos.data(), ok.data(), e_pt.data(), e_kf.data(), obs.data(), params, 1 << 20, ints, d, kf.data(),
                            xyz.data(), state.data(), extra);
    std::printf("rc %d iterations %d trials %d n_edges %d stopped %d chi2 %.6f blocks %d structural %d solve_fail %d\n", rc, ints[0], ints[2], ints[4], ints[7],
                d[0], extra[0], extra[1], extra[2]);
    return rc == 0 && ints[4] == ne && ints[0] >= 1 && extra[0] > extra[1] && extra[2] == 0 ? 0 : 1;
}
#endif

#ifdef LBA_HOST_MAIN
// a constructed scene: 4 keyframes on an arc (2 free, 2 fixed), 40 points, every point seen by every keyframe, one gross outlier
int main() {
    const int nk = 4, nf = 2, np = 40, ne = nk * np;
    std::vector<float> cams(17 * nk), pos(3 * np), obs(4 * (size_t)ne);
    std::vector<uint8_t> ok(np, 1), state(ne);
    std::vector<int> e_pt(ne), e_kf(ne);
    for (int k = 0; k < nk; ++k) {
        const float a = 0.05f * (float)(k - 1), c = cosf(a), s = sinf(a);
        const float R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
        float *o = cams.data() + 17 * k;
        for (int q = 0; q < 9; ++q) o[q] = R[q];
        o[9] = -0.3f * (float)k; o[10] = 0.0f; o[11] = 0.0f;
        o[12] = 500.0f; o[13] = 500.0f; o[14] = 320.0f; o[15] = 240.0f; o[16] = 40.0f;
    }
    unsigned seed = 12345u;
    auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.0f; };
    for (int p = 0; p < np; ++p) {
        pos[3 * p] = 4.0f * rnd() - 2.0f; pos[3 * p + 1] = 2.0f * rnd() - 1.0f; pos[3 * p + 2] = 4.0f + 4.0f * rnd();
        for (int k = 0; k < nk; ++k) {
            const int e = p * nk + k;
            const float *c = cams.data() + 17 * k;
            const float x = c[0] * pos[3 * p] + c[1] * pos[3 * p + 1] + c[2] * pos[3 * p + 2] + c[9];
            const float y = c[3] * pos[3 * p] + c[4] * pos[3 * p + 1] + c[5] * pos[3 * p + 2] + c[10];
            const float z = c[6] * pos[3 * p] + c[7] * pos[3 * p + 1] + c[8] * pos[3 * p + 2] + c[11];
            e_pt[e] = p; e_kf[e] = k;
            obs[4 * e] = 500.0f * x / z + 320.0f + (rnd() - 0.5f); obs[4 * e + 1] = 500.0f * y / z + 240.0f + (rnd() - 0.5f);
            obs[4 * e + 2] = (k & 1) ? obs[4 * e] - 40.0f / z : -1.0f;
            obs[4 * e + 3] = 1.0f;
        }
    }
    obs[4 * 7] += 60.0f;
    for (int p = 0; p < np; ++p) pos[3 * p] += 0.02f;
    const int params[6] = {5, 10, 1, 0, 1, -1};
    int ints[8];
    double d[4];
    std::vector<double> kf(12 * nf), xyz(3 * np);
    lba_host(nk, nf, np, ne, cams.data(), pos.data(), ok.data(), e_pt.data(), e_kf.data(), obs.data(), params, ints, d, kf.data(), xyz.data(), state.data());
    std::printf("iterations %d %d trials %d %d n_edges %d removed_first %d n_erase %d stopped %d chi2 %.6f %.6f\n", ints[0], ints[1], ints[2], ints[3],
                ints[4], ints[5], ints[6], ints[7], d[0], d[1]);
    return ints[4] == ne && ints[6] >= 1 ? 0 : 1;
}
#endif
