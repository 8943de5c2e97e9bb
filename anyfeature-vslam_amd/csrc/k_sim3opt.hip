// k_sim3opt.hip — Optimizer::OptimizeSim3 (src/Optimizer.cc:1033-1226) over slots of the keyframe table and ids of the map-point store,
// for every candidate of a loop check at once (include/afv_hip.h, "OptimizeSim3"; host side: afv_sim3opt.hip).
//
//   k_sim3opt_gather  one workgroup per job.  The edge set (:1084-1163): filters i = 0 .. n1 - 1 (mp2 >= 0, mp1 >= 0, both points set
//                     and not bad, idx2 >= 0), compacts the survivors in ascending i (ballot + popcount ranks, a workgroup prefix, no
//                     atomics - k_sim3_gather's scheme) and writes per survivor P3D1c / P3D2c (float), the two observations and the two
//                     informations; writes every feature's first state (no match / not an edge / kept).
//   k_sim3opt_solve   ONE WAVEFRONT per job: optimize(5), the first classification, optimize(nMoreIterations), the second.  The
//                     estimate, H (28), b (7), lambda and the trial state are lane-uniform and live in registers; the 14 perturbed
//                     estimates of a linearisation (and their inverses) are computed once, lane p computing number p, and read across
//                     the lanes through scalar registers (afv_wave_read_f64); the lanes stride over the correspondences for residuals,
//                     Jacobian columns and the 36 partial sums; the halving tree is cross-lane moves.  No __syncthreads, no LDS, no
//                     spinning; the stream orders it behind the gather.  Every array is indexed at compile time (no scratch).
//
// The arithmetic is the restatement's (tests/_sim3opt_ref.py), statement for statement; its scalar part is afv_sim3opt_math.h, shared
// with the host program.  PARITY WITH g2o UNPINNED.  Deliberate deviations (include/afv_hip.h has the full text):
//   O1  classification at the accepted estimate          O2  a chi2 that is not finite is an outlier
//   O3  the state is R, t, s in double, no quaternion    O4  no library sin / cos / exp; failed trials beyond pi and |sigma| > 64
//   O5  64 partial sums, lane l takes l, l + 64, ..., then p[l] += p[l + s], s = 32 .. 1
//   O6  unpivoted L L^T, a bad pivot is a failed trial; fix_scale: row 6 holds lambda alone
//   O7  no (remaining) edges: nothing is evaluated
#include "afv_device.h"
#include "afv_runtime.h"
#include "afv_wave.h"
#include "afv_sim3opt_math.h"

#define SO_T AFV_SIM3OPT_T
#define SO_WAVES (SO_T / 64)
#define SO_SCALAR (1.0 / (2.0 * SO_DELTA))

__device__ __forceinline__ float so_row(const float *R, const float *t, int r, float X, float Y, float Z) {
    return (R[3 * r] * X + (R[3 * r + 1] * Y + R[3 * r + 2] * Z)) + t[r];
}

__global__ __launch_bounds__(SO_T) void k_sim3opt_gather(const DevSim3OptArgs A) {
    __shared__ int s_wave[SO_WAVES];
    const int tid = threadIdx.x, c = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const DevSim3OptJob &J = A.jobs[c];
    const size_t row0 = (size_t)c * A.cap;
    const int n1 = min(J.n1, A.cap);
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += SO_T) {
        const int i1 = i0 + tid;
        int p1 = -1, p2 = -1, k2 = -1;
        bool keep = false;
        if (i1 < n1) {
            p2 = A.mp2[row0 + i1];
            p1 = A.mp1[row0 + i1];
            k2 = A.idx2[row0 + i1];
            keep = p2 >= 0 && p2 < A.pcap && p1 >= 0 && p1 < A.pcap && k2 >= 0 && k2 < A.cap;
            if (keep) {
                const unsigned f1 = A.flags[p1], f2 = A.flags[p2];
                keep = (f1 & AFV_PTF_SET) && !(f1 & AFV_PTF_BAD) && (f2 & AFV_PTF_SET) && !(f2 & AFV_PTF_BAD);
            }
            A.state[row0 + i1] = p2 < 0 ? AFV_SIM3OPT_NO_MATCH : (keep ? AFV_SIM3OPT_KEPT : AFV_SIM3OPT_NOT_EDGE);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int rank = base + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < SO_WAVES; ++w) {
            if (w < wave) rank += s_wave[w];
            total += s_wave[w];
        }
        if (keep) {
            const size_t o = row0 + rank;
            DevSim3OptEdge e;
            const float X1 = A.pos[0][p1], Y1 = A.pos[1][p1], Z1 = A.pos[2][p1];
            const float X2 = A.pos[0][p2], Y2 = A.pos[1][p2], Z2 = A.pos[2][p2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                e.p1[r] = so_row(J.R1, J.t1, r, X1, Y1, Z1);
                e.p2[r] = so_row(J.R2, J.t2, r, X2, Y2, Z2);
            }
            e.obs1[0] = J.x1[i1]; e.obs1[1] = J.y1[i1];
            e.obs2[0] = J.x2[k2]; e.obs2[1] = J.y2[k2];
            e.inf1 = J.inf1[i1];
            e.inf2 = J.inf2[k2];
            A.edges[o] = e;
            A.index1[o] = i1;
            A.active[o] = 1;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) A.n[c] = base;
    for (int k = n1 + tid; k < A.cap; k += SO_T) A.state[row0 + k] = AFV_SIM3OPT_NO_MATCH;
    for (int k = base + tid; k < A.cap; k += SO_T) {
        A.index1[row0 + k] = -1;
        A.active[row0 + k] = 0;
    }
}

// ---- the solve: one wavefront ----
struct SoProblem {
    const DevSim3OptEdge *edges;  // the job's row
    uint8_t *active;
    int n;
    SoCam K1, K2;
    double delta, th2;
    bool fix_scale;
};

// O5: the halving tree over the 64 partial sums; every lane returns p[0]
__device__ __forceinline__ double so_tree(double p) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_down(p, s, 64);
    return afv_wave_read_f64(p, 0);
}

// correspondence k0 + lane of this pass, or (off) correspondence 0 as a stand-in whose terms are not added
__device__ __forceinline__ bool so_load(const SoProblem &P, int k0, int lane, bool need_active, SoEdge &g) {
    const int k = k0 + lane;
    const bool on = k < P.n && (!need_active || P.active[k] != 0);
    const DevSim3OptEdge e = P.edges[on ? k : 0];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        g.p1[r] = (double)e.p1[r];
        g.p2[r] = (double)e.p2[r];
    }
    g.obs1[0] = (double)e.obs1[0]; g.obs1[1] = (double)e.obs1[1];
    g.obs2[0] = (double)e.obs2[0]; g.obs2[1] = (double)e.obs2[1];
    g.inf1 = (double)e.inf1;
    g.inf2 = (double)e.inf2;
    return on;
}

__device__ __forceinline__ void so_read_est(const SoEst &v, int src, SoEst &out) {
#pragma unroll
    for (int k = 0; k < 9; ++k) out.R[k] = afv_wave_read_f64(v.R[k], src);
#pragma unroll
    for (int k = 0; k < 3; ++k) out.t[k] = afv_wave_read_f64(v.t[k], src);
    out.s = afv_wave_read_f64(v.s, src);
}

__device__ __forceinline__ double so_robust_chi2(const SoProblem &P, const SoPair &E, int lane) {
    double acc = 0.0;
    for (int k0 = 0; k0 < P.n; k0 += 64) {
        SoEdge g;
        const bool on = so_load(P, k0, lane, true, g);
        const double v = so_edge_robust(E, P.K1, P.K2, g, P.delta);
        acc = on ? acc + v : acc;
    }
    return so_tree(acc);
}

// computeActiveErrors + activeRobustChi2 + buildSystem: acc = H's upper triangle (28), b (7), the robust chi2
__device__ __forceinline__ void so_linearise(const SoProblem &P, const SoPair &E, int lane, double (&acc)[36]) {
    // BaseBinaryEdge::linearizeOplus: lane 2 d holds Sim3(+delta e_d) * estimate, lane 2 d + 1 Sim3(-delta e_d) * estimate, with their inverses
    SoPair mine;
    {
        const int d = lane >> 1;
        const double v = (lane & 1) ? -SO_DELTA : SO_DELTA;
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) u[k] = k == d ? v : 0.0;
        (void)so_step(E.f, u, P.fix_scale, mine);  // |u| = 1e-9: never a failed trial
    }
#pragma unroll
    for (int q = 0; q < 36; ++q) acc[q] = 0.0;
    for (int k0 = 0; k0 < P.n; k0 += 64) {
        SoEdge g;
        const bool on = so_load(P, k0, lane, true, g);
        double e12[2], e21[2], J12[2][7], J21[2][7];
        so_edge_errors(E, P.K1, P.K2, g, e12, e21);
#pragma unroll
        for (int d = 0; d < 7; ++d) {
            SoPair Ep, Em;
            double p12[2], p21[2], m12[2], m21[2];
            so_read_est(mine.f, 2 * d, Ep.f);
            so_read_est(mine.i, 2 * d, Ep.i);
            so_edge_errors(Ep, P.K1, P.K2, g, p12, p21);
            so_read_est(mine.f, 2 * d + 1, Em.f);
            so_read_est(mine.i, 2 * d + 1, Em.i);
            so_edge_errors(Em, P.K1, P.K2, g, m12, m21);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                J12[r][d] = SO_SCALAR * (p12[r] - m12[r]);
                J21[r][d] = SO_SCALAR * (p21[r] - m21[r]);
            }
        }
        double term[36];
        so_edge_terms(e12, e21, J12, J21, g.inf1, g.inf2, P.delta, term);
#pragma unroll
        for (int q = 0; q < 36; ++q) acc[q] = on ? acc[q] + term[q] : acc[q];
    }
#pragma unroll
    for (int q = 0; q < 36; ++q) acc[q] = so_tree(acc[q]);
}

struct SoStage {
    int iterations, trials;
    double chi2, lambda;
};

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve; E is the accepted estimate on return
__device__ __forceinline__ SoStage so_optimize(const SoProblem &P, SoPair &E, int n_active, int iterations, int lane) {
    SoStage S{0, 0, 0.0, 0.0};
    if (n_active == 0) return S;  // O7
    double lam = 0.0, ni = 2.0, cur = 0.0;
    for (int it = 0; it < iterations; ++it) {
        double acc[36], Hu[28], b[7];
        so_linearise(P, E, lane, acc);
#pragma unroll
        for (int q = 0; q < 28; ++q) Hu[q] = acc[q];
#pragma unroll
        for (int q = 0; q < 7; ++q) b[q] = acc[28 + q];
        cur = acc[35];
        if (it == 0) {
            lam = so_lambda_init(Hu);
            ni = 2.0;
        }
        ++S.iterations;
        double rho = 0.0;
        int qmax = 0;
        do {
            ++S.trials;
            double x[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            SoPair st = E;
            bool failed = !so_solve7(Hu, b, lam, x);
            if (!failed) failed = !so_step(E.f, x, P.fix_scale, st);
            double temp = 0.0;
            if (!failed) temp = so_robust_chi2(P, st, lane);
            const SoTrial T = so_judge(failed, cur, temp, x, b, lam, ni);
            rho = T.rho;
            if (T.accepted) {
                cur = temp;
                E = st;
            }
            ++qmax;
        } while (rho < 0.0 && qmax < SO_MAX_TRIALS);
        if (qmax == SO_MAX_TRIALS || rho == 0.0) break;
    }
    S.chi2 = cur;
    S.lambda = lam;
    return S;
}

__global__ __launch_bounds__(64) void k_sim3opt_solve(const DevSim3OptArgs A) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const DevSim3OptJob &J = A.jobs[c];
    const size_t row0 = (size_t)c * A.cap;
    SoProblem P;
    P.edges = A.edges + row0;
    P.active = A.active + row0;
    P.n = __builtin_amdgcn_readfirstlane(min(A.n[c], A.cap));
    P.K1 = SoCam{(double)J.fx1, (double)J.fy1, (double)J.cx1, (double)J.cy1};
    P.K2 = SoCam{(double)J.fx2, (double)J.fy2, (double)J.cx2, (double)J.cy2};
    P.delta = (double)sqrtf(J.th2);  // const float deltaHuber = sqrt(th2)
    P.th2 = (double)J.th2;
    P.fix_scale = J.fix_scale != 0;
    SoPair E0;
#pragma unroll
    for (int k = 0; k < 9; ++k) E0.f.R[k] = (double)J.R12[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) E0.f.t[k] = (double)J.t12[k];
    E0.f.s = (double)J.s12;
    so_inverse(E0.f, E0.i);
    SoPair E = E0;
    const int *index1 = A.index1 + row0;
    uint8_t *state = A.state + row0;

    const SoStage S0 = so_optimize(P, E, P.n, 5, lane);
    int n_bad = 0;
    for (int k0 = 0; k0 < P.n; k0 += 64) {  // the first classification: both edges and the match go
        SoEdge g;
        const bool in = so_load(P, k0, lane, false, g);
        const bool bad = in && so_edge_outlier(E, P.K1, P.K2, g, P.th2);
        if (bad) {
            P.active[k0 + lane] = 0;
            state[index1[k0 + lane]] = AFV_SIM3OPT_REMOVED_FIRST;
        }
        n_bad += __popcll(__ballot(bad));
    }
    const int more = n_bad > 0 ? 10 : 5;
    const bool early = P.n - n_bad < SO_MIN_CORRESPONDENCES;
    SoStage S1{0, 0, 0.0, 0.0};
    int n_in = 0;
    if (!early) {
        S1 = so_optimize(P, E, P.n - n_bad, more, lane);
        for (int k0 = 0; k0 < P.n; k0 += 64) {  // the second: matches only
            SoEdge g;
            const bool on = so_load(P, k0, lane, true, g);
            const bool bad = on && so_edge_outlier(E, P.K1, P.K2, g, P.th2);
            if (bad) state[index1[k0 + lane]] = AFV_SIM3OPT_REMOVED_SECOND;
            n_in += __popcll(__ballot(on && !bad));
        }
    }
    if (lane == 0) {
        const SoEst &out = early ? E0.f : E.f;  // answered 0: g2oS12 is not written back
        afv_sim3opt_result r;
        r.n_in = n_in; r.n_corr = P.n; r.n_bad = n_bad; r.more_iterations = more; r.early = early ? 1 : 0;
        r.iterations[0] = S0.iterations; r.iterations[1] = S1.iterations;
        r.trials[0] = S0.trials; r.trials[1] = S1.trials;
        r.reserved = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) r.R12[k] = out.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) r.t12[k] = out.t[k];
        r.s12 = out.s;
        r.chi2[0] = S0.chi2; r.chi2[1] = S1.chi2;
        r.lambda[0] = S0.lambda; r.lambda[1] = S1.lambda;
        A.results[c] = r;
    }
}

extern "C" void afv_launch_sim3opt_gather(const DevSim3OptArgs *args, hipStream_t stream) {
    hipLaunchKernelGGL(k_sim3opt_gather, dim3(args->nc), dim3(SO_T), 0, stream, *args);
}

extern "C" void afv_launch_sim3opt_solve(const DevSim3OptArgs *args, hipStream_t stream) {
    hipLaunchKernelGGL(k_sim3opt_solve, dim3(args->nc), dim3(64), 0, stream, *args);
}
