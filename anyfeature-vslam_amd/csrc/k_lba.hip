// k_lba.hip — Optimizer::LocalBundleAdjustment (src/Optimizer.cc:450-768) and Optimizer::BundleAdjustment (:61-243) over slots of the
// keyframe table and ids of the map-point store (include/afv_hip.h, "Bundle adjustment"; host side: afv_lba.hip).
//
//   k_lba_gather     once per call, a lane per edge / point / keyframe: filters the points (unset or bad: dropped with their edges), reads
//                    the observations, informations and positions, the poses and intrinsics as doubles.  (The by-keyframe order of the
//                    edges depends on obs_kf alone: the host builds it while it checks the arguments and uploads it with them.)
//   per iteration    k_lba_linearise  a lane per edge: error, both Jacobians, rho, the edge's Hpl and its contributions (55 terms)
//                    k_lba_build      a wavefront per free keyframe: Hpp, bp with the 64-partial tree; a lane per point: Hll, bl
//                    k_lba_begin      one wavefront: the robust chi2 (tree over the edge list), lambda at iteration 0
//   per trial        k_lba_invert     a lane per point: (Hll + lambda I)^-1 by cofactors, Hll^-1 bl
//                    k_lba_schur      a wavefront per block (i, j >= i) of the reduced system, striding over the edges of keyframe i and
//                                     looking up j in the point's short edge list; block (i, i) also yields bS_i
//                    k_lba_solve      one workgroup of 1024: the dense L L^T (at most 384 x 384, in global memory: 1.2 MB does not fit the
//                                     LDS) right-looking with the current column in the LDS, both substitutions as column sweeps
//                    k_lba_step       a lane per point / keyframe: the trial estimate into the other state buffer
//                    k_lba_trial      a lane per edge: its term of the trial chi2
//                    k_lba_judge      one wavefront: the trial chi2 and computeScale trees, the failure flags, accept / reject, lambda,
//                                     ni and what comes next, into the status record the host reads in the trial's one wait
//   k_lba_check      a lane per edge: the first / the final classification;  k_lba_finish: the outputs and the store
// The host drives the trial loop (its length depends on the data, and the stop flag is a host variable that must be honoured between
// trials); the decision is taken here.  No atomics, no spinning, no cooperative launch.
//
// The arithmetic is the restatement's (tests/_lba_ref.py), statement for statement; it is afv_lba_math.h, shared with the host program
// (tools/lba_host.cpp).  PARITY WITH g2o UNPINNED.  Deliberate deviations (include/afv_hip.h has the text):
//   L1  checks at the accepted estimate                  L2  a chi2 that is not finite is an outlier
//   L3  the state is R, t in double, no quaternion       L4  no libm; a step beyond pi is a failed trial
//   L5  one fixed shape per sum: 64 strided partials + halving tree per keyframe / over the edge list / over the unknowns; per point
//       one after the other                              L6  Hll^-1 by cofactors; det 0 or not finite: a failed trial
//   L7  dense unpivoted L L^T, ascending k; a bad pivot is a failed trial
//   L8  no free keyframe, no point or no edge: nothing is evaluated        L9  what is not written reads 0
#include "afv_device.h"
#include "afv_runtime.h"
#include "afv_lba_math.h"

#define LB_T 256

// L5: the halving tree over the 64 partial sums; lane 0 holds p[0]
__device__ __forceinline__ double lb_tree(double p) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}

__global__ __launch_bounds__(LB_T) void k_lba_gather(const LbView V, const DevLbaGather G) {
    const int tid = blockIdx.x * LB_T + threadIdx.x;
    if (tid < V.nk) {
        const float *c = G.cams + 17 * (size_t)tid;
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            V.pose[(size_t)tid * 12 + q] = (double)c[q];
            V.pose[((size_t)V.nk + tid) * 12 + q] = (double)c[q];
        }
        G.cam[tid] = LbCam{(double)c[12], (double)c[13], (double)c[14], (double)c[15], (double)c[16]};
    }
    if (tid < V.np) {
        const int id = G.point_ids[tid];
        const unsigned f = G.flags[id];
        const bool on = (f & AFV_PTF_SET) && !(f & AFV_PTF_BAD);
        G.p_on[tid] = on ? 1 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = on ? (double)G.pos[c][id] : 0.0;
            V.xyz[(size_t)tid * 3 + c] = v;
            V.xyz[((size_t)V.np + tid) * 3 + c] = v;
        }
    }
    if (tid < V.ne) {
        const size_t ne = (size_t)V.ne;
        const unsigned f = G.flags[G.point_ids[V.e_pt[tid]]];
        const bool on = (f & AFV_PTF_SET) && !(f & AFV_PTF_BAD);
        const size_t at = (size_t)G.slots[V.e_kf[tid]] * G.cap + G.obs_idx[tid];
        const float ur = G.geo[3 * G.plane + at], inf = G.inf[at];
        G.obs[tid] = (double)G.geo[at];
        G.obs[ne + tid] = (double)G.geo[G.plane + at];
        G.obs[2 * ne + tid] = (double)ur;
        G.obs[3 * ne + tid] = (double)inf;
        G.obs[4 * ne + tid] = (double)(0.5f * (inf + inf));  // GetKeyPt1DInf
        G.stereo[tid] = ur >= 0.0f ? 1 : 0;
        V.e_on[tid] = on ? 1 : 0;
        V.e_state[tid] = on ? LB_KEPT : LB_DROPPED;
        V.e_chi2[tid] = 0.0;
    }
}

__global__ void k_lba_round(const LbView V, int max_it, int robust) {
    LbStatus &S = *V.st;
    S.lam = 0.0; S.ni = 2.0; S.cur = 0.0; S.temp = 0.0; S.rho = 0.0;
    S.it = 0; S.qmax = 0; S.iterations = 0; S.trials = 0; S.max_it = max_it; S.robust = robust; S.next = LB_NEXT_ITERATION; S.failed = 0; S.accepted = 0;
}

__global__ __launch_bounds__(LB_T) void k_lba_linearise(const LbView V) {
    const int e = blockIdx.x * LB_T + threadIdx.x;
    if (e < V.ne) lb_edge_linearise(V, e);
}

__global__ __launch_bounds__(64) void k_lba_build(const LbView V) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b < V.nf) {
        double acc[27];
        lb_pose_partials(V, b, lane, acc);
#pragma unroll
        for (int q = 0; q < 27; ++q) {
            const double v = lb_tree(acc[q]);
            if (lane == 0) V.Hpp[(size_t)b * 27 + q] = v;
        }
    } else {
        const int p = (b - V.nf) * 64 + lane;
        if (p < V.np) lb_point_build(V, p);
    }
}

__global__ __launch_bounds__(64) void k_lba_begin(const LbView V) {
    const int lane = threadIdx.x;
    const double c = lb_tree(lb_edge_partial(V, V.term + (size_t)54 * V.ne, lane));
    double m = lb_diag_partial(V, lane);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double o = __shfl_down(m, s, 64);
        m = o > m ? o : m;
    }
    if (lane == 0) lb_begin(*V.st, c, m);
}

__global__ __launch_bounds__(LB_T) void k_lba_invert(const LbView V) {
    const int p = blockIdx.x * LB_T + threadIdx.x;
    if (p < V.np) lb_point_invert(V, p);
}

__global__ __launch_bounds__(64) void k_lba_schur(const LbView V) {
    const int i = blockIdx.y, j = blockIdx.x, lane = threadIdx.x;
    if (j < i) return;
    double acc[42];
    lb_schur_partials(V, i, j, lane, acc);
#pragma unroll
    for (int q = 0; q < 42; ++q) acc[q] = lb_tree(acc[q]);
    if (lane == 0) lb_schur_store(V, i, j, acc);
}

// L7: in place on M's lower triangle, right-looking: after column k is final, every element (i, j) with k < j <= i subtracts
// L[i][k] * L[j][k] - so each element subtracts its products in ascending k, as the restatement's left-looking loops do (same operations,
// same order, one rounding each).  Column k is staged in the LDS; the updates of a step are independent and coalesced along j.
#define LB_SOLVE_T 1024
__global__ __launch_bounds__(LB_SOLVE_T) void k_lba_solve(const LbView V) {
    __shared__ double s_col[6 * AFV_LBA_MAX_FREE];
    __shared__ double s_v;
    __shared__ int s_bad;
    const int n = 6 * V.nf, tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    double *M = V.M;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        if (tid == 0) {
            const double s = M[(size_t)k * n + k];
            if (!(s > 0.0 && lb_finite(s))) s_bad = 1;
            const double d = sqrt(s);
            M[(size_t)k * n + k] = d;
            s_v = d;
        }
        __syncthreads();
        const double d = s_v;
        for (int i = k + 1 + tid; i < n; i += LB_SOLVE_T) {
            const double v = M[(size_t)i * n + k] / d;
            M[(size_t)i * n + k] = v;
            s_col[i] = v;
        }
        __syncthreads();
        for (int i = k + 1 + ty; i < n; i += LB_SOLVE_T / 32) {
            const double li = s_col[i];
            for (int j = k + 1 + tx; j <= i; j += 32) M[(size_t)i * n + j] = M[(size_t)i * n + j] - li * s_col[j];
        }
        __syncthreads();
    }
    {   // forward: s_i -= L[i][k] y_k in ascending k; thread t owns row t (n <= 384)
        const int r = tid;
        double s = r < n ? V.bS[r] : 0.0;
        for (int k = 0; k < n; ++k) {
            if (k == r) s_v = s = s / M[(size_t)k * n + k];
            __syncthreads();
            const double y = s_v;
            if (r > k && r < n) s = s - M[(size_t)r * n + k] * y;
            __syncthreads();
        }
        // back: s_i -= L[k][i] x_k in descending k
        for (int k = n - 1; k >= 0; --k) {
            if (k == r) s_v = s = s / M[(size_t)k * n + k];
            __syncthreads();
            const double x = s_v;
            if (r < k) s = s - M[(size_t)k * n + r] * x;
            __syncthreads();
        }
        if (r < n) V.dx[r] = s;
    }
    if (tid == 0) *V.solve_fail = s_bad;
}

__global__ __launch_bounds__(LB_T) void k_lba_step(const LbView V) {
    const int tid = blockIdx.x * LB_T + threadIdx.x;
    if (tid < V.np) lb_point_step(V, tid);
    if (tid < V.nk) lb_pose_step(V, tid);
}

__global__ __launch_bounds__(LB_T) void k_lba_trial(const LbView V) {
    const int e = blockIdx.x * LB_T + threadIdx.x;
    if (e < V.ne && V.e_on[e]) V.rho_trial[e] = lb_edge_rho0(V, e, 1 - V.st->buf, V.st->robust != 0);
}

__global__ __launch_bounds__(64) void k_lba_judge(const LbView V) {
    const int lane = threadIdx.x;
    bool bad = *V.solve_fail != 0;
    for (int p = lane; p < V.np; p += 64) bad = bad || (V.p_on[p] && V.p_fail[p]);
    for (int k = lane; k < V.nf; k += 64) bad = bad || V.k_fail[k];
    const bool failed = __ballot(bad) != 0ull;
    const double temp = lb_tree(lb_edge_partial(V, V.rho_trial, lane));
    const double scale = lb_tree(lb_scale_partial(V, lane));
    if (lane == 0) lb_judge(*V.st, failed, temp, scale);
}

__global__ __launch_bounds__(LB_T) void k_lba_check(const LbView V, int final_check) {
    const int e = blockIdx.x * LB_T + threadIdx.x;
    if (e >= V.ne) return;
    const int buf = V.st->buf;
    if (!final_check) {
        if (!V.e_on[e]) return;
        double chi2 = 0.0;
        const bool bad = lb_edge_outlier(V, e, buf, false, chi2);
        V.e_chi2[e] = chi2;
        if (bad) {
            V.e_on[e] = 0;
            V.e_state[e] = LB_REMOVED_KEPT;
        }
    } else {
        const int st = V.e_state[e];
        if (st == LB_DROPPED) return;
        double chi2 = V.e_chi2[e];
        if (lb_edge_outlier(V, e, buf, st == LB_REMOVED_KEPT, chi2)) V.e_state[e] = LB_ERASE;
    }
}

__global__ __launch_bounds__(LB_T) void k_lba_finish(const LbView V, const DevLbaFinish F) {
    const int tid = blockIdx.x * LB_T + threadIdx.x, buf = V.st->buf;
    if (tid < V.nf) {
#pragma unroll
        for (int q = 0; q < 12; ++q) F.kf_out[(size_t)tid * 12 + q] = V.pose[((size_t)buf * V.nk + tid) * 12 + q];
    }
    if (tid < V.np) {
        const bool on = V.p_on[tid] != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = on ? V.xyz[((size_t)buf * V.np + tid) * 3 + c] : 0.0;  // L9
            F.xyz_out[(size_t)tid * 3 + c] = v;
            if (on && F.write_points) F.pos[c][F.point_ids[tid]] = (float)v;  // SetWorldPos
        }
    }
}

static inline int lb_blocks(int n) { return (n + LB_T - 1) / LB_T; }

extern "C" void afv_launch_lba_gather(const LbView *V, const DevLbaGather *G, hipStream_t stream) {
    const int n = std::max(V->ne, std::max(V->np, V->nk));
    if (n > 0) hipLaunchKernelGGL(k_lba_gather, dim3(lb_blocks(n)), dim3(LB_T), 0, stream, *V, *G);
}

extern "C" void afv_launch_lba_round(const LbView *V, int max_it, int robust, hipStream_t stream) {
    hipLaunchKernelGGL(k_lba_round, dim3(1), dim3(1), 0, stream, *V, max_it, robust);
}

// the callers guarantee nf >= 1, np >= 1, ne >= 1 (L8)
extern "C" void afv_launch_lba_iteration(const LbView *V, hipStream_t stream) {
    hipLaunchKernelGGL(k_lba_linearise, dim3(lb_blocks(V->ne)), dim3(LB_T), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_build, dim3(V->nf + (V->np + 63) / 64), dim3(64), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_begin, dim3(1), dim3(64), 0, stream, *V);
}

extern "C" void afv_launch_lba_trial(const LbView *V, hipStream_t stream) {
    hipLaunchKernelGGL(k_lba_invert, dim3(lb_blocks(V->np)), dim3(LB_T), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_schur, dim3(V->nf, V->nf), dim3(64), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(LB_SOLVE_T), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_step, dim3(lb_blocks(std::max(V->np, V->nk))), dim3(LB_T), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_trial, dim3(lb_blocks(V->ne)), dim3(LB_T), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_judge, dim3(1), dim3(64), 0, stream, *V);
}

// the same launches around another solve (k_gba.hip: the block-sparse route of afv_table_global_bundle_adjust)
extern "C" void afv_launch_lba_trial_head(const LbView *V, hipStream_t stream) {
    hipLaunchKernelGGL(k_lba_invert, dim3(lb_blocks(V->np)), dim3(LB_T), 0, stream, *V);
}

extern "C" void afv_launch_lba_trial_tail(const LbView *V, hipStream_t stream) {
    hipLaunchKernelGGL(k_lba_step, dim3(lb_blocks(std::max(V->np, V->nk))), dim3(LB_T), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_trial, dim3(lb_blocks(V->ne)), dim3(LB_T), 0, stream, *V);
    hipLaunchKernelGGL(k_lba_judge, dim3(1), dim3(64), 0, stream, *V);
}

extern "C" void afv_launch_lba_check(const LbView *V, int final_check, hipStream_t stream) {
    if (V->ne > 0) hipLaunchKernelGGL(k_lba_check, dim3(lb_blocks(V->ne)), dim3(LB_T), 0, stream, *V, final_check);
}

extern "C" void afv_launch_lba_finish(const LbView *V, const DevLbaFinish *F, hipStream_t stream) {
    const int n = std::max(V->np, V->nf);
    if (n > 0) hipLaunchKernelGGL(k_lba_finish, dim3(lb_blocks(n)), dim3(LB_T), 0, stream, *V, *F);
}
