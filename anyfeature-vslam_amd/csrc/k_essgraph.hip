// k_essgraph.hip — Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:771-1031) over plain arrays and the point correction of
// LoopClosing::CorrectLoop (LoopClosing.cc:487-516) over the map-point store (include/afv_hip.h, "Essential graph"; host side:
// afv_essgraph.hip).
//
//   per iteration    k_ess_perturb    a lane per (vertex, perturbation): the 14 estimates Sim3(+-delta e_d) * estimate
//                    k_ess_linearise  a lane per (edge, perturbation): the 28 perturbed errors and the error itself
//                    k_ess_terms      a lane per (edge, term): the edge's J^T J blocks, J^T (-e) and its chi2 (120 terms)
//                    k_ess_build      a wavefront per free vertex: H_ii, b_i with the 64-partial tree; a wavefront per off-diagonal
//                                     block of H: its edges one after the other, a lane per entry
//                    k_ess_begin      one wavefront: the chi2 (tree over the edge list); at iteration 0 lambda and the G5 test
//   per trial        k_ess_load       a lane per entry of L: H + lambda I on the pattern of L (fill reads 0), b
//                    k_ess_factor     ONE workgroup walks the block columns: a lane factors the diagonal block, a lane per row of every
//                                     sub-diagonal block solves it against L_jj, a wavefront per update triple applies L_ij L_kj^T (a lane
//                                     per entry); then the forward and the back substitution, column by column, in the same launch
//                    k_ess_step       a lane per vertex: the trial estimate into the other state buffer
//                    k_ess_trial      a lane per edge: its chi2 at the trial estimate
//                    k_ess_judge      one wavefront: the chi2 and computeScale trees, the failure flags, accept / reject, lambda, ni and
//                                     what comes next, into the status record the host reads in the trial's one wait
//   k_ess_recover    a lane per keyframe: S_out, Tiw, S^-1;   k_ess_correct_points: a lane per point, the store in place
// The host drives the trial loop (its length depends on the data); the decision is taken here.  No atomics, no spinning, no cooperative
// launch, no captured graph, plain vector stores.  The blocks of L live in global memory (at the caps 49 MiB); the walk of k_ess_factor
// is a latency chain: three barriers per column for the factorisation, two per column for each substitution - README, "Essential graph",
// has what that costs.
//
// The arithmetic is the restatement's (tests/_essgraph_ref.py), statement for statement; it is afv_essgraph_math.h, shared with the host
// program (tools/essgraph_host.cpp).  PARITY WITH g2o UNPINNED.  Deviations G1-G11: include/afv_hip.h has the text.
#include "afv_device.h"
#include "afv_runtime.h"
#include "afv_essgraph_math.h"
#include "afv_essgraph.h"

#define EG_T 256
#define EG_FACTOR_T 1024

__device__ __forceinline__ double eg_tree(double p) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}

__global__ void k_ess_round(const EgView V, int max_it) {
    EgStatus &S = *V.st;
    S.lam = 0.0; S.ni = 2.0; S.cur = 0.0; S.temp = 0.0; S.rho = 0.0; S.chi2_first = 0.0;
    S.buf = 0; S.it = 0; S.qmax = 0; S.iterations = 0; S.trials = 0; S.max_it = max_it; S.next = EG_NEXT_ITERATION; S.failed = 0; S.accepted = 0;
    S.status = EG_OK;
}

__global__ __launch_bounds__(EG_T) void k_ess_perturb(const EgView V) {
    const int tid = blockIdx.x * EG_T + threadIdx.x;
    if (tid < V.nk * 14) eg_perturb(V, tid / 14, tid % 14);
}

__global__ __launch_bounds__(EG_T) void k_ess_linearise(const EgView V) {
    const int tid = blockIdx.x * EG_T + threadIdx.x;
    if (tid < V.ne * EG_NP) eg_edge_perr(V, tid / EG_NP, tid % EG_NP);
}

__global__ __launch_bounds__(EG_T) void k_ess_terms(const EgView V) {
    const int tid = blockIdx.x * EG_T + threadIdx.x;
    if (tid < V.ne * EG_NT) eg_edge_term(V, tid / EG_NT, tid % EG_NT);
}

__global__ __launch_bounds__(64) void k_ess_build(const EgView V) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b < V.nf) {
        for (int q = 0; q < 35; ++q) {
            const double v = eg_tree(eg_vertex_partial(V, b, q, lane));
            if (lane == 0) V.Hd[(size_t)b * 35 + q] = v;
        }
    } else if (lane < 49) {
        const int q = b - V.nf;
        V.Aoff[(size_t)q * 49 + lane] = eg_offdiag_entry(V, q, lane / 7, lane % 7);
    }
}

__global__ __launch_bounds__(64) void k_ess_begin(const EgView V, double lambda_init) {
    const int lane = threadIdx.x;
    const double c = eg_tree(eg_edge_partial(V, V.term + 119, EG_NT, lane));
    bool bad = false;
    for (int e = lane; e < V.ne; e += 64) bad = bad || V.e_bad[e];
    const bool any = __ballot(bad) != 0ull;
    if (lane == 0) eg_begin(*V.st, c, any, lambda_init);
}

__global__ __launch_bounds__(EG_T) void k_ess_load(const EgView V) {
    const int tid = blockIdx.x * EG_T + threadIdx.x;
    if (tid < V.nb * 49) eg_load_entry(V, tid / 49, tid % 49);
    if (tid < V.nf * 7) V.rhs[tid] = V.Hd[(size_t)(tid / 7) * 35 + 28 + tid % 7];
}

// G1.  Every block is written by one lane per entry and read by other lanes only after the barrier that follows; the barriers are
// reached by all lanes (the early exit on a bad pivot is taken by the whole workgroup: s_bad is read after a barrier).
__global__ __launch_bounds__(EG_FACTOR_T) void k_ess_factor(const EgView V) {
    __shared__ int s_bad;
    __shared__ double s_s[7];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double *L = V.L;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int j = 0; j < V.nf; ++j) {
        const int b0 = V.col_ptr[j], m = V.col_ptr[j + 1] - b0 - 1;
        if (tid == 0 && !eg_chol7(L + (size_t)b0 * 49)) s_bad = 1;
        __syncthreads();
        if (s_bad) break;
        for (int t = tid; t < 7 * m; t += EG_FACTOR_T) eg_trsm_row(L + (size_t)b0 * 49, L + (size_t)(b0 + 1 + t / 7) * 49, t % 7);
        __syncthreads();
        for (int u = V.upd_ptr[j] + wave; u < V.upd_ptr[j + 1]; u += EG_FACTOR_T / 64)
            if (lane < 49)
                eg_update_entry(L + (size_t)V.upd[3 * u] * 49, L + (size_t)V.upd[3 * u + 1] * 49, L + (size_t)V.upd[3 * u + 2] * 49, lane / 7, lane % 7);
        __syncthreads();
    }
    const bool bad = s_bad != 0;
    if (tid == 0) *V.solve_fail = bad ? 1 : 0;
    if (bad) return;
    for (int j = 0; j < V.nf; ++j) {  // forward, ascending: y_j, then every row of column j
        const int b0 = V.col_ptr[j], m = V.col_ptr[j + 1] - b0 - 1;
        if (tid == 0) eg_fwd_diag(L + (size_t)b0 * 49, V.rhs + (size_t)j * 7);
        __syncthreads();
        for (int t = tid; t < 7 * m; t += EG_FACTOR_T) {
            const int b = b0 + 1 + t / 7;
            eg_fwd_row(L + (size_t)b * 49, V.rhs + (size_t)j * 7, V.rhs + (size_t)V.blk_row[b] * 7, t % 7);
        }
        __syncthreads();
    }
    for (int j = V.nf - 1; j >= 0; --j) {  // back, descending
        if (tid < 7) s_s[tid] = eg_back_gather(V, j, tid);
        __syncthreads();
        if (tid == 0) eg_back_diag(L + (size_t)V.col_ptr[j] * 49, s_s, V.rhs + (size_t)j * 7);
        __syncthreads();
    }
}

__global__ __launch_bounds__(EG_T) void k_ess_step(const EgView V) {
    const int k = blockIdx.x * EG_T + threadIdx.x;
    if (k < V.nk) eg_vertex_step(V, k);
}

__global__ __launch_bounds__(EG_T) void k_ess_trial(const EgView V) {
    const int e = blockIdx.x * EG_T + threadIdx.x;
    if (e < V.ne) eg_edge_trial(V, e);
}

__global__ __launch_bounds__(64) void k_ess_judge(const EgView V) {
    const int lane = threadIdx.x;
    bool bad = *V.solve_fail != 0;
    for (int i = lane; i < V.nf; i += 64) bad = bad || V.v_fail[i];
    for (int e = lane; e < V.ne; e += 64) bad = bad || V.e_bad[e];
    const bool failed = __ballot(bad) != 0ull;
    const double temp = eg_tree(eg_edge_partial(V, V.chi_trial, 1, lane));
    const double scale = eg_tree(eg_scale_partial(V, lane));
    if (lane == 0) eg_judge(*V.st, failed, temp, scale);
}

__global__ __launch_bounds__(EG_T) void k_ess_recover(const EgView V, double *S_out, double *Tiw, double *Swc) {
    const int k = blockIdx.x * EG_T + threadIdx.x;
    if (k < V.nk) eg_recover(V.S + ((size_t)V.st->buf * V.nk + k) * 13, S_out + (size_t)k * 13, Tiw + (size_t)k * 12, Swc + (size_t)k * 13);
}

__global__ __launch_bounds__(EG_T) void k_ess_correct_points(const DevEssCorrect J) {
    const int i = blockIdx.x * EG_T + threadIdx.x;
    if (i >= J.n) return;
    const int id = J.ids[i], q = J.pair[i];
    const unsigned f = J.flags[id];
    double out[3] = {0.0, 0.0, 0.0};
    uint8_t st = EG_MOVED;
    if (!(f & AFV_PTF_SET) || (f & AFV_PTF_BAD)) {
        st = EG_BAD_OR_UNSET;
    } else if (q < 0) {
        st = EG_NO_PAIR;
    } else {
        const float P[3] = {J.pos[0][id], J.pos[1][id], J.pos[2][id]};
        eg_correct(J.S_from + (size_t)q * 13, J.S_to + (size_t)q * 13, P, out);
        if (J.write_points) {
#pragma unroll
            for (int c = 0; c < 3; ++c) J.pos[c][id] = (float)out[c];  // SetWorldPos
        }
    }
    J.status[i] = st;
    if (J.xyz_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) J.xyz_out[(size_t)i * 3 + c] = out[c];
    }
}

static inline int eg_blocks(long long n) { return (int)((n + EG_T - 1) / EG_T); }

extern "C" void afv_launch_ess_round(const EgView *V, int max_it, hipStream_t stream) {
    hipLaunchKernelGGL(k_ess_round, dim3(1), dim3(1), 0, stream, *V, max_it);
}

// the callers guarantee nf >= 1 and ne >= 1 (G8)
extern "C" void afv_launch_ess_iteration(const EgView *V, double lambda_init, hipStream_t stream) {
    hipLaunchKernelGGL(k_ess_perturb, dim3(eg_blocks((long long)V->nk * 14)), dim3(EG_T), 0, stream, *V);
    hipLaunchKernelGGL(k_ess_linearise, dim3(eg_blocks((long long)V->ne * EG_NP)), dim3(EG_T), 0, stream, *V);
    hipLaunchKernelGGL(k_ess_terms, dim3(eg_blocks((long long)V->ne * EG_NT)), dim3(EG_T), 0, stream, *V);
    hipLaunchKernelGGL(k_ess_build, dim3(V->nf + V->nob), dim3(64), 0, stream, *V);
    hipLaunchKernelGGL(k_ess_begin, dim3(1), dim3(64), 0, stream, *V, lambda_init);
}

extern "C" void afv_launch_ess_trial(const EgView *V, hipStream_t stream) {
    hipLaunchKernelGGL(k_ess_load, dim3(eg_blocks((long long)V->nb * 49)), dim3(EG_T), 0, stream, *V);
    hipLaunchKernelGGL(k_ess_factor, dim3(1), dim3(EG_FACTOR_T), 0, stream, *V);
    hipLaunchKernelGGL(k_ess_step, dim3(eg_blocks(V->nk)), dim3(EG_T), 0, stream, *V);
    hipLaunchKernelGGL(k_ess_trial, dim3(eg_blocks(V->ne)), dim3(EG_T), 0, stream, *V);
    hipLaunchKernelGGL(k_ess_judge, dim3(1), dim3(64), 0, stream, *V);
}

extern "C" void afv_launch_ess_recover(const EgView *V, double *S_out, double *Tiw, double *Swc, hipStream_t stream) {
    hipLaunchKernelGGL(k_ess_recover, dim3(eg_blocks(V->nk)), dim3(EG_T), 0, stream, *V, S_out, Tiw, Swc);
}

extern "C" void afv_launch_ess_correct_points(const DevEssCorrect *J, hipStream_t stream) {
    if (J->n > 0) hipLaunchKernelGGL(k_ess_correct_points, dim3(eg_blocks(J->n)), dim3(EG_T), 0, stream, *J);
}
