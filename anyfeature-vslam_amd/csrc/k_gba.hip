// k_gba.hip — the block-sparse solve of afv_table_global_bundle_adjust (Optimizer::GlobalBundleAdjustemnt, src/Optimizer.cc:53-58, as
// LoopClosing::RunGlobalBundleAdjustment calls it: every keyframe of the map free except keyId == 0) and the float point correction of
// RunGlobalBundleAdjustment (LoopClosing.cc:731-750).  include/afv_hip.h, "Global bundle adjustment"; host side: afv_lba.hip.
//
// Everything of a trial but the solve is k_lba.hip's, launched unchanged.  Between k_lba_invert and k_lba_step stand, per trial:
//   k_gba_schur      a wavefront per block of L, from the plan's list (never an nf x nf grid): a structural block (i, j >= i) of the
//                    reduced system is evaluated as k_lba_schur does (lb_schur_partials, the 64-partial tree) and stored into the block
//                    of L it loads to, block (i, i) also yields bS_i; a fill block is zeroed (36 lanes, the load step folded in)
//   k_gba_factor     ONE workgroup of 1024 walks the block columns: a lane factors the diagonal 6 x 6 block, a lane per row solves the
//                    sub-diagonal blocks against it, a lane per entry of the target block applies L_ik L_jk^T (28 updates of 36 entries
//                    per pass; the target is found by a binary search in its column's rows, no update triples are stored); then the
//                    forward and the back substitution, column by column, in the same launch, into dx in the dense layout that
//                    k_lba_step reads.  On a bad pivot the whole workgroup leaves after a barrier that every lane has reached.
// No atomics, no spinning, no cooperative launch, no captured graph, plain vector stores.  The blocks of L live in global memory (288
// bytes each); the dense n x n matrix of k_lba_solve does not exist on this route.
//
// The arithmetic is the restatement's (tests/_gba_ref.py, deviation L7'), statement for statement; it is afv_gba_math.h, shared with the
// host program (tools/lba_host.cpp, gba_host).  Every scalar element of L subtracts its products one after the other in ascending k: the
// updates of block column k reach an element before those of column k + 1, and inside a column in ascending c.
#include "afv_device.h"
#include "afv_runtime.h"
#include "afv_gba_math.h"

#define GB_T 256
#define GB_FACTOR_T 1024
#define GB_UPD_PER_PASS (GB_FACTOR_T / 36)   // 28 updates of 36 entries: 1008 of the 1024 lanes

__device__ __forceinline__ double gb_tree(double p) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}

__global__ __launch_bounds__(64) void k_gba_schur(const LbView V, const GbView G) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= G.nb) return;
    double *blk = G.L + (size_t)b * 36;
    if (!G.blk_kind[b]) {
        if (lane < 36) blk[lane] = 0.0;
        return;
    }
    const int i = G.blk_col[b], j = G.blk_row[b];
    double acc[42];
    lb_schur_partials(V, i, j, lane, acc);
#pragma unroll
    for (int q = 0; q < 42; ++q) acc[q] = gb_tree(acc[q]);
    if (lane == 0) gb_schur_store(V, blk, i, j, acc);
}

// L7'.  Every block is written by one lane per entry and read by other lanes only after the barrier that follows; the barriers are
// reached by all lanes (the early exit on a bad pivot is taken by the whole workgroup: s_bad is read after a barrier).
__global__ __launch_bounds__(GB_FACTOR_T) void k_gba_factor(const LbView V, const GbView G) {
    __shared__ int s_bad;
    __shared__ double s_s[6];
    const int tid = threadIdx.x, nf = G.nf;
    double *L = G.L;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int j = 0; j < nf; ++j) {
        const int b0 = G.col_ptr[j], m = G.col_ptr[j + 1] - b0 - 1;
        if (tid == 0 && !gb_chol6(L + (size_t)b0 * 36)) s_bad = 1;
        __syncthreads();
        if (s_bad) break;
        for (int t = tid; t < 6 * m; t += GB_FACTOR_T) gb_trsm_row(L + (size_t)b0 * 36, L + (size_t)(b0 + 1 + t / 6) * 36, t % 6);
        __syncthreads();
        const long long nu = (long long)m * (m + 1) / 2;
        const int slot = tid / 36, entry = tid % 36;
        if (slot < GB_UPD_PER_PASS) {
            for (long long u = slot; u < nu; u += GB_UPD_PER_PASS) {
                int qi, qk;
                gb_update_pair(u, qi, qk);
                const int bi = b0 + 1 + qi, bk = b0 + 1 + qk, a = entry / 6, c = entry % 6;
                if (qi == qk) {
                    if (c <= a) gb_update_entry(L + (size_t)bi * 36, L + (size_t)bk * 36, L + (size_t)G.col_ptr[G.blk_row[bi]] * 36, a, c);
                } else {
                    gb_update_entry(L + (size_t)bi * 36, L + (size_t)bk * 36, L + (size_t)gb_block_of(G, G.blk_row[bi], G.blk_row[bk]) * 36, a, c);
                }
            }
        }
        __syncthreads();
    }
    const bool bad = s_bad != 0;
    if (tid == 0) *V.solve_fail = bad ? 1 : 0;
    if (bad) return;
    double *x = V.dx;
    for (int t = tid; t < 6 * nf; t += GB_FACTOR_T) x[t] = V.bS[t];
    __syncthreads();
    for (int j = 0; j < nf; ++j) {  // forward, ascending: y_j, then every row of column j
        const int b0 = G.col_ptr[j], m = G.col_ptr[j + 1] - b0 - 1;
        if (tid == 0) gb_fwd_diag(L + (size_t)b0 * 36, x + (size_t)j * 6);
        __syncthreads();
        for (int t = tid; t < 6 * m; t += GB_FACTOR_T) {
            const int b = b0 + 1 + t / 6;
            gb_fwd_row(L + (size_t)b * 36, x + (size_t)j * 6, x + (size_t)G.blk_row[b] * 6, t % 6);
        }
        __syncthreads();
    }
    for (int j = nf - 1; j >= 0; --j) {  // back, descending
        if (tid < 6) s_s[tid] = gb_back_gather(G, x, j, tid);
        __syncthreads();
        if (tid == 0) gb_back_diag(L + (size_t)G.col_ptr[j] * 36, s_s, x + (size_t)j * 6);
        __syncthreads();
    }
}

// LoopClosing.cc:731-750: a lane per point, the store in place, in float
__global__ __launch_bounds__(GB_T) void k_gba_correct_points(const DevGbaCorrect J) {
    const int i = blockIdx.x * GB_T + threadIdx.x;
    if (i >= J.n) return;
    const int id = J.ids[i], q = J.pair[i];
    const unsigned f = J.flags[id];
    uint8_t st = AFV_POINT_MOVED;
    if (!(f & AFV_PTF_SET) || (f & AFV_PTF_BAD)) {
        st = AFV_POINT_BAD_OR_UNSET;
    } else if (q < 0) {
        st = AFV_POINT_NO_PAIR;
    } else {
        const float P[3] = {J.pos[0][id], J.pos[1][id], J.pos[2][id]};
        float out[3];
        gb_correct_se3(J.T_before + (size_t)q * 12, J.T_after + (size_t)q * 12, P, out);
#pragma unroll
        for (int c = 0; c < 3; ++c) J.pos[c][id] = out[c];  // SetWorldPos
    }
    J.status[i] = st;
}

extern "C" void afv_launch_gba_solve(const LbView *V, const GbView *G, hipStream_t stream) {
    hipLaunchKernelGGL(k_gba_schur, dim3(G->nb), dim3(64), 0, stream, *V, *G);
    hipLaunchKernelGGL(k_gba_factor, dim3(1), dim3(GB_FACTOR_T), 0, stream, *V, *G);
}

extern "C" void afv_launch_gba_correct_points(const DevGbaCorrect *J, hipStream_t stream) {
    if (J->n > 0) hipLaunchKernelGGL(k_gba_correct_points, dim3((J->n + GB_T - 1) / GB_T), dim3(GB_T), 0, stream, *J);
}
