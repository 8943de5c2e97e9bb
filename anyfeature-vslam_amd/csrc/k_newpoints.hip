// k_newpoints.hip — the neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:265-472) as a chain of launches on one
// stream (include/afv_hip.h, afv_table_create_new_points; host side: afv_newpoints.hip).  Two launches per neighbour k, grid
// (ceil(cap / 256), 1), a lane per feature i of the current keyframe:
//
//   k_newpts_judge  the row search of SearchForTriangulation (tri_row<W>, k_tri_row.h) under the device masks as the store launch of
//                   neighbour k - 1 left them, then the judgement of the match (tri_judge, k_tri_match.h) in the same lane: the match
//                   never leaves its registers.  Writes match12, status, route, x3D and the number of accepted matches of its workgroup.
//   k_newpts_store  ranks the accepted lanes as k_tri_store does, takes the id base from next_id[k], writes new_id / n_new[k], the point
//                   planes and the descriptor row (tri_store_point / tri_store_rows) and sets the two masks.
//
// What neighbour k + 1 needs from neighbour k - the mask of the current keyframe and the next free id - travels through device memory and
// the ORDER OF THE STREAM: a launch reads cell k of next_id / stop, one thread of the store launch writes cell k + 1; no cell is read and
// written by the same launch, no workgroup waits for another.  stop[k] set = the points of an earlier neighbour did not fit the store:
// every workgroup of both launches leaves at once (the host fills the rows of those neighbours).
// Several features of the current keyframe may match the same feature j of a neighbour (vbMatched2 is never set, FeatureMatcher.cc:681,
// 724): their mask writes store the same value.
#include "k_tri_match.h"
#include "k_tri_row.h"

__global__ __launch_bounds__(TRI_T) void k_newpts_judge(const DevNewPtsArgs A, const int k) {
    __shared__ int s_cnt[TRI_WAVES];
    if (A.stop[k]) return;  // (uniform)
    const int tid = threadIdx.x, i = blockIdx.x * TRI_T + tid;
    const DevTriPair &J = A.pairs[k];
    int j = -1;
    if (i < J.n1 && i < A.cap) j = tri_row_any(A.search[k], i);
    int route;
    float X, Y, Z;
    const int status = tri_judge(J, i, j, route, X, Y, Z);
    if (i < A.cap) {
        const size_t o = (size_t)k * A.cap + i;
        A.match12[o] = j;
        A.status[o] = (uint8_t)status;
        A.route[o] = (uint8_t)route;
        A.x3d[3 * o] = X; A.x3d[3 * o + 1] = Y; A.x3d[3 * o + 2] = Z;
    }
    const unsigned long long m = __ballot(status == TS_ACCEPTED);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < TRI_WAVES; ++w) n += s_cnt[w];
        A.blk_count[k * A.nblk + blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(TRI_T) void k_newpts_store(const DevNewPtsArgs A, const int k) {
    __shared__ int s_red[2][TRI_WAVES];
    __shared__ int s_wave[TRI_WAVES];
    __shared__ int s_id[TRI_T];
    const int tid = threadIdx.x, b = blockIdx.x, i = b * TRI_T + tid;
    const int base = A.next_id[k];
    if (A.stop[k]) {  // (uniform) the rule is handed on
        if (b == 0 && tid == 0) {
            A.stop[k + 1] = 1;
            A.next_id[k + 1] = base;
            A.n_new[k] = 0;
        }
        return;
    }
    const DevTriPair &J = A.pairs[k];
    // accepted matches ahead of this workgroup (feature order), of the neighbour
    const int *cnt = A.blk_count + k * A.nblk;
    int before = 0, all = 0;
    for (int w = tid; w < A.nblk; w += TRI_T) {
        const int c = cnt[w];
        all += c;
        if (w < b) before += c;
    }
    for (int off = 32; off > 0; off >>= 1) {
        before += __shfl_down(before, off);
        all += __shfl_down(all, off);
    }
    if ((tid & 63) == 0) {
        s_red[0][tid >> 6] = before; s_red[1][tid >> 6] = all;
    }
    const size_t o = (size_t)k * A.cap + i;
    const bool acc = i < A.cap && A.status[o] == TS_ACCEPTED;
    const unsigned long long m = __ballot(acc);
    if ((tid & 63) == 0) s_wave[tid >> 6] = __popcll(m);
    __syncthreads();
    before = all = 0;
#pragma unroll
    for (int w = 0; w < TRI_WAVES; ++w) {
        before += s_red[0][w]; all += s_red[1][w];
    }
    int rank = __popcll(m & ((1ull << (tid & 63)) - 1ull));
#pragma unroll
    for (int w = 0; w < TRI_WAVES; ++w)
        if (w < (tid >> 6)) rank += s_wave[w];
    const DevPointPlanes &P = A.P;
    // the points of this neighbour go beyond the store: it and every later neighbour do nothing (uniform over the launch)
    const bool fits = !A.has_points || (long long)base + all <= (long long)P.cap;
    if (b == 0 && tid == 0) {
        A.stop[k + 1] = fits ? 0 : 1;
        A.next_id[k + 1] = fits ? base + all : base;
        A.n_new[k] = fits ? all : 0;
    }
    if (!fits) return;
    const int id = acc ? base + before + rank : -1;
    if (i < A.cap) A.new_id[o] = id;
    if (acc) {
        A.mask_cur[i] = 1;
        A.mask_nb[(size_t)k * A.cap + A.match12[o]] = 1;
    }
    if (!A.has_points) return;
    s_id[tid] = id;
    if (acc) tri_store_point(P, J, i, id, A.x3d[3 * o], A.x3d[3 * o + 1], A.x3d[3 * o + 2]);
    __syncthreads();
    tri_store_rows(P, J, s_id, b * TRI_T, tid);
}

extern "C" void afv_launch_newpts_judge(const DevNewPtsArgs *args, int k, hipStream_t stream) {
    hipLaunchKernelGGL(k_newpts_judge, dim3(args->nblk), dim3(TRI_T), 0, stream, *args, k);
}

extern "C" void afv_launch_newpts_store(const DevNewPtsArgs *args, int k, hipStream_t stream) {
    hipLaunchKernelGGL(k_newpts_store, dim3(args->nblk), dim3(TRI_T), 0, stream, *args, k);
}
