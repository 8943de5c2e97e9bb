// k_triangulate.hip — the match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:315-461) over slots of the keyframe table
// (include/afv_hip.h, "new map points"; host side: afv_triangulate.hip).
//
//   k_tri_points  a lane per (pair, feature i of keyframe a); feature j of keyframe b = match12[pair][i].  Parallax test, linear
//                 triangulation through the 4 x 4 Jacobi SVD or a stereo unprojection, depth tests, reprojection gates, scale consistency:
//                 all in registers.  Writes status, route, x3D and the number of accepted matches of its workgroup.
//   k_tri_store   the same grid: ranks the accepted matches in (pair, feature) order from the workgroup counts, writes new_id / n_new and,
//                 when the call has a store whose capacity takes every new id, what MapPoint::MapPoint + UpdateNormalAndDepth
//                 (MapPoint.cc:372-418) would hold for the point and the descriptor row of feature i, device to device.
//
// The arithmetic is the restatement's (tests/_tri_ref.py), statement for statement: float, one rounding per operator (the build's
// -ffp-contract=off; hipcc's correctly rounded divide and square root), three-term sums as a0 + (a1 + a2), the comparisons the reference
// evaluates in double evaluated in double.  The SVD restates OpenCV 4.x's JacobiSVDImpl_<float> - PARITY UNPINNED.
// Quirks restated as written: Q1 the stereo gate of keyframe b uses keyframe a's mbf (:438); Q2 UnprojectStereo reads the distorted
// keypoint (KeyFrame.cc:664-665).
// Deliberate deviations: T1 cos(2 atan2(mb / 2, d)) = (d^2 - h^2) / (d^2 + h^2) in float, h = mb / 2; T2 hypot(p, beta) =
// sqrt(p * p + beta * beta) in double; T3 an x3D with a component that is not finite is rejected.
#include "k_tri_match.h"

__global__ __launch_bounds__(TRI_T) void k_tri_points(const DevTriArgs A) {
    __shared__ int s_cnt[TRI_WAVES];
    const int tid = threadIdx.x, p = blockIdx.y, i = blockIdx.x * TRI_T + tid;
    const DevTriPair &J = A.pairs[p];
    int j = -1;
    if (i < J.n1 && i < A.cap) {
        j = A.match12[(size_t)p * A.cap + i];
        if (j >= J.n2) j = -1;  // (the host refused such a call)
    }
    int route;
    float X, Y, Z;
    const int status = tri_judge(J, i, j, route, X, Y, Z);
    if (i < A.cap) {
        const size_t o = (size_t)p * A.cap + i;
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
        A.blk_count[p * A.nblk + blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(TRI_T) void k_tri_store(const DevTriArgs A) {
    __shared__ int s_red[3][TRI_WAVES];
    __shared__ int s_wave[TRI_WAVES];
    __shared__ int s_id[TRI_T];
    const int tid = threadIdx.x, p = blockIdx.y, b = blockIdx.x, i = b * TRI_T + tid;
    const DevTriPair &J = A.pairs[p];
    // accepted matches ahead of this workgroup (pair order, then feature order), of its pair, of the call
    const int me = p * A.nblk + b, lo = p * A.nblk, hi = lo + A.nblk, nall = A.npairs * A.nblk;
    int before = 0, pair = 0, all = 0;
    for (int k = tid; k < nall; k += TRI_T) {
        const int c = A.blk_count[k];
        all += c;
        if (k < me) before += c;
        if (k >= lo && k < hi) pair += c;
    }
    for (int off = 32; off > 0; off >>= 1) {
        before += __shfl_down(before, off);
        pair += __shfl_down(pair, off);
        all += __shfl_down(all, off);
    }
    if ((tid & 63) == 0) {
        s_red[0][tid >> 6] = before; s_red[1][tid >> 6] = pair; s_red[2][tid >> 6] = all;
    }
    const bool acc = i < A.cap && A.status[(size_t)p * A.cap + i] == TS_ACCEPTED;
    const unsigned long long m = __ballot(acc);
    if ((tid & 63) == 0) s_wave[tid >> 6] = __popcll(m);
    __syncthreads();
    before = pair = all = 0;
#pragma unroll
    for (int w = 0; w < TRI_WAVES; ++w) {
        before += s_red[0][w]; pair += s_red[1][w]; all += s_red[2][w];
    }
    int rank = __popcll(m & ((1ull << (tid & 63)) - 1ull));
#pragma unroll
    for (int w = 0; w < TRI_WAVES; ++w)
        if (w < (tid >> 6)) rank += s_wave[w];
    const int id = acc ? A.first_id + before + rank : -1;
    if (i < A.cap) A.new_id[(size_t)p * A.cap + i] = id;
    if (b == 0 && tid == 0) A.n_new[p] = pair;
    if (me == 0 && tid == 0) *A.total = all;
    const DevPointPlanes &P = A.P;
    // a range that does not fit leaves the store untouched: the host answers AFV_ECAPACITY from `total` (uniform)
    if (!A.has_points || (long long)A.first_id + all > (long long)P.cap) return;
    s_id[tid] = id;
    if (acc) {
        const size_t o = (size_t)p * A.cap + i;
        tri_store_point(P, J, i, id, A.x3d[3 * o], A.x3d[3 * o + 1], A.x3d[3 * o + 2]);
    }
    __syncthreads();
    tri_store_rows(P, J, s_id, b * TRI_T, tid);
}

extern "C" void afv_launch_tri_points(const DevTriArgs *args, hipStream_t stream) {
    hipLaunchKernelGGL(k_tri_points, dim3(args->nblk, args->npairs), dim3(TRI_T), 0, stream, *args);
}

extern "C" void afv_launch_tri_store(const DevTriArgs *args, hipStream_t stream) {
    hipLaunchKernelGGL(k_tri_store, dim3(args->nblk, args->npairs), dim3(TRI_T), 0, stream, *args);
}
