// k_tri_row.h - the row search of SearchForTriangulation (FeatureMatcher.cc:640-760) for ONE feature of keyframe 1, and the float
// descriptor distance it shares with the other matchers of k_match.hip.  One copy of the program text for the kernels that run it:
// k_match_tri (k_match.hip: the match as an answer of its own) and k_newpts_judge (k_newpoints.hip: the match stays in the lane's
// registers and is judged at once).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "afv_jobs.h"
#include "afv_wave.h"

// ---------------- float descriptors inside the BoW-guided matchers (round 6; W == 0 in the templates) ----------------
// FeatureMatcher::DescriptorDistance dispatches on DescriptorType (FeatureMatcher.cc:1508-1531, called from SearchByBoW :236 / :616 and
// SearchForTriangulation :734); for SIFT128 / SURF64 / KAZE64 / R2D2 it is cv::norm(a, b, NORM_L2SQR) narrowed to float
// (Feature_sift128.cpp:132-134, Types.h:127).  A non-negative float's bits order like the number, so (best key, second distance) =
// (distance bits << 32 | position, distance bits) merge exactly like the integer pair of the binary path.
__device__ __forceinline__ float l2sqr(const float *a, const float *b, int n) {
    // normL2Sqr<float,double>: float differences, double squares, 4-way partial sums
    double s = 0;
    int i = 0;
    for (; i <= n - 4; i += 4) {
        const double v0 = (double)(a[i] - b[i]), v1 = (double)(a[i + 1] - b[i + 1]), v2 = (double)(a[i + 2] - b[i + 2]),
                     v3 = (double)(a[i + 3] - b[i + 3]);
        s += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
    }
    for (; i < n; ++i) {
        const double v = (double)(a[i] - b[i]);
        s += v * v;
    }
    return (float)s;
}
__device__ __forceinline__ const float *frow(const uint32_t *base, int idx, int dim) { return reinterpret_cast<const float *>(base) + (size_t)idx * dim; }

// ---------------- M4: SearchForTriangulation ----------------

// One thread per KF1 feature (row_seg = the shared node it belongs to, -1 if none): rows are independent here (vbMatched2 is
// never set, FeatureMatcher.cc:681,724), so the whole job runs in one pass; the threads of a wave mostly sit in the same node
// and read the same KF2 candidates (uniform loads).  Equal distances: the LAST candidate in the node's order wins (:736).
template <int W>
__device__ int tri_row(const DevTriJob &T, int idx1) {
    const DevMatchJob &J = T.m;
    const int sg = T.row_seg[idx1];
    if (sg < 0) return -1;
    if (J.valid1 && J.valid1[idx1]) return -1;  // already has a MapPoint (:699-703)
    const bool stereo1 = T.u_right1 && T.u_right1[idx1] >= 0.0f;  // :705
    if (T.only_stereo && !stereo1) return -1;                      // :707-709
    const Seg S = J.segs[sg];
    uint32_t q[W == 0 ? 1 : W];
    if constexpr (W != 0) {
#pragma unroll
        for (int i = 0; i < W; ++i) q[i] = J.d1[(size_t)idx1 * W + i];
    }
    const float kx = T.x1[idx1], ky = T.y1[idx1];
    // epipolar line in image 2: l = x1' F12 (:168-170)
    const float la = kx * T.F[0] + ky * T.F[3] + T.F[6];
    const float lb = kx * T.F[1] + ky * T.F[4] + T.F[7];
    const float lc = kx * T.F[2] + ky * T.F[5] + T.F[8];
    const float den = la * la + lb * lb;
    if (den == 0) return -1;
    std::conditional_t<W == 0, float, int> best;  // bestDist starts at TH_LOW (:714): the test below against J.th says the same
    if constexpr (W == 0) best = 3.402823466e+38f;
    else best = 0x7fffffff;
    int best_idx = -1;
    for (int b = 0; b < S.n2; ++b) {
        const int idx2 = J.idx2 ? J.idx2[S.s2 + b] : S.s2 + b;
        if (J.valid2 && J.valid2[idx2]) continue;
        const bool stereo2 = T.u_right2 && T.u_right2[idx2] >= 0.0f;  // :727
        if (T.only_stereo && !stereo2) continue;                      // :729-731
        decltype(best) d;
        if constexpr (W == 0) {
            (void)q;
            d = l2sqr(frow(J.d1, idx1, J.fdim), frow(J.d2, idx2, J.fdim), J.fdim);
        } else {
            d = afv_hamming<W>(q, J.d2 + (size_t)idx2 * W);
        }
        if ((float)d > J.th || d > best) continue;
        const float x2 = T.x2[idx2], y2 = T.y2[idx2], sg2 = T.sigma2_2[idx2];
        if (!stereo1 && !stereo2) {
            const float dex = T.ex - x2, dey = T.ey - y2;
            if (dex * dex + dey * dey < 100.0f * sqrtf(sg2)) continue;  // too close to the epipole (:741-748)
        }
        const float num = la * x2 + lb * y2 + lc;
        const float dsqr = num * num / den;
        if (!(dsqr < 3.84f * sg2)) continue;  // CheckDistEpipolarLine (:172-181)
        best = d;
        best_idx = idx2;
    }
    return best_idx;
}

// the row of the slot's kind and width (the dispatch of k_match_tri)
__device__ __forceinline__ int tri_row_any(const DevTriJob &T, int idx1) {
    return T.m.fdim ? tri_row<0>(T, idx1) : (T.m.words == 8 ? tri_row<8>(T, idx1) : tri_row<16>(T, idx1));
}
