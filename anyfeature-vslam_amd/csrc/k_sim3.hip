// k_sim3.hip — Sim3Solver (src/Sim3Solver.cc:38-411) over slots of the keyframe table and ids of the map-point store: the constructor
// and ALL RANSAC hypotheses of every candidate of a loop check (include/afv_hip.h, "Sim3Solver"; host side: afv_sim3.hip).
//
//   k_sim3_gather      one workgroup per candidate.  Filters i1 = 0 .. n1 - 1 (mp2 >= 0, mp1 >= 0, neither point bad in the store,
//                      idx1 >= 0, idx2 >= 0), compacts the survivors in ascending i1 (ballot + popcount ranks, a workgroup prefix, no
//                      atomics) and writes per survivor mvnIndices1, mvX3Dc1 / mvX3Dc2, their images and the two error bounds; writes N.
//   k_sim3_hypotheses  one wavefront per (candidate, hypothesis h): the three draws from the device-side N, Horn's closed form on them
//                      (lane-uniform), T12 and T21, then the lanes stride over the N correspondences: a ballot is a 64-bit inlier word, its
//                      popcount the count.  The stream orders it behind the gather: no flag, no spinning.
//
// The arithmetic is the restatement's (tests/_sim3_ref.py), statement for statement: float, one rounding per operator (the build's
// -ffp-contract=off; hipcc's correctly rounded divide and square root), a three-term sum as a0 + (a1 + a2), scalar expressions left to
// right as written, double where the reference accumulates in double (cv::Mat::dot: nom, err1, err2; den).  PARITY UNPINNED.
// Quirks restated as written:
//   Q1  mvnMaxError1/2 are vector<size_t>: the bound is (size_t)(9.210 * sigmaSquare), truncated, and err < bound compares in float
//   Q2  the best hypothesis is updated on mnInliersi >= mnBestInliers, iterate returns on mnInliersi > mRansacMinInliers (host)
//   Q3  SetRansacParameters: epsilon in float, the logarithms in double, max(1, min(nIterations, maxIterations)) (host)
// Deliberate deviations:
//   S1  N is Horn's symmetric matrix: N(3,0..2) = N(0..2,3) as computed at :242, :247, :252 (the reference reads row 3 unwritten)
//   S2  the eigenvector of the largest eigenvalue: cyclic Jacobi on the symmetric 4 x 4 in double, pairs (0,1) (0,2) (0,3) (1,2) (1,3)
//       (2,3), + - * / sqrt only, at most 12 sweeps, a pair skipped when a_pq == 0 or |a_pp| + |a_pq| == |a_pp| and |a_qq| + |a_pq| ==
//       |a_qq|, a sweep without a rotation ends it, ties on the maximum to the lowest index
//   S3  R12 from the normalised quaternion in double, then rounded to float (no atan2, no Rodrigues)
//   S4  draws: key_h = sm(sm(seed) ^ (h + 1)), draw d = sm(key_h + (d + 1) * DRAW_STEP) % (N - d) on vAvailableIndices with swap-with-back
//   S5  degenerate: den (scale estimated), s12i, R12 or t12 not finite, or den == 0: 0 inliers, flagged, record and words 0; an error that
//       is not finite is no inlier; a sigma2 that is negative or not finite gives bound 0
//   S6  N < 3: no hypothesis is evaluated, all counts 0, no flag
#include "afv_device.h"
#include "afv_runtime.h"

#define SIM3_T AFV_SIM3_T
#define SIM3_WAVES (SIM3_T / 64)
#define SIM3_SWEEPS 12

__device__ __forceinline__ float s3_sum3(float a0, float a1, float a2) { return a0 + (a1 + a2); }
__device__ __forceinline__ float s3_row(const float *R, const float *t, int r, float X, float Y, float Z) {
    return s3_sum3(R[3 * r] * X, R[3 * r + 1] * Y, R[3 * r + 2] * Z) + t[r];
}
__device__ __forceinline__ bool s3_finite(float v) { return fabsf(v) <= 3.402823466e38f; }
__device__ __forceinline__ bool s3_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
// Q1 / S5: (size_t)(9.210 * sigmaSquare) as the float the comparison promotes it to
__device__ __forceinline__ float s3_bound(float sigma2) {
    if (!(sigma2 >= 0.0f) || !s3_finite(sigma2)) return 0.0f;
    return (float)trunc(9.210 * (double)sigma2);
}
__device__ __forceinline__ unsigned long long s3_sm(unsigned long long x) {  // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(SIM3_T) void k_sim3_gather(const DevSim3Args A) {
    __shared__ int s_wave[SIM3_WAVES];
    const int tid = threadIdx.x, c = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const DevSim3Cand &J = A.cands[c];
    const size_t row0 = (size_t)c * A.cap;
    const int n1 = min(J.n1, A.cap);
    int base = 0;
    for (int i0 = 0; i0 < n1; i0 += SIM3_T) {
        const int i1 = i0 + tid;
        int p1 = -1, p2 = -1, k1 = -1, k2 = -1;
        bool keep = false;
        if (i1 < n1) {
            p2 = A.mp2[row0 + i1];
            p1 = A.mp1[row0 + i1];
            k1 = A.idx1 ? A.idx1[row0 + i1] : i1;
            k2 = A.idx2[row0 + i1];
            keep = p2 >= 0 && p2 < A.pcap && p1 >= 0 && p1 < A.pcap && k1 >= 0 && k1 < A.cap && k2 >= 0 && k2 < A.cap;
            if (keep) {
                const unsigned f1 = A.flags[p1], f2 = A.flags[p2];
                keep = (f1 & AFV_PTF_SET) && !(f1 & AFV_PTF_BAD) && (f2 & AFV_PTF_SET) && !(f2 & AFV_PTF_BAD);
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int rank = base + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < SIM3_WAVES; ++w) {
            if (w < wave) rank += s_wave[w];
            total += s_wave[w];
        }
        if (keep) {
            const size_t o = row0 + rank;
            A.index1[o] = i1;
            const float X1 = A.pos[0][p1], Y1 = A.pos[1][p1], Z1 = A.pos[2][p1];
            const float X2 = A.pos[0][p2], Y2 = A.pos[1][p2], Z2 = A.pos[2][p2];
            const float a0 = s3_row(J.R1, J.t1, 0, X1, Y1, Z1), a1 = s3_row(J.R1, J.t1, 1, X1, Y1, Z1), a2 = s3_row(J.R1, J.t1, 2, X1, Y1, Z1);
            const float b0 = s3_row(J.R2, J.t2, 0, X2, Y2, Z2), b1 = s3_row(J.R2, J.t2, 1, X2, Y2, Z2), b2 = s3_row(J.R2, J.t2, 2, X2, Y2, Z2);
            A.x1[3 * o] = a0; A.x1[3 * o + 1] = a1; A.x1[3 * o + 2] = a2;
            A.x2[3 * o] = b0; A.x2[3 * o + 1] = b1; A.x2[3 * o + 2] = b2;
            const float iz1 = 1.0f / a2, iz2 = 1.0f / b2;  // FromCameraToImage
            A.im1[2 * o] = J.fx1 * (a0 * iz1) + J.cx1; A.im1[2 * o + 1] = J.fy1 * (a1 * iz1) + J.cy1;
            A.im2[2 * o] = J.fx2 * (b0 * iz2) + J.cx2; A.im2[2 * o + 1] = J.fy2 * (b1 * iz2) + J.cy2;
            A.max_err[2 * o] = s3_bound(J.sigma2_1[k1]);
            A.max_err[2 * o + 1] = s3_bound(J.sigma2_2[k2]);
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) A.n[c] = base;
    for (int k = base + tid; k < A.cap; k += SIM3_T) {  // what the outputs read from N on
        const size_t o = row0 + k;
        A.index1[o] = -1;
        A.x1[3 * o] = 0.0f; A.x1[3 * o + 1] = 0.0f; A.x1[3 * o + 2] = 0.0f;
        A.x2[3 * o] = 0.0f; A.x2[3 * o + 1] = 0.0f; A.x2[3 * o + 2] = 0.0f;
        A.max_err[2 * o] = 0.0f; A.max_err[2 * o + 1] = 0.0f;
    }
}

// S2: one rotation of the pair (P, Q), compile-time indices: everything stays in registers
template <int P, int Q>
__device__ __forceinline__ bool s3_rotate(double (&a)[4][4], double (&v)[4][4]) {
    const double apq = a[P][Q], app = a[P][P], aqq = a[Q][Q];
    if (apq == 0.0) return false;
    const double g = fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == P || k == Q) continue;
        const double akp = a[k][P], akq = a[k][Q];
        const double np = c * akp - s * akq, nq = s * akp + c * akq;
        a[k][P] = np; a[P][k] = np;
        a[k][Q] = nq; a[Q][k] = nq;
    }
    a[P][P] = app - t * apq;
    a[Q][Q] = aqq + t * apq;
    a[P][Q] = 0.0; a[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
    return true;
}

// ComputeCentroid (:212-218): P[r][i] = component r of point i
__device__ __forceinline__ void s3_centroid(const float (&P)[3][3], float (&Pr)[3][3], float (&C)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        C[r] = s3_sum3(P[r][0], P[r][1], P[r][2]) / 3.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) Pr[r][i] = P[r][i] - C[r];
    }
}

// ComputeSim3 (:220-325) on the sample: R (R12i), t (t12i), s (s12i), Rt21 / t21 (T21i's blocks).  false: degenerate (S5)
__device__ __forceinline__ bool s3_solve(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, float (&R)[9], float (&t)[3], float &s,
                                         float (&sR)[9], float (&sRi)[9], float (&ti)[3]) {
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3], M[3][3];
    s3_centroid(P1, Pr1, O1);
    s3_centroid(P2, Pr2, O2);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] = s3_sum3(Pr2[r][0] * Pr1[c][0], Pr2[r][1] * Pr1[c][1], Pr2[r][2] * Pr1[c][2]);
    double a[4][4], v[4][4];
    {
        const float n00 = M[0][0] + M[1][1] + M[2][2], n01 = M[1][2] - M[2][1], n02 = M[2][0] - M[0][2], n03 = M[0][1] - M[1][0];
        const float n11 = M[0][0] - M[1][1] - M[2][2], n12 = M[0][1] + M[1][0], n13 = M[2][0] + M[0][2];
        const float n22 = -M[0][0] + M[1][1] - M[2][2], n23 = M[1][2] + M[2][1];
        const float n33 = -M[0][0] - M[1][1] + M[2][2];
        a[0][0] = n00; a[0][1] = n01; a[0][2] = n02; a[0][3] = n03;
        a[1][0] = n01; a[1][1] = n11; a[1][2] = n12; a[1][3] = n13;
        a[2][0] = n02; a[2][1] = n12; a[2][2] = n22; a[2][3] = n23;
        a[3][0] = n03; a[3][1] = n13; a[3][2] = n23; a[3][3] = n33;  // S1
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SIM3_SWEEPS; ++sweep) {
        bool any = s3_rotate<0, 1>(a, v);
        any |= s3_rotate<0, 2>(a, v);
        any |= s3_rotate<0, 3>(a, v);
        any |= s3_rotate<1, 2>(a, v);
        any |= s3_rotate<1, 3>(a, v);
        any |= s3_rotate<2, 3>(a, v);
        if (!any) break;
    }
    double best = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];
    if (a[1][1] > best) { best = a[1][1]; q0 = v[0][1]; q1 = v[1][1]; q2 = v[2][1]; q3 = v[3][1]; }
    if (a[2][2] > best) { best = a[2][2]; q0 = v[0][2]; q1 = v[1][2]; q2 = v[2][2]; q3 = v[3][2]; }
    if (a[3][3] > best) { best = a[3][3]; q0 = v[0][3]; q1 = v[1][3]; q2 = v[2][3]; q3 = v[3][3]; }
    {   // S3
        const double nrm = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
        const double w = q0 / nrm, x = q1 / nrm, y = q2 / nrm, z = q3 / nrm;
        R[0] = (float)(1.0 - 2.0 * (y * y + z * z)); R[1] = (float)(2.0 * (x * y - w * z)); R[2] = (float)(2.0 * (x * z + w * y));
        R[3] = (float)(2.0 * (x * y + w * z)); R[4] = (float)(1.0 - 2.0 * (x * x + z * z)); R[5] = (float)(2.0 * (y * z - w * x));
        R[6] = (float)(2.0 * (x * z - w * y)); R[7] = (float)(2.0 * (y * z + w * x)); R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && s3_finite(R[k]);
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p3 = s3_sum3(R[3 * r] * Pr2[0][c], R[3 * r + 1] * Pr2[1][c], R[3 * r + 2] * Pr2[2][c]);  // P3 = R12i * Pr2
                nom = nom + (double)Pr1[r][c] * (double)p3;
                const float sq = p3 * p3;
                den = den + (double)sq;
            }
        ok = ok && s3_finite(den) && den != 0.0;
        s = (float)(nom / den);
    } else {
        s = 1.0f;
    }
    ok = ok && s3_finite(s);
    const float inv_s = 1.0f / s;
#pragma unroll
    for (int k = 0; k < 9; ++k) sR[k] = s * R[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        t[r] = O1[r] - s3_sum3(sR[3 * r] * O2[0], sR[3 * r + 1] * O2[1], sR[3 * r + 2] * O2[2]);
        ok = ok && s3_finite(t[r]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) sRi[3 * r + c] = inv_s * R[3 * c + r];
#pragma unroll
    for (int r = 0; r < 3; ++r) ti[r] = s3_sum3(-sRi[3 * r] * t[0], -sRi[3 * r + 1] * t[1], -sRi[3 * r + 2] * t[2]);
    return ok;
}

// Project (:370-391) of one point and the squared distance to `im` as cv::Mat::dot gives it: products and sum in double, then float
__device__ __forceinline__ float s3_err(const float *R, const float *t, float fx, float fy, float cx, float cy, const float *X, const float *im,
                                        bool first_minus_projected) {
    const float x = s3_row(R, t, 0, X[0], X[1], X[2]), y = s3_row(R, t, 1, X[0], X[1], X[2]), z = s3_row(R, t, 2, X[0], X[1], X[2]);
    const float invz = 1.0f / z;
    const float u = fx * (x * invz) + cx, v = fy * (y * invz) + cy;
    const float d0 = first_minus_projected ? im[0] - u : u - im[0], d1 = first_minus_projected ? im[1] - v : v - im[1];
    return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}

__global__ __launch_bounds__(SIM3_T) void k_sim3_hypotheses(const DevSim3Args A) {
    const int lane = threadIdx.x & 63, c = blockIdx.y;
    const int h = blockIdx.x * SIM3_WAVES + (threadIdx.x >> 6);  // wave-uniform
    if (h >= A.nhyp) return;
    const DevSim3Cand &J = A.cands[c];
    const size_t row0 = (size_t)c * A.cap, ho = (size_t)c * A.nhyp + h;
    const int N = min(A.n[c], A.cap);
    const int pairs = (A.mask_words + 1) >> 1;
    uint32_t *words = A.inliers + ho * A.mask_words;
    float *rec = A.sim3 + ho * 13;
    bool ok = N >= 3;  // S6
    float R[9], t[3], s = 0.0f, sR[9], sRi[9], ti[3];
    if (ok) {
        // S4: the three draws on vAvailableIndices with swap-with-back, without the list
        const unsigned long long key = s3_sm(s3_sm(J.seed) ^ (unsigned long long)(h + 1));
        const unsigned long long step = 0xD1342543DE82EF95ull;
        const int r0 = (int)(s3_sm(key + step) % (unsigned long long)N);
        const int r1 = (int)(s3_sm(key + 2ull * step) % (unsigned long long)(N - 1));
        const int r2 = (int)(s3_sm(key + 3ull * step) % (unsigned long long)(N - 2));
        const int i0 = r0;
        const int i1 = r1 == r0 ? N - 1 : r1;
        const int back1 = N - 2 == r0 ? N - 1 : N - 2;  // what position N - 2 holds when draw 1 removes its pick
        const int i2 = r2 == r1 ? back1 : (r2 == r0 ? N - 1 : r2);
        const int idx[3] = {i0, i1, i2};
        float P1[3][3], P2[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                P1[r][i] = A.x1[3 * (row0 + idx[i]) + r];
                P2[r][i] = A.x2[3 * (row0 + idx[i]) + r];
            }
        ok = s3_solve(P1, P2, J.fix_scale != 0, R, t, s, sR, sRi, ti);
    }
    if (lane == 0) A.degenerate[ho] = (N >= 3 && !ok) ? 1 : 0;
    if (lane < 13) {
        float val = 0.0f;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (lane == k) val = R[k];
            if (lane == 9) val = t[0];
            if (lane == 10) val = t[1];
            if (lane == 11) val = t[2];
            if (lane == 12) val = s;
        }
        rec[lane] = val;
    }
    int count = 0;
    for (int j = 0; j < pairs; ++j) {
        const int k = j * 64 + lane;
        bool in = false;
        if (ok && k < N) {
            const size_t o = row0 + k;
            const float e1 = s3_err(sR, t, J.fx1, J.fy1, J.cx1, J.cy1, A.x2 + 3 * o, A.im1 + 2 * o, true);    // mvP1im1 - vP2im1
            const float e2 = s3_err(sRi, ti, J.fx2, J.fy2, J.cx2, J.cy2, A.x1 + 3 * o, A.im2 + 2 * o, false); // vP1im2 - mvP2im2
            in = e1 < A.max_err[2 * o] && e2 < A.max_err[2 * o + 1];
        }
        const unsigned long long m = __ballot(in);
        count += __popcll(m);
        if (lane == 0) words[2 * j] = (uint32_t)m;
        if (lane == 1 && 2 * j + 1 < A.mask_words) words[2 * j + 1] = (uint32_t)(m >> 32);
    }
    if (lane == 0) A.count[ho] = count;
}

extern "C" void afv_launch_sim3_gather(const DevSim3Args *args, hipStream_t stream) {
    hipLaunchKernelGGL(k_sim3_gather, dim3(args->nc), dim3(SIM3_T), 0, stream, *args);
}

extern "C" void afv_launch_sim3_hypotheses(const DevSim3Args *args, hipStream_t stream) {
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3((args->nhyp + SIM3_WAVES - 1) / SIM3_WAVES, args->nc), dim3(SIM3_T), 0, stream, *args);
}
