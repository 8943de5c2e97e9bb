// k_poseopt.hip — Optimizer::PoseOptimization (src/Optimizer.cc:245-448) for a resident frame (include/afv_hip.h, "pose optimisation";
// host side: afv_poseopt.hip).
//
//   k_pose_optimize<K>  one 1024-thread workgroup per job, one launch per call: the four rounds, the Levenberg iterations and trials, the
//                       6 x 6 solve and the classification all run inside the kernel.  K = P / 1024 features per thread (P = the smallest
//                       power of two >= max(N, 1024)): thread t owns the features t + 1024 p, p < K, and keeps each one's Xw (gathered from the
//                       store by id), observation, information and flags in registers across the whole call.
//
// g2o is an empty directory in the reference: the arithmetic follows upstream g2o as bundled with ORB-SLAM2 (EdgeSE3ProjectXYZOnlyPose /
// EdgeStereoSE3ProjectXYZOnlyPose::computeError and linearizeOplus, RobustKernelHuber::robustify, BaseUnaryEdge::constructQuadraticForm,
// OptimizationAlgorithmLevenberg::solve, SparseOptimizer::optimize) - parity unpinned.  The normative semantics are tests/_poseopt_ref.py,
// statement for statement: double, one rounding per operator (the build's -ffp-contract=off; correctly rounded divide and square root),
// three-term sums as a0 + (a1 + a2).  Deliberate deviations from upstream:
//   (P1) every edge is classified at the round's final ACCEPTED pose (upstream leaves an inlier edge with the error of the last trial,
//        rejected or not, when the call ends on a rejection).
//   (P2) a chi2 that is not finite is an outlier (upstream: NaN > th is false).
//   (P3) the state is R (3 x 3) and t in double; a step is R <- dR R, t <- dR t + V upsilon, no quaternion in between.
//   (P4) the three coefficients of the exponential map are 16-term Horner polynomials in theta^2 (the tables below are the restatement's,
//        digit for digit); no library sin / cos on either side; a step with theta^2 > pi^2 is a failed trial.  Accuracy: (1 - cos)/theta^2 and
//        (theta - sin)/theta^3 within 4 ulp of their values over [0, pi]; sin/theta within 4 ulp of its value up to theta = 2 and within
//        2^-52 absolute beyond (29 ulp of its value at 3.0, no relative accuracy at pi, where it crosses zero).
//   (P5) every sum over the edges (21 + 6 + 1 values per linearisation, 1 per trial) is a perfect binary tree over the feature index with P
//        leaves; a feature that is no active edge is +0.0 and every leaf is its value + 0.0, so no leaf is -0.0 and the zero leaves up to
//        1024 K are exactly neutral.  The 6 x 6 solve is an unpivoted L L^T in a fixed loop order; a pivot that is not positive and finite
//        is a failed trial.  A round with no active edge leaves the pose as it is.
// A failed trial is a rejected one whatever rho would have been.
//
// The tree: the wavefront w of pass p holds the features 1024 p + 64 w .. + 63, one per lane - a subtree of 64 leaves, summed by an xor
// butterfly (DPP inside the rows of 16 lanes, two ds_bpermute steps across them: a 64-bit value moves as two dwords); the 16 K wavefront
// results go through LDS, where rows of 16 lanes sum them in the same way, and every thread adds the last K values itself.
#include "afv_device.h"
#include "afv_runtime.h"
#include "afv_wave.h"

#define PO_T 1024
#define PO_NV 28            // 21 (upper triangle of H) + 6 (b) + 1 (the robust chi2)
#define DPP_ROW_MIRROR 0x140

#define PO_EDGE 1u
#define PO_STEREO 2u
#define PO_FLAGGED 4u

__device__ static const double PO_EXP_A[16] = {0x1.0000000000000p+0, -0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19,
                                               -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49, -0x1.2f49b46814157p-57,
                                               0x1.71b8ef6dcf572p-66, -0x1.761b41316381ap-75, 0x1.3f3ccdd165fa9p-84, -0x1.d1ab1c2dccea3p-94, 0x1.259f98b4358adp-103,
                                               -0x1.434d2e783f5bcp-113};
__device__ static const double PO_EXP_B[16] = {0x1.0000000000000p-1, -0x1.5555555555555p-5, 0x1.6c16c16c16c17p-10, -0x1.a01a01a01a01ap-16, 0x1.27e4fb7789f5cp-22,
                                               -0x1.1eed8eff8d898p-29, 0x1.93974a8c07c9dp-37, -0x1.ae7f3e733b81fp-45, 0x1.6827863b97d97p-53, -0x1.e542ba4020225p-62,
                                               0x1.0ce396db7f853p-70, -0x1.f2cf01972f578p-80, 0x1.88e85fc6a4e5ap-89, -0x1.0a18a2635085dp-98, 0x1.3932c5047d60ep-108,
                                               -0x1.434d2e783f5bcp-118};
__device__ static const double PO_EXP_C[16] = {0x1.5555555555555p-3, -0x1.1111111111111p-7, 0x1.a01a01a01a01ap-13, -0x1.71de3a556c734p-19, 0x1.ae64567f544e4p-26,
                                               -0x1.6124613a86d09p-33, 0x1.ae7f3e733b81fp-41, -0x1.952c77030ad4ap-49, 0x1.2f49b46814157p-57, -0x1.71b8ef6dcf572p-66,
                                               0x1.761b41316381ap-75, -0x1.3f3ccdd165fa9p-84, 0x1.d1ab1c2dccea3p-94, -0x1.259f98b4358adp-103, 0x1.434d2e783f5bcp-113,
                                               -0x1.3981254dd0d52p-123};
#define PO_PI2 0x1.3bd3cc9be45dep+3          // (double)pi * (double)pi
#define PO_DELTA_MONO 0x1.394ca80000000p+1    // (double)sqrtf(5.991f)
#define PO_DELTA_STEREO 0x1.65d4000000000p+1  // (double)sqrtf(7.815f)
#define PO_TH_MONO 5.991f
#define PO_TH_STEREO 7.815f
#define PO_DBL_MAX 0x1.fffffffffffffp+1023

__device__ __forceinline__ double po_horner(const double *c, double t2) {
    double r = c[15];
#pragma unroll
    for (int k = 14; k >= 0; --k) r = r * t2 + c[k];
    return r;
}

// ---- the tree ----
#define PO_DPP64(v, ctrl) \
    __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xf, 0xf, true), __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xf, 0xf, true))
// 16 values, one per lane of a row: every lane of the row receives the tree sum.  After the two quad steps the four lanes of a quad agree,
// so the mirrors (lane i <- lane 7 - i, lane i <- lane 15 - i) hand over exactly what xor 4 / xor 8 would
__device__ __forceinline__ double po_row_tree(double v) {
    v = v + PO_DPP64(v, DPP_QUAD_XOR1);
    v = v + PO_DPP64(v, DPP_QUAD_XOR2);
    v = v + PO_DPP64(v, DPP_ROW_HALF_MIRROR);
    v = v + PO_DPP64(v, DPP_ROW_MIRROR);
    return v;
}
__device__ __forceinline__ double po_wave_tree(double v) {
    v = po_row_tree(v);
    v = v + __shfl_xor(v, 16);
    v = v + __shfl_xor(v, 32);
    return v;
}

// the sums of NV values over all features, in two parts.  po_tree_put: this thread's leaves of pass p (one call per pass, so no more than
// NV leaves are alive whatever K is); po_tree_sum: every thread receives tot[0 .. NV).  Two barriers per sum: the next sum's writes to
// s_part come after the second, its writes to s_mid after its own first
template <int K, int NV>
__device__ __forceinline__ void po_tree_put(int p, const double (&leaf)[NV], double *s_part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const double r = po_wave_tree(leaf[v] + 0.0);
        if (lane == 0) s_part[(v * K + p) * 16 + wave] = r;
    }
}
template <int K, int NV>
__device__ __forceinline__ void po_tree_sum(double (&tot)[NV], const double *s_part, double *s_mid) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < NV * K * 16; idx += PO_T) {  // (whole rows of 16 lanes take part or none)
        const double r = po_row_tree(s_part[idx]);
        if ((idx & 15) == 0) s_mid[idx >> 4] = r;
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double q[K];
#pragma unroll
        for (int p = 0; p < K; ++p) q[p] = s_mid[v * K + p];
#pragma unroll
        for (int w = 1; w < K; w *= 2)
#pragma unroll
            for (int p = 0; p < K; p += 2 * w) q[p] = q[p] + q[p + w];
        tot[v] = q[0];
    }
}
// one value per feature
template <int K>
__device__ __forceinline__ double po_tree_sum1(const double (&leaf)[K], double *s_part, double *s_mid) {
#pragma unroll
    for (int p = 0; p < K; ++p) {
        const double l1[1] = {leaf[p]};
        po_tree_put<K, 1>(p, l1, s_part);
    }
    double tot[1];
    po_tree_sum<K, 1>(tot, s_part, s_mid);
    return tot[0];
}

// ---- an edge ----
struct PoEdge {
    float X, Y, Z, ox, oy, our, inf;
    unsigned fl;
};
struct PoCam {
    double fx, fy, cx, cy, bf;
};

// computeError + BaseEdge::chi2: e (e2 = +0.0 on a mono edge) and chi2 at the pose (R, t); x, y, z: the point in the camera
__device__ __forceinline__ double po_error(const PoEdge &E, const PoCam &C, const double *R, const double *t, double &x, double &y, double &z, double &e0,
                                           double &e1, double &e2) {
    const double X = E.X, Y = E.Y, Z = E.Z, inf = E.inf;
    const bool stereo = E.fl & PO_STEREO;
    x = (R[0] * X + (R[1] * Y + R[2] * Z)) + t[0];
    y = (R[3] * X + (R[4] * Y + R[5] * Z)) + t[1];
    z = (R[6] * X + (R[7] * Y + R[8] * Z)) + t[2];
    const double px = C.fx * (x / z) + C.cx;
    const double py = C.fy * (y / z) + C.cy;
    e0 = (double)E.ox - px;
    e1 = (double)E.oy - py;
    e2 = stereo ? (double)E.our - (px - C.bf / z) : 0.0;
    const double c2 = stereo ? e2 * (inf * e2) : 0.0;
    return e0 * (inf * e0) + (e1 * (inf * e1) + c2);
}

// RobustKernelHuber::robustify: rho[0] (returned) and rho[1]
__device__ __forceinline__ double po_huber(double chi2, bool stereo, bool robust, double &rho1) {
    if (!robust) {
        rho1 = 1.0;
        return chi2;
    }
    const double delta = stereo ? PO_DELTA_STEREO : PO_DELTA_MONO;
    const double dsqr = delta * delta;
    const double s = __builtin_sqrt(chi2);
    const bool inl = chi2 <= dsqr;
    rho1 = inl ? 1.0 : delta / s;
    return inl ? chi2 : (2.0 * s) * delta - dsqr;
}

__device__ __forceinline__ double po_robust_chi2(const PoEdge &E, const PoCam &C, const double *R, const double *t, bool robust) {
    double x, y, z, e0, e1, e2, rho1;
    const double chi2 = po_error(E, C, R, t, x, y, z, e0, e1, e2);
    return po_huber(chi2, E.fl & PO_STEREO, robust, rho1);
}

// linearizeOplus + constructQuadraticForm of one edge: out[0 .. 21) the upper triangle of J^T (w I) J row by row, [21 .. 27) J^T g, [27] rho[0]
__device__ __forceinline__ void po_linearise(const PoEdge &E, const PoCam &C, const double *R, const double *t, bool robust, double (&out)[PO_NV]) {
    double x, y, z, e[3], rho1;
    const bool stereo = E.fl & PO_STEREO;
    const double chi2 = po_error(E, C, R, t, x, y, z, e[0], e[1], e[2]);
    out[27] = po_huber(chi2, stereo, robust, rho1);
    const double inf = E.inf;
    const double invz = 1.0 / z, invz2 = invz * invz, fx = C.fx, fy = C.fy, bf = C.bf;
    double J[3][6];
    J[0][0] = ((x * y) * invz2) * fx;
    J[0][1] = -((1.0 + (x * x) * invz2) * fx);
    J[0][2] = (y * invz) * fx;
    J[0][3] = -(invz * fx);
    J[0][4] = 0.0;
    J[0][5] = (x * invz2) * fx;
    J[1][0] = (1.0 + (y * y) * invz2) * fy;
    J[1][1] = -(((x * y) * invz2) * fy);
    J[1][2] = -((x * invz) * fy);
    J[1][3] = 0.0;
    J[1][4] = -(invz * fy);
    J[1][5] = (y * invz2) * fy;
    J[2][0] = J[0][0] - (bf * y) * invz2;
    J[2][1] = J[0][1] + (bf * x) * invz2;
    J[2][2] = J[0][2];
    J[2][3] = J[0][3];
    J[2][4] = 0.0;
    J[2][5] = J[0][5] - bf * invz2;
    const double w = robust ? rho1 * inf : inf;  // robustInformation: rho[1] * Omega
    double g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[k] = -(inf * e[k]);                    // -Omega e
        if (robust) g[k] = rho1 * g[k];
    }
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double a2 = stereo ? J[2][i] * (w * J[2][j]) : 0.0;
            out[o++] = J[0][i] * (w * J[0][j]) + (J[1][i] * (w * J[1][j]) + a2);
        }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double a2 = stereo ? J[2][j] * g[2] : 0.0;
        out[21 + j] = J[0][j] * g[0] + (J[1][j] * g[1] + a2);
    }
}

__device__ __forceinline__ constexpr int po_h(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }  // (i <= j) in the packed upper triangle

// (H + lam I) x = b, unpivoted L L^T in the restatement's loop order; false: a pivot is not positive and finite
__device__ __forceinline__ bool po_solve6(const double (&S)[PO_NV], double lam, double (&x)[6]) {
    double L[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = S[po_h(j, j)] + lam;
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0 && __builtin_isfinite(s))) ok = false;
        L[j][j] = __builtin_sqrt(s);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double q = S[po_h(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) q = q - L[i][k] * L[j][k];
            L[i][j] = q / L[j][j];
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = S[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return ok;  // (a failed pivot makes what follows it garbage that nobody reads)
}

// SE3Quat::exp(x) * (R, t) (P3, P4); false: theta^2 > pi^2
__device__ __forceinline__ bool po_exp_step(const double *R, const double *t, const double (&x)[6], double *Rn, double *tn) {
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double t2 = w0 * w0 + (w1 * w1 + w2 * w2);
    const double A = po_horner(PO_EXP_A, t2), B = po_horner(PO_EXP_B, t2), Cc = po_horner(PO_EXP_C, t2);
    const double W[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    const double W2[3][3] = {{-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2}, {w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2}, {w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)}};
    double dR[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dR[i][j] = i == j ? 1.0 + B * W2[i][j] : A * W[i][j] + B * W2[i][j];
            V[i][j] = i == j ? 1.0 + Cc * W2[i][j] : B * W[i][j] + Cc * W2[i][j];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = dR[i][0] * R[j] + (dR[i][1] * R[3 + j] + dR[i][2] * R[6 + j]);
        tn[i] = (dR[i][0] * t[0] + (dR[i][1] * t[1] + dR[i][2] * t[2])) + (V[i][0] * x[3] + (V[i][1] * x[4] + V[i][2] * x[5]));
    }
    return !(t2 > PO_PI2);
}

__device__ __forceinline__ bool po_uniform(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }  // every thread computed the same value

template <int K>
__global__ __launch_bounds__(PO_T) void k_pose_optimize(const DevPoseArgs A) {
    __shared__ double s_part[PO_NV * K * 16];
    __shared__ double s_mid[PO_NV * K];
    const int tid = threadIdx.x, job = blockIdx.x;
    const int *pts = A.pts + (size_t)job * A.n;
    const float *pose0 = A.poses + (size_t)job * 12;
    const PoCam C = {(double)A.fx, (double)A.fy, (double)A.cx, (double)A.cy, (double)A.bf};

    PoEdge E[K];
#pragma unroll
    for (int p = 0; p < K; ++p) {
        const int i = p * PO_T + tid;
        PoEdge e = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u};
        if (i < A.n) {
            const int id = pts[i];
            if (id >= 0 && id < A.cap && (A.flags[id] & AFV_PTF_SET)) {  // isBad is not consulted (Optimizer.cc:282)
                e.X = A.pos[0][id]; e.Y = A.pos[1][id]; e.Z = A.pos[2][id];
                e.ox = A.x[i]; e.oy = A.y[i]; e.our = A.ur[i]; e.inf = A.inf[i];
                e.fl = PO_EDGE | (e.our < 0.0f ? 0u : PO_STEREO);          // mvuRight[i] < 0: mono (:285)
            }
        }
        E[p] = e;
    }

    double one[K];
#pragma unroll
    for (int p = 0; p < K; ++p) one[p] = (E[p].fl & PO_EDGE) ? 1.0 : 0.0;
    const int n_edges = (int)po_tree_sum1<K>(one, s_part, s_mid);

    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (double)pose0[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (double)pose0[9 + k];
    int rounds = 0, n_bad = 0;
    DevPoseOut *out = A.out + job;

    if (po_uniform(n_edges >= 3)) {
        for (int r = 0; r < 4; ++r) {
            const bool robust = r < 3;  // the kernel is removed after the classification of round 2 (:405-406)
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = (double)pose0[k];  // every round starts from the frame's pose (:375)
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = (double)pose0[9 + k];
#pragma unroll
            for (int p = 0; p < K; ++p) one[p] = (E[p].fl & (PO_EDGE | PO_FLAGGED)) == PO_EDGE ? 1.0 : 0.0;
            const double n_active = po_tree_sum1<K>(one, s_part, s_mid);
            int iterations = 0, trials = 0;
            double cur = 0.0, lam = 0.0, ni = 2.0;
            if (po_uniform(n_active > 0.0)) {
                for (int it = 0; it < 10; ++it) {
                    double tot[PO_NV];
#pragma unroll
                    for (int p = 0; p < K; ++p) {
                        double leaf[PO_NV];
                        po_linearise(E[p], C, R, t, robust, leaf);
                        if ((E[p].fl & (PO_EDGE | PO_FLAGGED)) != PO_EDGE)
#pragma unroll
                            for (int v = 0; v < PO_NV; ++v) leaf[v] = 0.0;
                        po_tree_put<K, PO_NV>(p, leaf, s_part);
                    }
                    po_tree_sum<K, PO_NV>(tot, s_part, s_mid);
                    cur = tot[27];
                    if (it == 0) {  // computeLambdaInit: tau * max |H_jj|
                        double m = __builtin_fabs(tot[po_h(0, 0)]);
#pragma unroll
                        for (int j = 1; j < 6; ++j) {
                            const double a = __builtin_fabs(tot[po_h(j, j)]);
                            m = a > m ? a : m;
                        }
                        lam = 1e-5 * m;
                        ni = 2.0;
                    }
                    ++iterations;
                    double rho = 0.0;
                    int qmax = 0;
                    do {
                        ++trials;
                        double x[6], Rn[9], tn[3];
                        bool ok = po_solve6(tot, lam, x);
                        if (po_uniform(ok)) ok = po_exp_step(R, t, x, Rn, tn);
                        bool accepted = false;
                        double temp = PO_DBL_MAX;
                        if (po_uniform(ok)) {
                            double tl[K];
#pragma unroll
                            for (int p = 0; p < K; ++p)
                                tl[p] = (E[p].fl & (PO_EDGE | PO_FLAGGED)) == PO_EDGE ? po_robust_chi2(E[p], C, Rn, tn, robust) : 0.0;
                            temp = po_tree_sum1<K>(tl, s_part, s_mid);
                            double scale = 0.0;
#pragma unroll
                            for (int j = 0; j < 6; ++j) scale = scale + x[j] * (lam * x[j] + tot[21 + j]);  // computeScale
                            scale = scale + 1e-3;
                            rho = (cur - temp) / scale;
                            accepted = rho > 0.0 && __builtin_isfinite(temp);
                        } else {
                            rho = -1.0;
                        }
                        if (po_uniform(accepted)) {
                            const double q = 2.0 * rho - 1.0;
                            double alpha = 1.0 - (q * q) * q;
                            const double up = 2.0 / 3.0, low = 1.0 / 3.0;
                            alpha = up < alpha ? up : alpha;
                            const double factor = low < alpha ? alpha : low;
                            lam = lam * factor;
                            ni = 2.0;
                            cur = temp;
#pragma unroll
                            for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
                            for (int k = 0; k < 3; ++k) t[k] = tn[k];
                        } else {
                            lam = lam * ni;
                            ni = ni * 2.0;
                        }
                        ++qmax;
                        if (!po_uniform(rho < 0.0 && qmax < 10)) break;
                    } while (true);
                    if (po_uniform(qmax == 10 || rho == 0.0)) break;
                }
            }
            // classification of every edge at the round's final accepted pose (P1, P2; :386-403)
#pragma unroll
            for (int p = 0; p < K; ++p) {
                double x, y, z, e0, e1, e2;
                const double chi2 = po_error(E[p], C, R, t, x, y, z, e0, e1, e2);
                const float th = (E[p].fl & PO_STEREO) ? PO_TH_STEREO : PO_TH_MONO;
                const bool bad = (E[p].fl & PO_EDGE) && (!__builtin_isfinite(chi2) || (float)chi2 > th);
                E[p].fl = (E[p].fl & ~PO_FLAGGED) | (bad ? PO_FLAGGED : 0u);
                one[p] = bad ? 1.0 : 0.0;
            }
            n_bad = (int)po_tree_sum1<K>(one, s_part, s_mid);
            if (tid == 0) {
                out->iterations[r] = iterations;
                out->trials[r] = trials;
                out->chi2[r] = cur;
                out->lambda[r] = lam;
            }
            rounds = r + 1;
            if (po_uniform(n_edges < 10)) break;  // optimizer.edges().size() < 10 (:438)
        }
    }
    if (tid == 0) {
        for (int r = rounds; r < 4; ++r) {
            out->iterations[r] = 0;
            out->trials[r] = 0;
            out->chi2[r] = 0.0;
            out->lambda[r] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) out->R[k] = (float)R[k];  // Converter::toMatrix4f
#pragma unroll
        for (int k = 0; k < 3; ++k) out->t[k] = (float)t[k];
        out->n_good = rounds ? n_edges - n_bad : 0;
        out->n_edges = n_edges;
        out->rounds = rounds;
    }
    uint8_t *flagged = A.outlier + (size_t)job * A.n;
#pragma unroll
    for (int p = 0; p < K; ++p) {
        const int i = p * PO_T + tid;
        if (i < A.n) flagged[i] = (E[p].fl & PO_FLAGGED) ? 1 : 0;
    }
}

extern "C" void afv_launch_pose_optimize(const DevPoseArgs *args, int njobs, hipStream_t stream) {
    if (njobs <= 0 || args->n <= 0) return;
    const dim3 grid(njobs), block(PO_T);
    if (args->n <= 1024) hipLaunchKernelGGL(k_pose_optimize<1>, grid, block, 0, stream, *args);
    else if (args->n <= 2048) hipLaunchKernelGGL(k_pose_optimize<2>, grid, block, 0, stream, *args);
    else if (args->n <= 4096) hipLaunchKernelGGL(k_pose_optimize<4>, grid, block, 0, stream, *args);
    else hipLaunchKernelGGL(k_pose_optimize<8>, grid, block, 0, stream, *args);  // (the host refused n > 8192)
}
