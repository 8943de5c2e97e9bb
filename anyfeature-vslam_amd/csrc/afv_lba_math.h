// afv_lba_math.h — the arithmetic of LocalBundleAdjustment / BundleAdjustment as tests/_lba_ref.py fixes it, statement for statement:
// double, one rounding per operator (-ffp-contract=off on every side), three-term sums as a0 + (a1 + a2).  ONE text for the kernels
// (k_lba.hip: every function here is the work of one lane - an edge, a point, or partial sum l of a 64-partial tree) and for the scalar
// host program (tools/lba_host.cpp, which calls the same functions in loops); the halving trees, the dense L L^T and the drivers are
// each side's own.  Deviations L1-L9: include/afv_hip.h.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LB_FN __host__ __device__ __forceinline__
#define LB_UNROLL _Pragma("unroll")
#else
#define LB_FN static inline
#define LB_UNROLL
#endif

#define LB_PI2 0x1.3bd3cc9be45dep+3            // (double)pi * (double)pi
#define LB_TAU 1e-5
#define LB_DBL_MAX 0x1.fffffffffffffp+1023
#define LB_MAX_TRIALS 10
#define LB_TH_MONO 5.991f                      // chi2_2dof / chi2_3dof: floats, promoted where a chi2 is compared
#define LB_TH_STEREO 7.815f
#define LB_NT 55                               // terms of an edge: Al 0..5, gl 6..8, W 9..26, Ap 27..47, gp 48..53, rho0 54
#define LB_DROPPED 0                           // edge states (AFV_LBA_EDGE_*)
#define LB_KEPT 1
#define LB_REMOVED_KEPT 2
#define LB_ERASE 3
#define LB_NEXT_TRIAL 0                        // what the judge tells the driver
#define LB_NEXT_ITERATION 1
#define LB_NEXT_DONE 2

struct LbCam {
    double fx, fy, cx, cy, bf;
};

struct LbStatus {       // the Levenberg state of the running optimize() call; the judge writes it, the driver follows it
    double lam, ni, cur, temp, rho;
    int32_t buf;        // which of the two state buffers holds the accepted estimate
    int32_t it, qmax, iterations, trials, max_it, robust, next, failed, accepted, pad[2];
};

struct LbView {         // the problem: the same arrays on either side
    int nk, nf, np, ne;
    const LbCam *cam;           // [nk]
    const int *e_pt, *e_kf;     // [ne] by point
    const double *e_obs;        // [5][ne]: x, y, u_right, inf, inf3
    const uint8_t *e_stereo;    // [ne]
    uint8_t *e_on;              // [ne] 1: active (level 0)
    uint8_t *e_state;           // [ne]
    double *e_chi2;             // [ne] the chi2 of the first check (L-Q1)
    const int *pt_ptr;          // [np + 1] the edges of point p
    const int *kf_ptr, *kf_edge;  // [nf + 1], [.]: the edges of free keyframe i, ascending
    const uint8_t *p_on;        // [np] 0: dropped
    double *pose;               // [2][nk][12] R row-major, t
    double *xyz;                // [2][np][3]
    double *term;               // [LB_NT][ne]
    double *rho_trial;          // [ne]
    double *Hll;                // [np][9]: upper triangle (00 01 02 11 12 22), bl
    double *Hinv;               // [np][9]: the inverse of Hll + lambda I, z = inverse * bl
    double *Hpp;                // [nf][27]: upper triangle by rows, bp
    double *M;                  // [n][n], n = 6 nf: the reduced system's lower triangle, then L in place
    double *bS, *dx;            // [n]; [n + 3 np]: dxp, dxl
    uint8_t *p_fail, *k_fail;   // [np], [nf]
    int32_t *solve_fail;        // [1]
    LbStatus *st;
};

LB_FN bool lb_finite(double v) { return fabs(v) <= LB_DBL_MAX; }

LB_FN double lb_horner16(const double (&c)[16], double t2) {
    double r = c[15];
LB_UNROLL
    for (int k = 14; k >= 0; --k) r = r * t2 + c[k];
    return r;
}
// L4: PoseOptimization's EXP_A / EXP_B / EXP_C, digit for digit
LB_FN double lb_exp_a(double t2) {
    const double c[16] = {0x1.0000000000000p+0, -0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19,
                          -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49, -0x1.2f49b46814157p-57,
                          0x1.71b8ef6dcf572p-66, -0x1.761b41316381ap-75, 0x1.3f3ccdd165fa9p-84, -0x1.d1ab1c2dccea3p-94, 0x1.259f98b4358adp-103,
                          -0x1.434d2e783f5bcp-113};
    return lb_horner16(c, t2);
}
LB_FN double lb_exp_b(double t2) {
    const double c[16] = {0x1.0000000000000p-1, -0x1.5555555555555p-5, 0x1.6c16c16c16c17p-10, -0x1.a01a01a01a01ap-16, 0x1.27e4fb7789f5cp-22,
                          -0x1.1eed8eff8d898p-29, 0x1.93974a8c07c9dp-37, -0x1.ae7f3e733b81fp-45, 0x1.6827863b97d97p-53, -0x1.e542ba4020225p-62,
                          0x1.0ce396db7f853p-70, -0x1.f2cf01972f578p-80, 0x1.88e85fc6a4e5ap-89, -0x1.0a18a2635085dp-98, 0x1.3932c5047d60ep-108,
                          -0x1.434d2e783f5bcp-118};
    return lb_horner16(c, t2);
}
LB_FN double lb_exp_c(double t2) {
    const double c[16] = {0x1.5555555555555p-3, -0x1.1111111111111p-7, 0x1.a01a01a01a01ap-13, -0x1.71de3a556c734p-19, 0x1.ae64567f544e4p-26,
                          -0x1.6124613a86d09p-33, 0x1.ae7f3e733b81fp-41, -0x1.952c77030ad4ap-49, 0x1.2f49b46814157p-57, -0x1.71b8ef6dcf572p-66,
                          0x1.761b41316381ap-75, -0x1.3f3ccdd165fa9p-84, 0x1.d1ab1c2dccea3p-94, -0x1.259f98b4358adp-103, 0x1.434d2e783f5bcp-113,
                          -0x1.3981254dd0d52p-123};
    return lb_horner16(c, t2);
}

// VertexSE3Expmap::oplusImpl (L3, L4): out = exp(x) * in, x = (omega, upsilon).  false: a failed trial
LB_FN bool lb_exp_step(const double *in, const double *x, double *out) {
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double t2 = w0 * w0 + (w1 * w1 + w2 * w2);
    if (t2 > LB_PI2) return false;
    const double A = lb_exp_a(t2), B = lb_exp_b(t2), Cc = lb_exp_c(t2);
    const double W[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    const double W2[9] = {-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2, w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2, w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)};
    double dR[9], V[9];
LB_UNROLL
    for (int i = 0; i < 3; ++i)
LB_UNROLL
        for (int j = 0; j < 3; ++j) {
            const int k = 3 * i + j;
            dR[k] = i == j ? (1.0 + B * W2[k]) : (A * W[k] + B * W2[k]);
            V[k] = i == j ? (1.0 + Cc * W2[k]) : (B * W[k] + Cc * W2[k]);
        }
LB_UNROLL
    for (int i = 0; i < 3; ++i) {
LB_UNROLL
        for (int j = 0; j < 3; ++j) out[3 * i + j] = dR[3 * i] * in[j] + (dR[3 * i + 1] * in[3 + j] + dR[3 * i + 2] * in[6 + j]);
        out[9 + i] = (dR[3 * i] * in[9] + (dR[3 * i + 1] * in[10] + dR[3 * i + 2] * in[11])) + (V[3 * i] * x[3] + (V[3 * i + 1] * x[4] + V[3 * i + 2] * x[5]));
    }
    return true;
}

// RobustKernelHuber::robustify; without a kernel (chi2, 1)
LB_FN void lb_huber(double chi2, double delta, bool robust, double &rho0, double &rho1) {
    const double dsqr = delta * delta;
    if (!robust || chi2 <= dsqr) {
        rho0 = chi2;
        rho1 = 1.0;
    } else {
        const double s = sqrt(chi2);
        rho0 = (2.0 * s) * delta - dsqr;
        rho1 = delta / s;
    }
}

struct LbEdgeAt {   // an edge at an estimate
    double x, y, z, e[3], chi2;
};
// computeError of both edge types and BaseEdge::chi2; a mono edge's third terms are +0.0
LB_FN void lb_edge_at(const LbView &V, int e, int buf, LbEdgeAt &a) {
    const int k = V.e_kf[e], p = V.e_pt[e];
    const double *T = V.pose + ((size_t)buf * V.nk + k) * 12;
    const double *X = V.xyz + ((size_t)buf * V.np + p) * 3;
    const LbCam K = V.cam[k];
    const size_t ne = (size_t)V.ne;
    const bool stereo = V.e_stereo[e] != 0;
    const double inf = V.e_obs[3 * ne + e], inf3 = V.e_obs[4 * ne + e];
    a.x = (T[0] * X[0] + (T[1] * X[1] + T[2] * X[2])) + T[9];
    a.y = (T[3] * X[0] + (T[4] * X[1] + T[5] * X[2])) + T[10];
    a.z = (T[6] * X[0] + (T[7] * X[1] + T[8] * X[2])) + T[11];
    const double px = K.fx * (a.x / a.z) + K.cx;
    const double py = K.fy * (a.y / a.z) + K.cy;
    a.e[0] = V.e_obs[e] - px;
    a.e[1] = V.e_obs[ne + e] - py;
    a.e[2] = stereo ? V.e_obs[2 * ne + e] - (px - K.bf / a.z) : 0.0;
    const double c2 = stereo ? a.e[2] * (inf3 * a.e[2]) : 0.0;
    a.chi2 = a.e[0] * (inf * a.e[0]) + (a.e[1] * (inf * a.e[1]) + c2);
}
LB_FN double lb_delta(bool stereo) { return stereo ? (double)sqrtf(LB_TH_STEREO) : (double)sqrtf(LB_TH_MONO); }

// the edge's term of the robust chi2 at the estimate in buffer `buf`
LB_FN double lb_edge_rho0(const LbView &V, int e, int buf, bool robust) {
    LbEdgeAt a;
    lb_edge_at(V, e, buf, a);
    double r0, r1;
    lb_huber(a.chi2, lb_delta(V.e_stereo[e] != 0), robust, r0, r1);
    return r0;
}
// L1, L2: chi2 > threshold || !isDepthPositive at the estimate in `buf`; cached: chi2 is the one of the first check (L-Q1), else it is
// evaluated here and returned
LB_FN bool lb_edge_outlier(const LbView &V, int e, int buf, bool cached, double &chi2) {
    LbEdgeAt a;
    lb_edge_at(V, e, buf, a);
    if (!cached) chi2 = a.chi2;
    const double th = V.e_stereo[e] ? (double)LB_TH_STEREO : (double)LB_TH_MONO;
    return !lb_finite(chi2) || chi2 > th || !(a.z > 0.0);
}

LB_FN double lb_w3(bool stereo, double u0, double u1, double u2, double w0, double w2, double v0, double v1, double v2) {
    const double a2 = stereo ? u2 * (w2 * v2) : 0.0;
    return u0 * (w0 * v0) + (u1 * (w0 * v1) + a2);
}
LB_FN double lb_g3(bool stereo, double u0, double u1, double u2, double g0, double g1, double g2) {
    const double a2 = stereo ? u2 * g2 : 0.0;
    return u0 * g0 + (u1 * g1 + a2);
}

// linearizeOplus of both vertices + constructQuadraticForm: the LB_NT terms of edge e at the accepted estimate (a fixed keyframe: no
// Jacobian, its W / Ap / gp are not written and not read)
LB_FN void lb_edge_linearise(const LbView &V, int e) {
    const size_t ne = (size_t)V.ne;
    double *T = V.term + e;
    if (!V.e_on[e]) return;
    const int buf = V.st->buf, k = V.e_kf[e];
    const bool robust = V.st->robust != 0, stereo = V.e_stereo[e] != 0;
    LbEdgeAt a;
    lb_edge_at(V, e, buf, a);
    double rho0, rho1;
    lb_huber(a.chi2, lb_delta(stereo), robust, rho0, rho1);
    T[54 * ne] = rho0;
    const LbCam K = V.cam[k];
    const double *R = V.pose + ((size_t)buf * V.nk + k) * 12;
    const double inf = V.e_obs[3 * ne + e], inf3 = V.e_obs[4 * ne + e];
    const double x = a.x, y = a.y;
    const double invz = 1.0 / a.z;
    const double invz2 = invz * invz;
    const double fx = K.fx, fy = K.fy, bf = K.bf;
    // the point (vertex 0): -1 / z * tmp * R, tmp = [fx 0 -x / z fx; 0 fy -y / z fy]; the stereo row as upstream: row 0 - bf R(2, c) / z^2
    double Jl[3][3];
    const double m = -invz, t02 = -((x * invz) * fx), t12 = -((y * invz) * fy);
LB_UNROLL
    for (int c = 0; c < 3; ++c) {
        Jl[0][c] = m * (fx * R[c] + t02 * R[6 + c]);
        Jl[1][c] = m * (fy * R[3 + c] + t12 * R[6 + c]);
        Jl[2][c] = Jl[0][c] - (bf * R[6 + c]) * invz2;
    }
    const double w0 = robust ? rho1 * inf : inf, w2 = robust ? rho1 * inf3 : inf3;   // robustInformation: rho[1] * Omega
    double g[3] = {-(inf * a.e[0]), -(inf * a.e[1]), -(inf3 * a.e[2])};               // -Omega e
    if (robust) {
LB_UNROLL
        for (int r = 0; r < 3; ++r) g[r] = rho1 * g[r];
    }
    {
        int q = 0;
LB_UNROLL
        for (int c = 0; c < 3; ++c)
LB_UNROLL
            for (int d = c; d < 3; ++d) T[(q++) * ne] = lb_w3(stereo, Jl[0][c], Jl[1][c], Jl[2][c], w0, w2, Jl[0][d], Jl[1][d], Jl[2][d]);
    }
LB_UNROLL
    for (int c = 0; c < 3; ++c) T[(6 + c) * ne] = lb_g3(stereo, Jl[0][c], Jl[1][c], Jl[2][c], g[0], g[1], g[2]);
    if (k >= V.nf) return;
    // the pose (vertex 1), rotation columns first: PoseOptimization's text
    double Jp[3][6];
    Jp[0][0] = ((x * y) * invz2) * fx; Jp[0][1] = -((1.0 + (x * x) * invz2) * fx); Jp[0][2] = (y * invz) * fx;
    Jp[0][3] = -(invz * fx); Jp[0][4] = 0.0; Jp[0][5] = (x * invz2) * fx;
    Jp[1][0] = (1.0 + (y * y) * invz2) * fy; Jp[1][1] = -(((x * y) * invz2) * fy); Jp[1][2] = -((x * invz) * fy);
    Jp[1][3] = 0.0; Jp[1][4] = -(invz * fy); Jp[1][5] = (y * invz2) * fy;
    Jp[2][0] = Jp[0][0] - (bf * y) * invz2; Jp[2][1] = Jp[0][1] + (bf * x) * invz2; Jp[2][2] = Jp[0][2];
    Jp[2][3] = Jp[0][3]; Jp[2][4] = 0.0; Jp[2][5] = Jp[0][5] - bf * invz2;
LB_UNROLL
    for (int i = 0; i < 6; ++i)
LB_UNROLL
        for (int c = 0; c < 3; ++c) T[(9 + 3 * i + c) * ne] = lb_w3(stereo, Jp[0][i], Jp[1][i], Jp[2][i], w0, w2, Jl[0][c], Jl[1][c], Jl[2][c]);
    {
        int q = 27;
LB_UNROLL
        for (int i = 0; i < 6; ++i)
LB_UNROLL
            for (int j = i; j < 6; ++j) T[(q++) * ne] = lb_w3(stereo, Jp[0][i], Jp[1][i], Jp[2][i], w0, w2, Jp[0][j], Jp[1][j], Jp[2][j]);
    }
LB_UNROLL
    for (int i = 0; i < 6; ++i) T[(48 + i) * ne] = lb_g3(stereo, Jp[0][i], Jp[1][i], Jp[2][i], g[0], g[1], g[2]);
}

// L5: Hll and bl of point p over its active edges in list order, one after the other
LB_FN void lb_point_build(const LbView &V, int p) {
    if (!V.p_on[p]) return;
    const size_t ne = (size_t)V.ne;
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = V.pt_ptr[p]; e < V.pt_ptr[p + 1]; ++e) {
        if (!V.e_on[e]) continue;
LB_UNROLL
        for (int q = 0; q < 9; ++q) acc[q] = acc[q] + V.term[q * ne + e];
    }
LB_UNROLL
    for (int q = 0; q < 9; ++q) V.Hll[(size_t)p * 9 + q] = acc[q];
}

// L6: (Hll + lambda I)^-1 by cofactors, z = inverse * bl
LB_FN void lb_point_invert(const LbView &V, int p) {
    if (!V.p_on[p]) return;
    const double *H = V.Hll + (size_t)p * 9;
    const double lam = V.st->lam;
    const double a = H[0] + lam, b = H[1], c = H[2], d = H[3] + lam, e = H[4], f = H[5] + lam;
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d, c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
    const double det = a * c00 + (b * c01 + c * c02);
    const bool bad = det == 0.0 || !lb_finite(det);
    V.p_fail[p] = bad ? 1 : 0;
    const double r = 1.0 / det;
    double *I = V.Hinv + (size_t)p * 9;
    I[0] = c00 * r; I[1] = c01 * r; I[2] = c02 * r; I[3] = c11 * r; I[4] = c12 * r; I[5] = c22 * r;
    I[6] = I[0] * H[6] + (I[1] * H[7] + I[2] * H[8]);
    I[7] = I[1] * H[6] + (I[3] * H[7] + I[4] * H[8]);
    I[8] = I[2] * H[6] + (I[4] * H[7] + I[5] * H[8]);
}

// L5: partial sum l of Hpp (21) and bp (6) of free keyframe i: its active edges at positions l, l + 64, ... of its list
LB_FN void lb_pose_partials(const LbView &V, int i, int l, double (&acc)[27]) {
    const size_t ne = (size_t)V.ne;
LB_UNROLL
    for (int q = 0; q < 27; ++q) acc[q] = 0.0;
    for (int s = V.kf_ptr[i] + l; s < V.kf_ptr[i + 1]; s += 64) {
        const int e = V.kf_edge[s];
        if (!V.e_on[e]) continue;
LB_UNROLL
        for (int q = 0; q < 27; ++q) acc[q] = acc[q] + V.term[(27 + q) * ne + e];
    }
}

// the symmetric inverse as a full 3 x 3
LB_FN void lb_inv_full(const double *I, double (&F)[3][3]) {
    F[0][0] = I[0]; F[0][1] = I[1]; F[0][2] = I[2];
    F[1][0] = I[1]; F[1][1] = I[3]; F[1][2] = I[4];
    F[2][0] = I[2]; F[2][1] = I[4]; F[2][2] = I[5];
}

// L5: partial sum l of the Schur sums of block (i, j >= i): sum over the active edges e of keyframe i whose point has an active edge e'
// to keyframe j of (W_e Hinv) W_e'^T (36 values, row-major); for j == i also (W_e z) in acc[36 .. 41]
LB_FN void lb_schur_partials(const LbView &V, int i, int j, int l, double (&acc)[42]) {
    const size_t ne = (size_t)V.ne;
LB_UNROLL
    for (int q = 0; q < 42; ++q) acc[q] = 0.0;
    for (int s = V.kf_ptr[i] + l; s < V.kf_ptr[i + 1]; s += 64) {
        const int e = V.kf_edge[s];
        if (!V.e_on[e]) continue;
        const int p = V.e_pt[e];
        int e2 = -1;
        if (j == i) {
            e2 = e;
        } else {
            for (int q = V.pt_ptr[p]; q < V.pt_ptr[p + 1]; ++q)
                if (V.e_kf[q] == j && V.e_on[q]) {
                    e2 = q;
                    break;
                }
        }
        if (e2 < 0) continue;
        const double *I = V.Hinv + (size_t)p * 9;
        double F[3][3];
        lb_inv_full(I, F);
LB_UNROLL
        for (int a = 0; a < 6; ++a) {
            const double wa0 = V.term[(9 + 3 * a) * ne + e], wa1 = V.term[(10 + 3 * a) * ne + e], wa2 = V.term[(11 + 3 * a) * ne + e];
            double Y[3];
LB_UNROLL
            for (int c = 0; c < 3; ++c) Y[c] = wa0 * F[0][c] + (wa1 * F[1][c] + wa2 * F[2][c]);
LB_UNROLL
            for (int b = 0; b < 6; ++b) {
                const double v = Y[0] * V.term[(9 + 3 * b) * ne + e2] + (Y[1] * V.term[(10 + 3 * b) * ne + e2] + Y[2] * V.term[(11 + 3 * b) * ne + e2]);
                acc[6 * a + b] = acc[6 * a + b] + v;
            }
            if (j == i) acc[36 + a] = acc[36 + a] + (wa0 * I[6] + (wa1 * I[7] + wa2 * I[8]));
        }
    }
}
// after the tree: S = (Hpp + lambda on the diagonal) - sum into M's lower triangle (element (r, c), r <= c, lies at M[c][r]); bS = bp - sum
LB_FN void lb_schur_store(const LbView &V, int i, int j, const double (&sum)[42]) {
    const int n = 6 * V.nf;
    const double lam = V.st->lam;
    const double *H = V.Hpp + (size_t)i * 27;
    int q = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            if (j == i && b < a) continue;
            double h = 0.0;
            if (j == i) {
                h = H[q++];
                if (a == b) h = h + lam;
            }
            V.M[(size_t)(6 * j + b) * n + (6 * i + a)] = h - sum[6 * a + b];
        }
    if (j == i)
        for (int a = 0; a < 6; ++a) V.bS[6 * i + a] = H[21 + a] - sum[36 + a];
}

// the trial estimate of point p into the other buffer: dxl = Hinv (bl - sum_e W_e^T dxp), its edges one after the other; x + dxl
LB_FN void lb_point_step(const LbView &V, int p) {
    if (!V.p_on[p]) return;
    const size_t ne = (size_t)V.ne;
    const int buf = V.st->buf, n = 6 * V.nf;
    const double *H = V.Hll + (size_t)p * 9, *I = V.Hinv + (size_t)p * 9;
    double r[3] = {H[6], H[7], H[8]};
    for (int e = V.pt_ptr[p]; e < V.pt_ptr[p + 1]; ++e) {
        const int k = V.e_kf[e];
        if (!V.e_on[e] || k >= V.nf) continue;
        const double *d = V.dx + 6 * k;
LB_UNROLL
        for (int c = 0; c < 3; ++c) {
            double s = V.term[(9 + c) * ne + e] * d[0];
LB_UNROLL
            for (int a = 1; a < 6; ++a) s = s + V.term[(9 + 3 * a + c) * ne + e] * d[a];
            r[c] = r[c] - s;
        }
    }
    double *dl = V.dx + n + 3 * p;
    dl[0] = I[0] * r[0] + (I[1] * r[1] + I[2] * r[2]);
    dl[1] = I[1] * r[0] + (I[3] * r[1] + I[4] * r[2]);
    dl[2] = I[2] * r[0] + (I[4] * r[1] + I[5] * r[2]);
    const double *X = V.xyz + ((size_t)buf * V.np + p) * 3;
    double *Y = V.xyz + ((size_t)(1 - buf) * V.np + p) * 3;
LB_UNROLL
    for (int c = 0; c < 3; ++c) Y[c] = X[c] + dl[c];
}
// the trial estimate of keyframe k into the other buffer (a fixed one is copied)
LB_FN void lb_pose_step(const LbView &V, int k) {
    const int buf = V.st->buf;
    const double *in = V.pose + ((size_t)buf * V.nk + k) * 12;
    double *out = V.pose + ((size_t)(1 - buf) * V.nk + k) * 12;
    if (k >= V.nf) {
        for (int q = 0; q < 12; ++q) out[q] = in[q];
        return;
    }
    V.k_fail[k] = lb_exp_step(in, V.dx + 6 * k, out) ? 0 : 1;
}

// L5: partial l of a sum over the edge list (src: one value per edge; inactive edges add nothing)
LB_FN double lb_edge_partial(const LbView &V, const double *src, int l) {
    double acc = 0.0;
    for (int e = l; e < V.ne; e += 64)
        if (V.e_on[e]) acc = acc + src[e];
    return acc;
}
// b of unknown u (poses first, then points), or false when the unknown takes no part
LB_FN bool lb_unknown(const LbView &V, int u, double &b, double &diag) {
    const int n = 6 * V.nf;
    if (u < n) {
        const int dg[6] = {0, 6, 11, 15, 18, 20};
        const double *H = V.Hpp + (size_t)(u / 6) * 27;
        b = H[21 + u % 6];
        diag = H[dg[u % 6]];
        return true;
    }
    const int p = (u - n) / 3, c = (u - n) % 3;
    if (!V.p_on[p]) return false;
    const int dg[3] = {0, 3, 5};
    const double *H = V.Hll + (size_t)p * 9;
    b = H[6 + c];
    diag = H[dg[c]];
    return true;
}
// computeScale: partial l of sum_u x_u (lambda x_u + b_u)
LB_FN double lb_scale_partial(const LbView &V, int l) {
    const int nu = 6 * V.nf + 3 * V.np;
    const double lam = V.st->lam;
    double acc = 0.0, b, dg;
    for (int u = l; u < nu; u += 64)
        if (lb_unknown(V, u, b, dg)) acc = acc + V.dx[u] * (lam * V.dx[u] + b);
    return acc;
}
// computeLambdaInit: lane l's share of max |diagonal|; m starts at +0.0, a NaN never enters
LB_FN double lb_diag_partial(const LbView &V, int l) {
    const int nu = 6 * V.nf + 3 * V.np;
    double m = 0.0, b, dg;
    for (int u = l; u < nu; u += 64)
        if (lb_unknown(V, u, b, dg)) {
            const double a = fabs(dg);
            m = a > m ? a : m;
        }
    return m;
}

// the start of an iteration (after the build): the robust chi2, lambda at iteration 0
LB_FN void lb_begin(LbStatus &S, double chi2, double max_diag) {
    S.cur = chi2;
    if (S.it == 0) {
        S.lam = LB_TAU * max_diag;
        S.ni = 2.0;
    }
    S.iterations = S.iterations + 1;
    S.qmax = 0;
    S.rho = 0.0;
}
// the verdict of a trial (OptimizationAlgorithmLevenberg::solve) and what the driver does next
LB_FN void lb_judge(LbStatus &S, bool failed, double temp, double scale_sum) {
    S.trials = S.trials + 1;
    S.failed = failed ? 1 : 0;
    bool accepted = false;
    if (failed) {
        S.rho = -1.0;
        S.temp = LB_DBL_MAX;
    } else {
        const double scale = scale_sum + 1e-3;
        S.temp = temp;
        S.rho = (S.cur - temp) / scale;
        accepted = S.rho > 0.0 && lb_finite(temp);
    }
    S.accepted = accepted ? 1 : 0;
    if (accepted) {
        const double q = 2.0 * S.rho - 1.0;
        double alpha = 1.0 - (q * q) * q;
        const double up = 2.0 / 3.0, low = 1.0 / 3.0;
        alpha = up < alpha ? up : alpha;
        const double factor = low < alpha ? alpha : low;
        S.lam = S.lam * factor;
        S.ni = 2.0;
        S.cur = temp;
        S.buf = 1 - S.buf;
    } else {
        S.lam = S.lam * S.ni;
        S.ni = S.ni * 2.0;
    }
    S.qmax = S.qmax + 1;
    if (S.rho < 0.0 && S.qmax < LB_MAX_TRIALS) {
        S.next = LB_NEXT_TRIAL;
    } else if (S.qmax == LB_MAX_TRIALS || S.rho == 0.0) {
        S.next = LB_NEXT_DONE;
    } else {
        S.it = S.it + 1;
        S.next = S.it < S.max_it ? LB_NEXT_ITERATION : LB_NEXT_DONE;
    }
}
