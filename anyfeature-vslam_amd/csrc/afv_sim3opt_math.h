// afv_sim3opt_math.h — the scalar arithmetic of OptimizeSim3 as tests/_sim3opt_ref.py fixes it, statement for statement: double, one
// rounding per operator (-ffp-contract=off on every side), three-term sums as a0 + (a1 + a2).  ONE text for the kernel (k_sim3opt.hip,
// where every function is lane-uniform or per-lane scalar code) and for the scalar host program (tools/sim3opt_host.cpp); the sums over
// the correspondences, the loops of optimize() and the classifications are each side's own.  Deviations O1-O7: include/afv_hip.h.
// Everything is indexed with compile-time indices: after unrolling no array here is addressed at run time (no scratch on the device).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define SO_FN __host__ __device__ __forceinline__
#define SO_UNROLL _Pragma("unroll")
#else
#define SO_FN static inline
#define SO_UNROLL
#endif

#define SO_EPS 0.00001                         // Sim3(Vector7): |sigma| < eps, theta < eps
#define SO_DELTA 1e-9                          // BaseBinaryEdge::linearizeOplus
#define SO_SIGMA_MAX 64.0                      // O4
#define SO_PI2 0x1.3bd3cc9be45dep+3            // (double)pi * (double)pi
#define SO_LOG2E 0x1.71547652b82fep+0
#define SO_LN2_HI 0x1.62e42fee00000p-1
#define SO_LN2_LO 0x1.a39ef35793c76p-33
#define SO_TAU 1e-5
#define SO_DBL_MAX 0x1.fffffffffffffp+1023
#define SO_MAX_TRIALS 10
#define SO_MIN_CORRESPONDENCES 10

struct SoEst {       // a Sim3: R row-major, t, s
    double R[9], t[3], s;
};
struct SoPair {      // an estimate and its inverse: what the two edges of a correspondence read
    SoEst f, i;
};
struct SoCam {
    double fx, fy, cx, cy;
};

SO_FN bool so_finite(double v) { return fabs(v) <= SO_DBL_MAX; }

// O4: PoseOptimization's EXP_A / EXP_B / EXP_C, digit for digit
SO_FN double so_horner16(const double (&c)[16], double t2) {
    double r = c[15];
SO_UNROLL
    for (int k = 14; k >= 0; --k) r = r * t2 + c[k];
    return r;
}
SO_FN double so_exp_a(double t2) {  // sin(th) / th
    const double c[16] = {0x1.0000000000000p+0, -0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19,
                          -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49, -0x1.2f49b46814157p-57,
                          0x1.71b8ef6dcf572p-66, -0x1.761b41316381ap-75, 0x1.3f3ccdd165fa9p-84, -0x1.d1ab1c2dccea3p-94, 0x1.259f98b4358adp-103,
                          -0x1.434d2e783f5bcp-113};
    return so_horner16(c, t2);
}
SO_FN double so_exp_b(double t2) {  // (1 - cos th) / th^2
    const double c[16] = {0x1.0000000000000p-1, -0x1.5555555555555p-5, 0x1.6c16c16c16c17p-10, -0x1.a01a01a01a01ap-16, 0x1.27e4fb7789f5cp-22,
                          -0x1.1eed8eff8d898p-29, 0x1.93974a8c07c9dp-37, -0x1.ae7f3e733b81fp-45, 0x1.6827863b97d97p-53, -0x1.e542ba4020225p-62,
                          0x1.0ce396db7f853p-70, -0x1.f2cf01972f578p-80, 0x1.88e85fc6a4e5ap-89, -0x1.0a18a2635085dp-98, 0x1.3932c5047d60ep-108,
                          -0x1.434d2e783f5bcp-118};
    return so_horner16(c, t2);
}
SO_FN double so_exp_c(double t2) {  // (th - sin th) / th^3
    const double c[16] = {0x1.5555555555555p-3, -0x1.1111111111111p-7, 0x1.a01a01a01a01ap-13, -0x1.71de3a556c734p-19, 0x1.ae64567f544e4p-26,
                          -0x1.6124613a86d09p-33, 0x1.ae7f3e733b81fp-41, -0x1.952c77030ad4ap-49, 0x1.2f49b46814157p-57, -0x1.71b8ef6dcf572p-66,
                          0x1.761b41316381ap-75, -0x1.3f3ccdd165fa9p-84, 0x1.d1ab1c2dccea3p-94, -0x1.259f98b4358adp-103, 0x1.434d2e783f5bcp-113,
                          -0x1.3981254dd0d52p-123};
    return so_horner16(c, t2);
}

// O4: exp of a finite |x| <= 64: 2^k * P(r), P the Taylor polynomial of degree 13 (EXP_T of the restatement: 1 / n! correctly rounded)
SO_FN double so_exp_sigma(double x) {
    const double c[14] = {0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x1.0000000000000p-1, 0x1.5555555555555p-3, 0x1.5555555555555p-5,
                          0x1.1111111111111p-7, 0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-13, 0x1.a01a01a01a01ap-16, 0x1.71de3a556c734p-19,
                          0x1.27e4fb7789f5cp-22, 0x1.ae64567f544e4p-26, 0x1.1eed8eff8d898p-29, 0x1.6124613a86d09p-33};
    const double kf = floor(x * SO_LOG2E + 0.5);
    const double r = (x - kf * SO_LN2_HI) - kf * SO_LN2_LO;
    double p = c[13];
SO_UNROLL
    for (int k = 12; k >= 0; --k) p = p * r + c[k];
    return ldexp(p, (int)kf);
}

// Sim3::Sim3(const Vector7 &update), update = (omega, upsilon, sigma).  false: a failed trial (O4)
SO_FN bool so_sim3_exp(const double (&u)[7], SoEst &d) {
    const double w0 = u[0], w1 = u[1], w2 = u[2], sg = u[6];
    if (!(fabs(sg) <= SO_SIGMA_MAX)) return false;
    const double t2 = w0 * w0 + (w1 * w1 + w2 * w2);
    if (!(t2 <= SO_PI2)) return false;
    const double theta = sqrt(t2);
    const double s = so_exp_sigma(sg);
    const double hA = so_exp_a(t2), hB = so_exp_b(t2), hC = so_exp_c(t2);
    double A, B, C, ra, rb;
    if (fabs(sg) < SO_EPS) {
        C = 1.0;
        if (theta < SO_EPS) {
            A = 0.5; B = 1.0 / 6.0; ra = 1.0; rb = 1.0;  // R = I + Omega + Omega2, as written upstream
        } else {
            A = hB; B = hC; ra = hA; rb = hB;
        }
    } else {
        C = (s - 1.0) / sg;
        const double sg2 = sg * sg;
        if (theta < SO_EPS) {
            A = ((sg - 1.0) * s + 1.0) / sg2;
            B = (((0.5 * sg2 - sg) + 1.0) * s) / (sg2 * sg);  // as written upstream (no "- 1")
            ra = 1.0; rb = 1.0;
        } else {
            ra = hA; rb = hB;
            const double a = s * (theta * hA);   // s sin(theta)
            const double b = s * (1.0 - t2 * hB);  // s cos(theta)
            const double c = t2 + sg2;
            A = (a * sg + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sg + a * theta) / c) * (1.0 / t2);
        }
    }
    const double W[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    const double W2[9] = {-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2, w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2, w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)};
    double Wm[9];
SO_UNROLL
    for (int i = 0; i < 3; ++i)
SO_UNROLL
        for (int j = 0; j < 3; ++j) {
            const int k = 3 * i + j;
            d.R[k] = i == j ? (1.0 + rb * W2[k]) : (ra * W[k] + rb * W2[k]);
            Wm[k] = i == j ? (C + B * W2[k]) : (A * W[k] + B * W2[k]);
        }
SO_UNROLL
    for (int i = 0; i < 3; ++i) d.t[i] = Wm[3 * i] * u[3] + (Wm[3 * i + 1] * u[4] + Wm[3 * i + 2] * u[5]);
    d.s = s;
    return true;
}

// Sim3::operator*: d * E
SO_FN void so_compose(const SoEst &d, const SoEst &E, SoEst &out) {
SO_UNROLL
    for (int i = 0; i < 3; ++i) {
SO_UNROLL
        for (int j = 0; j < 3; ++j) out.R[3 * i + j] = d.R[3 * i] * E.R[j] + (d.R[3 * i + 1] * E.R[3 + j] + d.R[3 * i + 2] * E.R[6 + j]);
        out.t[i] = d.s * (d.R[3 * i] * E.t[0] + (d.R[3 * i + 1] * E.t[1] + d.R[3 * i + 2] * E.t[2])) + d.t[i];
    }
    out.s = d.s * E.s;
}

// Sim3::inverse: (R^T, R^T (t * (-1 / s)), 1 / s)
SO_FN void so_inverse(const SoEst &E, SoEst &out) {
    const double m = -1.0 / E.s;
    const double tm0 = E.t[0] * m, tm1 = E.t[1] * m, tm2 = E.t[2] * m;
SO_UNROLL
    for (int i = 0; i < 3; ++i) {
SO_UNROLL
        for (int j = 0; j < 3; ++j) out.R[3 * i + j] = E.R[3 * j + i];
        out.t[i] = E.R[i] * tm0 + (E.R[3 + i] * tm1 + E.R[6 + i] * tm2);
    }
    out.s = 1.0 / E.s;
}

// VertexSim3Expmap::oplusImpl: Sim3(update) * estimate, update[6] = 0 under fix_scale; the inverse comes along.  false: a failed trial
SO_FN bool so_step(const SoEst &E, const double (&x)[7], bool fix_scale, SoPair &out) {
    const double u[7] = {x[0], x[1], x[2], x[3], x[4], x[5], fix_scale ? 0.0 : x[6]};
    SoEst d;
    if (!so_sim3_exp(u, d)) return false;
    so_compose(d, E, out.f);
    so_inverse(out.f, out.i);
    return true;
}

// obs - cam_map(project(Sim3.map(X))), Sim3::map = s (R x) + t
SO_FN void so_project_error(const SoEst &E, const SoCam &K, const double (&X)[3], const double (&obs)[2], double (&e)[2]) {
    const double q0 = E.s * (E.R[0] * X[0] + (E.R[1] * X[1] + E.R[2] * X[2])) + E.t[0];
    const double q1 = E.s * (E.R[3] * X[0] + (E.R[4] * X[1] + E.R[5] * X[2])) + E.t[1];
    const double q2 = E.s * (E.R[6] * X[0] + (E.R[7] * X[1] + E.R[8] * X[2])) + E.t[2];
    e[0] = obs[0] - (K.fx * (q0 / q2) + K.cx);
    e[1] = obs[1] - (K.fy * (q1 / q2) + K.cy);
}
SO_FN double so_chi2(const double (&e)[2], double inf) { return e[0] * (inf * e[0]) + e[1] * (inf * e[1]); }

// RobustKernelHuber::robustify: rho[0], rho[1]
SO_FN void so_huber(double chi2, double delta, double &rho0, double &rho1) {
    const double dsqr = delta * delta;
    if (chi2 <= dsqr) {
        rho0 = chi2;
        rho1 = 1.0;
    } else {
        const double s = sqrt(chi2);
        rho0 = (2.0 * s) * delta - dsqr;
        rho1 = delta / s;
    }
}

// one correspondence at one estimate: both errors, both chi2
struct SoEdge {
    double p1[3], p2[3], obs1[2], obs2[2], inf1, inf2;
};
SO_FN void so_edge_errors(const SoPair &E, const SoCam &K1, const SoCam &K2, const SoEdge &g, double (&e12)[2], double (&e21)[2]) {
    so_project_error(E.f, K1, g.p2, g.obs1, e12);
    so_project_error(E.i, K2, g.p1, g.obs2, e21);
}
// the correspondence's term of the robust chi2 (O5: e12's + e21's)
SO_FN double so_edge_robust(const SoPair &E, const SoCam &K1, const SoCam &K2, const SoEdge &g, double delta) {
    double e12[2], e21[2], a0, a1, b0, b1;
    so_edge_errors(E, K1, K2, g, e12, e21);
    so_huber(so_chi2(e12, g.inf1), delta, a0, a1);
    so_huber(so_chi2(e21, g.inf2), delta, b0, b1);
    return a0 + b0;
}
// O1, O2: e12.chi2() > th2 || e21.chi2() > th2; not finite counts as an outlier
SO_FN bool so_edge_outlier(const SoPair &E, const SoCam &K1, const SoCam &K2, const SoEdge &g, double th2) {
    double e12[2], e21[2];
    so_edge_errors(E, K1, K2, g, e12, e21);
    const double c12 = so_chi2(e12, g.inf1), c21 = so_chi2(e21, g.inf2);
    return !so_finite(c12) || c12 > th2 || !so_finite(c21) || c21 > th2;
}

// the 36 terms of a correspondence (O5): H's upper triangle by rows (28), b (7), the robust chi2; J12 / J21 [r][d]
SO_FN void so_edge_terms(const double (&e12)[2], const double (&e21)[2], const double (&J12)[2][7], const double (&J21)[2][7], double inf1, double inf2,
                         double delta, double (&term)[36]) {
    double r12_0, r12_1, r21_0, r21_1;
    so_huber(so_chi2(e12, inf1), delta, r12_0, r12_1);
    so_huber(so_chi2(e21, inf2), delta, r21_0, r21_1);
    const double w12 = r12_1 * inf1, w21 = r21_1 * inf2;                   // robustInformation: rho[1] * Omega
    const double g12_0 = r12_1 * -(inf1 * e12[0]), g12_1 = r12_1 * -(inf1 * e12[1]);  // rho[1] * (-Omega e)
    const double g21_0 = r21_1 * -(inf2 * e21[0]), g21_1 = r21_1 * -(inf2 * e21[1]);
    int k = 0;
SO_UNROLL
    for (int i = 0; i < 7; ++i)
SO_UNROLL
        for (int j = i; j < 7; ++j) {
            const double h12 = J12[0][i] * (w12 * J12[0][j]) + J12[1][i] * (w12 * J12[1][j]);
            const double h21 = J21[0][i] * (w21 * J21[0][j]) + J21[1][i] * (w21 * J21[1][j]);
            term[k++] = h12 + h21;
        }
SO_UNROLL
    for (int j = 0; j < 7; ++j) term[28 + j] = (J12[0][j] * g12_0 + J12[1][j] * g12_1) + (J21[0][j] * g21_0 + J21[1][j] * g21_1);
    term[35] = r12_0 + r21_0;
}

// (H + lam I) x = b by an unpivoted L L^T in a fixed loop order (O6); Hu = the upper triangle by rows.  false: a pivot not positive and finite
SO_FN bool so_solve7(const double (&Hu)[28], const double (&b)[7], double lam, double (&x)[7]) {
    double H[7][7], L[7][7];
    {
        int k = 0;
SO_UNROLL
        for (int i = 0; i < 7; ++i)
SO_UNROLL
            for (int j = i; j < 7; ++j) {
                H[i][j] = Hu[k];
                H[j][i] = Hu[k];
                ++k;
            }
    }
SO_UNROLL
    for (int j = 0; j < 7; ++j) {
        double s = H[j][j] + lam;
SO_UNROLL
        for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
        if (!(s > 0.0 && so_finite(s))) return false;
        L[j][j] = sqrt(s);
SO_UNROLL
        for (int i = j + 1; i < 7; ++i) {
            s = H[j][i];
SO_UNROLL
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    double y[7];
SO_UNROLL
    for (int i = 0; i < 7; ++i) {
        double s = b[i];
SO_UNROLL
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
SO_UNROLL
    for (int i = 6; i >= 0; --i) {
        double s = y[i];
SO_UNROLL
        for (int k = i + 1; k < 7; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

// computeLambdaInit: tau * max |H_jj|
SO_FN double so_lambda_init(const double (&Hu)[28]) {
    const int diag[7] = {0, 7, 13, 18, 22, 25, 27};
    double m = fabs(Hu[0]);
SO_UNROLL
    for (int j = 1; j < 7; ++j) {
        const double a = fabs(Hu[diag[j]]);
        m = a > m ? a : m;
    }
    return SO_TAU * m;
}

// the verdict of a trial (OptimizationAlgorithmLevenberg::solve): rho from the robust chi2 before / after; updates lambda and ni
struct SoTrial {
    double rho;
    bool accepted;
};
SO_FN SoTrial so_judge(bool failed, double cur, double temp, const double (&x)[7], const double (&b)[7], double &lam, double &ni) {
    SoTrial T;
    T.accepted = false;
    if (failed) {
        T.rho = -1.0;
    } else {
        double scale = 0.0;
SO_UNROLL
        for (int j = 0; j < 7; ++j) scale = scale + x[j] * (lam * x[j] + b[j]);  // computeScale
        scale = scale + 1e-3;
        T.rho = (cur - temp) / scale;
        T.accepted = T.rho > 0.0 && so_finite(temp);
    }
    if (T.accepted) {
        const double q = 2.0 * T.rho - 1.0;
        double alpha = 1.0 - (q * q) * q;
        const double up = 2.0 / 3.0, low = 1.0 / 3.0;
        alpha = up < alpha ? up : alpha;
        const double factor = low < alpha ? alpha : low;
        lam = lam * factor;
        ni = 2.0;
    } else {
        lam = lam * ni;
        ni = ni * 2.0;
    }
    return T;
}
