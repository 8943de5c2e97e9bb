// afv_essgraph_math.h — the arithmetic of OptimizeEssentialGraph as tests/_essgraph_ref.py fixes it, statement for statement: double, one
// rounding per operator (-ffp-contract=off on every side), three-term sums as a0 + (a1 + a2).  ONE text for the kernels (k_essgraph.hip:
// every function here is the work of one lane - a perturbed estimate, a perturbed error, one term of an edge, partial sum l of a
// 64-partial tree, a row or an entry of a 7 x 7 block) and for the scalar host program (tools/essgraph_host.cpp, which calls the same
// functions in loops); the halving trees, the walk over the block columns and the drivers are each side's own.  The Sim3 exponential,
// product and inverse are afv_sim3opt_math.h's.  Deviations G1-G11: include/afv_hip.h.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "afv_sim3opt_math.h"

#if defined(__HIPCC__)
#define EG_FN __host__ __device__ __forceinline__
#define EG_UNROLL _Pragma("unroll")
#else
#define EG_FN static inline
#define EG_UNROLL
#endif

#define EG_NT 120                              // terms of an edge: A00 0..27 (upper triangle by rows), g0 28..34, A11 35..62, g1 63..69, A01 70..118, chi2 119
#define EG_NP 29                               // errors of an edge per linearisation: 14 with S0 perturbed, 14 with S1 perturbed, the error itself
#define EG_SCALAR (1.0 / (2.0 * SO_DELTA))
#define EG_SQRT_HALF 0x1.6a09e667f3bcdp-1
#define EG_NEXT_TRIAL 0                        // what the judge tells the driver
#define EG_NEXT_ITERATION 1
#define EG_NEXT_DONE 2
#define EG_OK 0                                // AFV_ESS_*
#define EG_NOT_FINITE 1
#define EG_EMPTY 2
#define EG_MOVED 0                             // AFV_POINT_*
#define EG_BAD_OR_UNSET 1
#define EG_NO_PAIR 2

struct EgStatus {       // the Levenberg state of the call; begin and the judge write it, the driver follows it
    double lam, ni, cur, temp, rho, chi2_first;
    int32_t buf;        // which of the two state buffers holds the accepted estimate
    int32_t it, qmax, iterations, trials, max_it, next, failed, accepted, status;
};

struct EgView {         // the problem: the same arrays on either side
    int nk, nf, ne, fixed, fix_scale;
    int nob, nb, nu;
    const int *v0, *v1;           // [ne]
    const double *meas;           // [ne][13]: R row-major, t, s
    double *S;                    // [2][nk][13]
    const int *vertex_of;         // [nf] system position -> vertex
    const int *sys_of;            // [nk] vertex -> system position, -1 for the fixed one
    const int *ve_ptr, *ve_edge;  // [nf + 1], [.]: the edges of system position i in list order, as 2 * edge + (1: the vertex is v1)
    const int *ob_ptr, *ob_edge;  // [nob + 1], [.]: the edges of off-diagonal block q of H in list order, as 2 * edge + (1: v0 is the earlier vertex)
    const int *col_ptr;           // [nf + 1]: the blocks of column j of L: col_ptr[j] the diagonal, then the rows below it, ascending
    const int *blk_row, *blk_col; // [nb]
    const int *blk_src;           // [nb]: the off-diagonal block of H that fills it, -1: fill alone
    const int *upd_ptr, *upd;     // [nf + 1], [nu][3]: per column the update triples (block L_ij, block L_kj, destination block (i, k))
    double *pert;                 // [nk][14][13]: Sim3(+-delta e_d) * estimate, d = q / 2, sign + for even q
    double *perr;                 // [ne][EG_NP][7]
    double *term;                 // [ne][EG_NT]
    double *Hd;                   // [nf][35]: H_ii's upper triangle by rows, b_i
    double *Aoff;                 // [nob][49]
    double *L;                    // [nb][49]: H + lambda I, then L in place
    double *rhs;                  // [nf][7]: b, y, x in place
    double *chi_trial;            // [ne]
    uint8_t *e_bad;               // [ne]: the error is not finite (at the estimate / at the trial)
    uint8_t *v_fail;              // [nf]: the step failed
    int32_t *solve_fail;          // [1]
    EgStatus *st;
};

// ---- G3: log and acos without a library ----
EG_FN double eg_nan() { return __builtin_nan(""); }
EG_FN double eg_log(double x) {
    const double c[12] = {0x1.0000000000000p+0, 0x1.5555555555555p-2, 0x1.999999999999ap-3, 0x1.2492492492492p-3, 0x1.c71c71c71c71cp-4, 0x1.745d1745d1746p-4,
                          0x1.3b13b13b13b14p-4, 0x1.1111111111111p-4, 0x1.e1e1e1e1e1e1ep-5, 0x1.af286bca1af28p-5, 0x1.8618618618618p-5, 0x1.642c8590b2164p-5};
    if (!(x > 0.0 && x <= SO_DBL_MAX)) return eg_nan();
    int k;
    double m = frexp(x, &k);
    if (m < EG_SQRT_HALF) {
        m = m * 2.0;
        k -= 1;
    }
    const double kf = (double)k;
    const double f = (m - 1.0) / (m + 1.0);
    const double z = f * f;
    double p = c[11];
EG_UNROLL
    for (int n = 10; n >= 0; --n) p = p * z + c[n];
    return kf * SO_LN2_HI + ((2.0 * f) * p + kf * SO_LN2_LO);
}
EG_FN double eg_acos_r(double z) {
    const double p = z * (1.66666666666666657415e-01 + z * (-3.25565818622400915405e-01 + z * (2.01212532134862925881e-01 + z * (-4.00555345006794114027e-02 +
                     z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))));
    const double q = 1.0 + z * (-2.40339491173441421878e+00 + z * (2.02094576023350569471e+00 + z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)));
    return p / q;
}
EG_FN double eg_acos(double x) {
    const double hi = 1.57079632679489655800e+00, lo = 6.12323399573676603587e-17;
    if (!(fabs(x) <= 1.0)) return eg_nan();
    if (fabs(x) < 0.5) {
        const double z = x * x;
        return hi - (x - (lo - x * eg_acos_r(z)));
    }
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5;
        const double s = sqrt(z);
        const double w = eg_acos_r(z) * s - lo;
        return 2.0 * (hi - (s + w));
    }
    if (x == 1.0) return 0.0;
    const double z = (1.0 - x) * 0.5;
    const double s = sqrt(z);
    uint64_t u;
    memcpy(&u, &s, 8);
    u &= 0xFFFFFFFF00000000ull;
    double df;
    memcpy(&df, &u, 8);
    const double c = (z - df * df) / (s + df);
    const double w = eg_acos_r(z) * s + c;
    return 2.0 * (df + w);
}

// Sim3::log: e = (omega, upsilon, sigma); returns the branch 2 * (|sigma| >= eps) + (d <= 1 - eps)
EG_FN int eg_sim3_log(const SoEst &E, double (&e)[7]) {
    const double *R = E.R;
    const double s = E.s;
    const double sg = eg_log(s);
    const double d = 0.5 * ((R[0] + (R[4] + R[8])) - 1.0);
    const double dr0 = R[7] - R[5], dr1 = R[2] - R[6], dr2 = R[3] - R[1];
    const bool near = d > (1.0 - SO_EPS), small = fabs(sg) < SO_EPS;
    double theta = 0.0, k = 0.5;
    if (!near) {
        theta = eg_acos(d);
        k = theta / (2.0 * sqrt(1.0 - d * d));
    }
    const double t2 = theta * theta;
    const double w0 = k * dr0, w1 = k * dr1, w2 = k * dr2;
    double A, B, C;
    if (small) {
        C = 1.0;
        if (near) {
            A = 0.5; B = 1.0 / 6.0;
        } else {
            A = so_exp_b(t2); B = so_exp_c(t2);
        }
    } else {
        C = (s - 1.0) / sg;
        const double sg2 = sg * sg;
        if (near) {
            A = ((sg - 1.0) * s + 1.0) / sg2;
            B = ((((0.5 * sg2 - sg) + 1.0) * s) - 1.0) / (sg2 * sg);  // G10
        } else {
            const double hA = so_exp_a(t2), hB = so_exp_b(t2);
            const double a = s * (theta * hA);     // s sin(theta)
            const double b = s * (1.0 - t2 * hB);  // s cos(theta)
            const double c = t2 + sg2;
            A = (a * sg + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sg + a * theta) / c) * (1.0 / t2);
        }
    }
    const double W[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    const double W2[9] = {-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2, w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2, w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)};
    double M[9], cof[9];
EG_UNROLL
    for (int i = 0; i < 3; ++i)
EG_UNROLL
        for (int j = 0; j < 3; ++j) {
            const int q = 3 * i + j;
            M[q] = i == j ? (C + B * W2[q]) : (A * W[q] + B * W2[q]);
        }
    // G4: the cofactors, the determinant along row 0, M^-1 = cof^T / det
EG_UNROLL
    for (int i = 0; i < 3; ++i)
EG_UNROLL
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            cof[3 * i + j] = M[3 * i1 + j1] * M[3 * i2 + j2] - M[3 * i1 + j2] * M[3 * i2 + j1];
        }
    const double det = M[0] * cof[0] + (M[1] * cof[1] + M[2] * cof[2]);
    const double r = 1.0 / det;
    e[0] = w0; e[1] = w1; e[2] = w2;
EG_UNROLL
    for (int i = 0; i < 3; ++i) e[3 + i] = (cof[i] * r) * E.t[0] + ((cof[3 + i] * r) * E.t[1] + (cof[6 + i] * r) * E.t[2]);
    e[6] = sg;
    return 2 * (small ? 0 : 1) + (near ? 0 : 1);
}

EG_FN void eg_load(const double *p, SoEst &E) {
EG_UNROLL
    for (int q = 0; q < 9; ++q) E.R[q] = p[q];
EG_UNROLL
    for (int q = 0; q < 3; ++q) E.t[q] = p[9 + q];
    E.s = p[12];
}
EG_FN void eg_store(const SoEst &E, double *p) {
EG_UNROLL
    for (int q = 0; q < 9; ++q) p[q] = E.R[q];
EG_UNROLL
    for (int q = 0; q < 3; ++q) p[9 + q] = E.t[q];
    p[12] = E.s;
}

// EdgeSim3::computeError: log((C * S0) * S1^-1)
EG_FN int eg_edge_error(const SoEst &C, const SoEst &S0, const SoEst &S1, double (&e)[7]) {
    SoEst T, I, U;
    so_compose(C, S0, T);
    so_inverse(S1, I);
    so_compose(T, I, U);
    return eg_sim3_log(U, e);
}

// Sim3::map: s (R x) + t
EG_FN void eg_map(const SoEst &E, const double (&X)[3], double (&Y)[3]) {
EG_UNROLL
    for (int r = 0; r < 3; ++r) Y[r] = E.s * (E.R[3 * r] * X[0] + (E.R[3 * r + 1] * X[1] + E.R[3 * r + 2] * X[2])) + E.t[r];
}

// perturbed estimate q (d = q / 2, + for even q) of vertex k: Sim3(+-delta e_d) * estimate, update[6] = 0 under fix_scale
EG_FN void eg_perturb(const EgView &V, int k, int q) {
    double u[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
EG_UNROLL
    for (int d = 0; d < 7; ++d)
        if (d == q / 2) u[d] = (q & 1) ? -SO_DELTA : SO_DELTA;
    if (V.fix_scale) u[6] = 0.0;
    SoEst D, E, out;
    so_sim3_exp(u, D);
    eg_load(V.S + ((size_t)V.st->buf * V.nk + k) * 13, E);
    so_compose(D, E, out);
    eg_store(out, V.pert + ((size_t)k * 14 + q) * 13);
}

// error p of edge e: p < 14: S0 perturbed (q = p), p < 28: S1 perturbed (q = p - 14), 28: at the estimate
EG_FN void eg_edge_perr(const EgView &V, int e, int p) {
    SoEst C, S0, S1;
    const int a = V.v0[e], b = V.v1[e];
    eg_load(V.meas + (size_t)e * 13, C);
    eg_load(p < 14 ? V.pert + ((size_t)a * 14 + p) * 13 : V.S + ((size_t)V.st->buf * V.nk + a) * 13, S0);
    eg_load(p >= 14 && p < 28 ? V.pert + ((size_t)b * 14 + (p - 14)) * 13 : V.S + ((size_t)V.st->buf * V.nk + b) * 13, S1);
    double err[7];
    eg_edge_error(C, S0, S1, err);
    double *o = V.perr + ((size_t)e * EG_NP + p) * 7;
EG_UNROLL
    for (int r = 0; r < 7; ++r) o[r] = err[r];
}

// BaseBinaryEdge::linearizeOplus: entry (r, d) of the Jacobian of side 0 / 1 of edge e
EG_FN double eg_jac(const EgView &V, int e, int side, int r, int d) {
    const double *p = V.perr + ((size_t)e * EG_NP + side * 14 + 2 * d) * 7;
    return EG_SCALAR * (p[r] - p[7 + r]);
}
// sum_r Ja[r][a] Jb[r][b], one after the other
EG_FN double eg_jtj(const EgView &V, int e, int sa, int a, int sb, int b) {
    double s = eg_jac(V, e, sa, 0, a) * eg_jac(V, e, sb, 0, b);
    for (int r = 1; r < 7; ++r) s = s + eg_jac(V, e, sa, r, a) * eg_jac(V, e, sb, r, b);
    return s;
}
// sum_r J[r][a] (-e[r])
EG_FN double eg_jtg(const EgView &V, int e, int side, int a) {
    const double *err = V.perr + ((size_t)e * EG_NP + 28) * 7;
    double s = eg_jac(V, e, side, 0, a) * -err[0];
    for (int r = 1; r < 7; ++r) s = s + eg_jac(V, e, side, r, a) * -err[r];
    return s;
}
EG_FN void eg_upper(int q, int &i, int &j) {  // position q of the upper triangle by rows
    i = 0;
    while (q >= 7 - i) {
        q -= 7 - i;
        ++i;
    }
    j = i + q;
}
EG_FN int eg_upper_at(int a, int b) {  // where entry (a, b) of a symmetric block lies in its upper triangle
    const int i = a < b ? a : b, j = a < b ? b : a;
    return 7 * i - (i * (i - 1)) / 2 + (j - i);
}
// term q of edge e
EG_FN void eg_edge_term(const EgView &V, int e, int q) {
    double v;
    int i, j;
    if (q < 28) {
        eg_upper(q, i, j);
        v = eg_jtj(V, e, 0, i, 0, j);
    } else if (q < 35) {
        v = eg_jtg(V, e, 0, q - 28);
    } else if (q < 63) {
        eg_upper(q - 35, i, j);
        v = eg_jtj(V, e, 1, i, 1, j);
    } else if (q < 70) {
        v = eg_jtg(V, e, 1, q - 63);
    } else if (q < 119) {
        v = eg_jtj(V, e, 0, (q - 70) / 7, 1, (q - 70) % 7);
    } else {
        const double *err = V.perr + ((size_t)e * EG_NP + 28) * 7;
        bool ok = so_finite(err[0]);
        v = err[0] * err[0];
        for (int r = 1; r < 7; ++r) {
            v = v + err[r] * err[r];
            ok = ok && so_finite(err[r]);
        }
        V.e_bad[e] = ok ? 0 : 1;
    }
    V.term[(size_t)e * EG_NT + q] = v;
}

// G6: partial l of value q (0..27 H_ii, 28..34 b_i) of system position i over that vertex's edges
EG_FN double eg_vertex_partial(const EgView &V, int i, int q, int l) {
    double acc = 0.0;
    for (int p = V.ve_ptr[i] + l; p < V.ve_ptr[i + 1]; p += 64) {
        const int c = V.ve_edge[p];
        acc = acc + V.term[(size_t)(c >> 1) * EG_NT + (c & 1) * 35 + q];
    }
    return acc;
}
// G6: entry (a, b) of off-diagonal block q of H (rows: the later vertex), its edges one after the other
EG_FN double eg_offdiag_entry(const EgView &V, int q, int a, int b) {
    double acc = 0.0;
    for (int p = V.ob_ptr[q]; p < V.ob_ptr[q + 1]; ++p) {
        const int c = V.ob_edge[p];
        acc = acc + V.term[(size_t)(c >> 1) * EG_NT + 70 + ((c & 1) ? 7 * b + a : 7 * a + b)];
    }
    return acc;
}
// partial l of a sum over the edge list
EG_FN double eg_edge_partial(const EgView &V, const double *src, size_t stride, int l) {
    double acc = 0.0;
    for (int e = l; e < V.ne; e += 64) acc = acc + src[(size_t)e * stride];
    return acc;
}
// computeScale: partial l of sum_u x_u (lambda x_u + b_u) over the unknowns in system order
EG_FN double eg_scale_partial(const EgView &V, int l) {
    const double lam = V.st->lam;
    double acc = 0.0;
    for (int u = l; u < 7 * V.nf; u += 64) acc = acc + V.rhs[u] * (lam * V.rhs[u] + V.Hd[(size_t)(u / 7) * 35 + 28 + u % 7]);
    return acc;
}

// entry t of block b of the damped system before a factorisation
EG_FN void eg_load_entry(const EgView &V, int b, int t) {
    double v = 0.0;
    if (V.blk_row[b] == V.blk_col[b]) {
        v = V.Hd[(size_t)V.blk_col[b] * 35 + eg_upper_at(t / 7, t % 7)];
        if (t / 7 == t % 7) v = v + V.st->lam;
    } else if (V.blk_src[b] >= 0) {
        v = V.Aoff[(size_t)V.blk_src[b] * 49 + t];
    }
    V.L[(size_t)b * 49 + t] = v;
}

// G1: the unpivoted L L^T of the lower triangle of a block, in place (L7's loops).  false: a pivot that is not positive and finite
EG_FN bool eg_chol7(double *blk) {
    double A[49];
EG_UNROLL
    for (int q = 0; q < 49; ++q) A[q] = blk[q];
    bool ok = true;
EG_UNROLL
    for (int c = 0; c < 7; ++c) {
        double s = A[7 * c + c];
EG_UNROLL
        for (int k = 0; k < c; ++k) s = s - A[7 * c + k] * A[7 * c + k];
        if (!(s > 0.0 && so_finite(s))) ok = false;
        const double d = sqrt(s);
        A[7 * c + c] = d;
EG_UNROLL
        for (int r = c + 1; r < 7; ++r) {
            s = A[7 * r + c];
EG_UNROLL
            for (int k = 0; k < c; ++k) s = s - A[7 * r + k] * A[7 * c + k];
            A[7 * r + c] = s / d;
        }
    }
EG_UNROLL
    for (int q = 0; q < 49; ++q) blk[q] = A[q];
    return ok;
}
// G1: row a of L_ij = A_ij L_jj^-T, in place
EG_FN void eg_trsm_row(const double *Ljj, double *blk, int a) {
    double x[7];
EG_UNROLL
    for (int c = 0; c < 7; ++c) {
        double s = blk[7 * a + c];
EG_UNROLL
        for (int k = 0; k < c; ++k) s = s - x[k] * Ljj[7 * c + k];
        x[c] = s / Ljj[7 * c + c];
    }
EG_UNROLL
    for (int c = 0; c < 7; ++c) blk[7 * a + c] = x[c];
}
// G1: entry (a, b) of A_ik -= L_ij L_kj^T
EG_FN void eg_update_entry(const double *Li, const double *Lk, double *dst, int a, int b) {
    double v = dst[7 * a + b];
EG_UNROLL
    for (int c = 0; c < 7; ++c) v = v - Li[7 * a + c] * Lk[7 * b + c];
    dst[7 * a + b] = v;
}
// forward substitution inside block column j: L_jj y = r, in place
EG_FN void eg_fwd_diag(const double *Ljj, double *r) {
    double y[7];
EG_UNROLL
    for (int c = 0; c < 7; ++c) {
        double s = r[c];
EG_UNROLL
        for (int k = 0; k < c; ++k) s = s - Ljj[7 * c + k] * y[k];
        y[c] = s / Ljj[7 * c + c];
    }
EG_UNROLL
    for (int c = 0; c < 7; ++c) r[c] = y[c];
}
// ... and below it: entry a of r_i -= L_ij y_j
EG_FN void eg_fwd_row(const double *Lij, const double *y, double *ri, int a) {
    double s = ri[a];
EG_UNROLL
    for (int c = 0; c < 7; ++c) s = s - Lij[7 * a + c] * y[c];
    ri[a] = s;
}
// back substitution: entry a of r_j - sum_i L_ij^T x_i over the rows of column j in descending order
EG_FN double eg_back_gather(const EgView &V, int j, int a) {
    double s = V.rhs[(size_t)j * 7 + a];
    for (int b = V.col_ptr[j + 1] - 1; b > V.col_ptr[j]; --b) {
        const double *Lij = V.L + (size_t)b * 49, *x = V.rhs + (size_t)V.blk_row[b] * 7;
        for (int c = 6; c >= 0; --c) s = s - Lij[7 * c + a] * x[c];
    }
    return s;
}
// ... and the block's own: L_jj^T x = s, descending
EG_FN void eg_back_diag(const double *Ljj, const double *s, double *xo) {
    double x[7];
EG_UNROLL
    for (int a = 6; a >= 0; --a) {
        double v = s[a];
EG_UNROLL
        for (int k = 6; k > a; --k) v = v - Ljj[7 * k + a] * x[k];
        x[a] = v / Ljj[7 * a + a];
    }
EG_UNROLL
    for (int a = 0; a < 7; ++a) xo[a] = x[a];
}

// the trial estimate of vertex k into the other buffer (the fixed one is copied)
EG_FN void eg_vertex_step(const EgView &V, int k) {
    const int buf = V.st->buf, i = V.sys_of[k];
    const double *in = V.S + ((size_t)buf * V.nk + k) * 13;
    double *out = V.S + ((size_t)(1 - buf) * V.nk + k) * 13;
    for (int q = 0; q < 13; ++q) out[q] = in[q];
    if (i < 0) return;
    const double *x = V.rhs + (size_t)i * 7;
    const double u[7] = {x[0], x[1], x[2], x[3], x[4], x[5], V.fix_scale ? 0.0 : x[6]};
    SoEst D, E, N;
    if (!so_sim3_exp(u, D)) {
        V.v_fail[i] = 1;
        return;
    }
    V.v_fail[i] = 0;
    eg_load(in, E);
    so_compose(D, E, N);
    eg_store(N, out);
}
// the chi2 of edge e at the trial estimate
EG_FN void eg_edge_trial(const EgView &V, int e) {
    SoEst C, S0, S1;
    const size_t base = (size_t)(1 - V.st->buf) * V.nk;
    eg_load(V.meas + (size_t)e * 13, C);
    eg_load(V.S + (base + V.v0[e]) * 13, S0);
    eg_load(V.S + (base + V.v1[e]) * 13, S1);
    double err[7];
    eg_edge_error(C, S0, S1, err);
    bool ok = so_finite(err[0]);
    double v = err[0] * err[0];
EG_UNROLL
    for (int r = 1; r < 7; ++r) {
        v = v + err[r] * err[r];
        ok = ok && so_finite(err[r]);
    }
    V.chi_trial[e] = v;
    V.e_bad[e] = ok ? 0 : 1;
}

// the start of an iteration (after the build): the chi2; at iteration 0 lambda = userLambdaInit and G5
EG_FN void eg_begin(EgStatus &S, double chi2, bool bad, double lambda_init) {
    S.cur = chi2;
    if (S.it == 0) {
        if (bad) {
            S.status = EG_NOT_FINITE;
            S.next = EG_NEXT_DONE;
            S.cur = 0.0;
            return;
        }
        S.lam = lambda_init;
        S.ni = 2.0;
        S.chi2_first = chi2;
    }
    S.iterations = S.iterations + 1;
    S.qmax = 0;
    S.rho = 0.0;
}
// the verdict of a trial (OptimizationAlgorithmLevenberg::solve) and what the driver does next
EG_FN void eg_judge(EgStatus &S, bool failed, double temp, double scale_sum) {
    if (S.status != EG_OK) return;
    S.trials = S.trials + 1;
    S.failed = failed ? 1 : 0;
    bool accepted = false;
    if (failed) {
        S.rho = -1.0;
        S.temp = SO_DBL_MAX;
    } else {
        const double scale = scale_sum + 1e-3;
        S.temp = temp;
        S.rho = (S.cur - temp) / scale;
        accepted = S.rho > 0.0 && so_finite(temp);
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
    if (S.rho < 0.0 && S.qmax < SO_MAX_TRIALS) {
        S.next = EG_NEXT_TRIAL;
    } else if (S.qmax == SO_MAX_TRIALS || S.rho == 0.0) {
        S.next = EG_NEXT_DONE;
    } else {
        S.it = S.it + 1;
        S.next = S.it < S.max_it ? EG_NEXT_ITERATION : EG_NEXT_DONE;
    }
}

// :979-998: Tiw = [R | t * (1 / s)], correctedSwc = S^-1 (13 doubles)
EG_FN void eg_recover(const double *S, double *S_out, double *Tiw, double *Swc) {
    SoEst E, I;
    eg_load(S, E);
    so_inverse(E, I);
    const double inv_s = 1.0 / E.s;
    for (int q = 0; q < 9; ++q) Tiw[q] = E.R[q];
    for (int q = 0; q < 3; ++q) Tiw[9 + q] = E.t[q] * inv_s;
    eg_store(E, S_out);
    eg_store(I, Swc);
}
// :1000-1030: S_to.map(S_from.map(double(P)))
EG_FN void eg_correct(const double *S_from, const double *S_to, const float (&P)[3], double (&out)[3]) {
    SoEst A, B;
    eg_load(S_from, A);
    eg_load(S_to, B);
    const double X[3] = {(double)P[0], (double)P[1], (double)P[2]};
    double Y[3];
    eg_map(A, X, Y);
    eg_map(B, Y, out);
}
