// afv_gba_math.h — the block-sparse solve of the reduced camera system (deviation L7' of tests/_gba_ref.py) and the float point correction
// of LoopClosing::RunGlobalBundleAdjustment, as ONE text for the kernels (k_gba.hip: every function here is the work of one lane) and for
// the scalar host program (tools/lba_host.cpp, gba_host).  Everything else of the bundle adjustment is afv_lba_math.h, unchanged.
//
// L is stored by block columns in the order of the free-keyframe list: block b = col_ptr[j] is the diagonal block of column j, the blocks
// col_ptr[j] + 1 .. col_ptr[j + 1] - 1 are its sub-diagonal blocks in ascending row.  A block is 36 doubles, row-major: entry (a, c) of
// block (row i, column j) is element (6 i + a, 6 j + c) of L.  Of a diagonal block only a >= c is written and read.
// Every scalar element subtracts its products ONE AFTER THE OTHER in ascending k, exactly as the dense L7 does; the products with a
// factor in a block outside the fill do not exist here.
#pragma once

#include "afv_lba_math.h"

struct GbView {              // the plan (host-derived, afv_gba_plan.h) and the blocks of L
    int nf, nb;
    const int *col_ptr;      // [nf + 1]
    const int *blk_row;      // [nb]
    const int *blk_col;      // [nb]
    const uint8_t *blk_kind; // [nb] 1: a structural block of S (evaluated every trial); 0: fill (starts every trial as zeros)
    double *L;               // [nb][36]
};

// after the tree: block (i, j >= i) of S = (Hpp + lambda on the diagonal) - sum, into block (row j, column i) of L; bS from the diagonal
// block.  The values are lb_schur_store's, only the place differs.
LB_FN void gb_schur_store(const LbView &V, double *blk, int i, int j, const double (&sum)[42]) {
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
            blk[6 * b + a] = h - sum[6 * a + b];
        }
    if (j == i)
        for (int a = 0; a < 6; ++a) V.bS[6 * i + a] = H[21 + a] - sum[36 + a];
}

// the diagonal block of a column, after every earlier column has updated it: its own 6 x 6 L L^T.  false: a pivot that is not positive and finite
LB_FN bool gb_chol6(double *blk) {
    double A[36];
LB_UNROLL
    for (int q = 0; q < 36; ++q) A[q] = q % 6 <= q / 6 ? blk[q] : 0.0;
    bool ok = true;
LB_UNROLL
    for (int c = 0; c < 6; ++c) {
        double s = A[6 * c + c];
LB_UNROLL
        for (int k = 0; k < c; ++k) s = s - A[6 * c + k] * A[6 * c + k];
        if (!(s > 0.0 && lb_finite(s))) ok = false;
        const double d = sqrt(s);
        A[6 * c + c] = d;
LB_UNROLL
        for (int r = c + 1; r < 6; ++r) {
            s = A[6 * r + c];
LB_UNROLL
            for (int k = 0; k < c; ++k) s = s - A[6 * r + k] * A[6 * c + k];
            A[6 * r + c] = s / d;
        }
    }
LB_UNROLL
    for (int c = 0; c < 6; ++c)
LB_UNROLL
        for (int r = c; r < 6; ++r) blk[6 * r + c] = A[6 * r + c];
    return ok;
}
// row a of a sub-diagonal block against the factored diagonal block of its column
LB_FN void gb_trsm_row(const double *Ljj, double *blk, int a) {
    double x[6];
LB_UNROLL
    for (int c = 0; c < 6; ++c) {
        double s = blk[6 * a + c];
LB_UNROLL
        for (int k = 0; k < c; ++k) s = s - x[k] * Ljj[6 * c + k];
        x[c] = s / Ljj[6 * c + c];
    }
LB_UNROLL
    for (int c = 0; c < 6; ++c) blk[6 * a + c] = x[c];
}
// entry (a, b) of the target block -= L_ik L_jk^T: its six products one after the other
LB_FN void gb_update_entry(const double *Li, const double *Lj, double *dst, int a, int b) {
    double v = dst[6 * a + b];
LB_UNROLL
    for (int c = 0; c < 6; ++c) v = v - Li[6 * a + c] * Lj[6 * b + c];
    dst[6 * a + b] = v;
}
// the block (row i, column k) of L, i > k: a binary search in the ascending rows of column k.  The symbolic fill guarantees it exists
LB_FN int gb_block_of(const GbView &G, int i, int k) {
    int lo = G.col_ptr[k] + 1, hi = G.col_ptr[k + 1] - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (G.blk_row[mid] < i) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// update u of column j (b0 = col_ptr[j] + 1, m sub-diagonal blocks): the pair (qi >= qk) in the order (0,0) (1,0) (1,1) (2,0) ...
LB_FN void gb_update_pair(long long u, int &qi, int &qk) {
    long long r = (long long)((sqrt(8.0 * (double)u + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > u) --r;
    while ((r + 1) * (r + 2) / 2 <= u) ++r;
    qi = (int)r;
    qk = (int)(u - r * (r + 1) / 2);
}
// forward substitution inside block column j: L_jj y = r, in place
LB_FN void gb_fwd_diag(const double *Ljj, double *r) {
    double y[6];
LB_UNROLL
    for (int c = 0; c < 6; ++c) {
        double s = r[c];
LB_UNROLL
        for (int k = 0; k < c; ++k) s = s - Ljj[6 * c + k] * y[k];
        y[c] = s / Ljj[6 * c + c];
    }
LB_UNROLL
    for (int c = 0; c < 6; ++c) r[c] = y[c];
}
// ... and below it: entry a of r_i -= L_ij y_j
LB_FN void gb_fwd_row(const double *Lij, const double *y, double *ri, int a) {
    double s = ri[a];
LB_UNROLL
    for (int c = 0; c < 6; ++c) s = s - Lij[6 * a + c] * y[c];
    ri[a] = s;
}
// back substitution: entry a of r_j - sum_i L_ij^T x_i over the rows of column j in descending order
LB_FN double gb_back_gather(const GbView &G, const double *x, int j, int a) {
    double s = x[(size_t)j * 6 + a];
    for (int b = G.col_ptr[j + 1] - 1; b > G.col_ptr[j]; --b) {
        const double *Lij = G.L + (size_t)b * 36, *xi = x + (size_t)G.blk_row[b] * 6;
        for (int c = 5; c >= 0; --c) s = s - Lij[6 * c + a] * xi[c];
    }
    return s;
}
// ... and the block's own: L_jj^T x = s, descending
LB_FN void gb_back_diag(const double *Ljj, const double *s, double *xo) {
    double x[6];
LB_UNROLL
    for (int a = 5; a >= 0; --a) {
        double v = s[a];
LB_UNROLL
        for (int k = 5; k > a; --k) v = v - Ljj[6 * k + a] * x[k];
        x[a] = v / Ljj[6 * a + a];
    }
LB_UNROLL
    for (int a = 0; a < 6; ++a) xo[a] = x[a];
}

// LoopClosing.cc:731-750 in float, one rounding per operator: Xc = Rcw_before X + tcw_before, X' = Rwc_after Xc + twc_after.
// T: 12 floats, R row-major then t
LB_FN void gb_se3_apply(const float *T, const float *X, float *out) {
LB_UNROLL
    for (int r = 0; r < 3; ++r) out[r] = ((T[3 * r] * X[0] + T[3 * r + 1] * X[1]) + T[3 * r + 2] * X[2]) + T[9 + r];
}
LB_FN void gb_correct_se3(const float *T_before, const float *T_after, const float *X, float *out) {
    float c[3];
    gb_se3_apply(T_before, X, c);
    gb_se3_apply(T_after, c, out);
}
