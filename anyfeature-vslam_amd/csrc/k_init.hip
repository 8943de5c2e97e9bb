// k_init.hip — Initializer::Initialize (src/Initializer.cc:41-908) between two resident frames: from matches12 to (R21, t21, vP3D,
// vbTriangulated) in three launches (include/afv_hip.h, "Initializer"; host side: afv_init.hip).
//
//   k_init_prepare      one workgroup.  Compacts matches12 into the pairs (i1, i2) in ascending i1 (:52-61; ballot + popcount ranks, no
//                       atomics) and writes N; Normalize (:728-770) of both frames over ALL their keypoints; the 8-sets of every iteration
//                       (:74-91) without an N-sized list: 8 draws disturb at most 8 positions of availableIndices.
//   k_init_hypotheses   one wavefront per (model, iteration).  The DLT system of ComputeH21 / ComputeF21 in LDS, A^T A and the cyclic
//                       Jacobi on the 9 x 9 in double with the element updates of one rotation dealt to lanes (they are independent: the
//                       arithmetic order is the restatement's whatever the mapping), de-normalisation, then the lanes stride over the N
//                       matches of CheckHomography / CheckFundamental: a ballot is a 64-bit inlier word, the score a fixed-shape sum.
//   k_init_reconstruct  one workgroup.  Wavefronts 0 / 1 pick the winning iteration of H / F; lane 0 forms RH and builds the 8 motion
//                       hypotheses of ReconstructH or the 4 of ReconstructF; the 8 wavefronts run CheckRT (Triangulate = tri_null_vector
//                       of k_tri_match.h), one per motion hypothesis of H, two per motion hypothesis of F, and one per hypothesis selects
//                       the min(50, n - 1)-th smallest cosine by its key bits; lane 0 applies the accept / reject rules; the workgroup
//                       writes the outputs.
//   The stream orders the three launches: no flags, no spinning.
//
// The arithmetic is the restatement's (tests/_init_ref.py), statement for statement: float, one rounding per operator (the build's
// -ffp-contract=off; hipcc's correctly rounded divide and square root), a three-term sum as a0 + (a1 + a2), other scalar expressions left
// to right as written, A * B * C = (A * B) * C, det3 / inv3 by cofactors, double sums left to right.  PARITY UNPINNED.
// Quirks restated as written: CheckFundamental gates on 3.841 and scores with 5.991; CheckRT counts in nGood (and writes p3d for) points
// that fail cosParallax < minCos while isGood stays false; ReconstructF's else-if chain tests only the first hypothesis equal to maxGood;
// RH is NaN when both scores are 0 and goes to ReconstructF; ReconstructF counts inliers in a float, ReconstructH in an int.
// Deliberate deviations (the full text: include/afv_hip.h, tests/_init_ref.py):
//   I1  DLT null vector: A^T A in double, cyclic Jacobi 9 x 9 in double, <= 30 sweeps, smallest diagonal entry (ties: lowest index)
//   I2  svd3: V from the Jacobi on the 3 x 3 A^T A, descending order, u_0 = A v_0 / |A v_0|, u_1 likewise, u_2 = u_0 x u_1, v_2 negated
//       when (A v_2) . u_2 < 0
//   I3  ReconstructH negates A = K^-1 H21 K when det3(A) < 0
//   I4  counter-based draws (splitmix64) on availableIndices with swap-with-back; H and F share the sets
//   I5  fixed-shape sums: 256 partial sums + halving tree (Normalize), 64 partial sums + halving tree (the scores)
//   I6  no acosf: decisions on the selected cosine against float(cos(1 degree))
//   I7  N < 8: nothing is evaluated    I8  degenerate hypotheses score 0, are flagged, read 0    I9  no winner: zeros, index -1
//   I10 CheckRT skips x3Dh(3) == 0 and cosines that are not finite    I11 what is not written reads 0
#include "k_tri_match.h"

#define INIT_SWEEPS 30
#define INIT_RANK_GAP 1e-12
#define INIT_COS_MIN_PARALLAX 0.99984770f  // (float)cos(pi / 180)

__device__ __forceinline__ float i_sum3(float a0, float a1, float a2) { return a0 + (a1 + a2); }
__device__ __forceinline__ bool i_finite(float v) { return fabsf(v) <= 3.402823466e38f; }
__device__ __forceinline__ unsigned long long i_sm(unsigned long long x) {  // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// row-major 3 x 3
__device__ __forceinline__ void i_mm(const float (&A)[9], const float (&B)[9], float (&C)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = i_sum3(A[3 * r] * B[c], A[3 * r + 1] * B[3 + c], A[3 * r + 2] * B[6 + c]);
}
__device__ __forceinline__ void i_transpose(const float (&A)[9], float (&T)[9]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = A[3 * c + r];
}
__device__ __forceinline__ float i_det3(const float (&m)[9]) {
    const float c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    return i_sum3(m[0] * c0, m[1] * c1, m[2] * c2);
}
__device__ __forceinline__ void i_inv3(const float (&m)[9], float (&o)[9]) {
    const float c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const float i = 1.0f / i_sum3(m[0] * c0, m[1] * c1, m[2] * c2);
    o[0] = c0 * i; o[1] = (m[2] * m[7] - m[1] * m[8]) * i; o[2] = (m[1] * m[5] - m[2] * m[4]) * i;
    o[3] = c1 * i; o[4] = (m[0] * m[8] - m[2] * m[6]) * i; o[5] = (m[2] * m[3] - m[0] * m[5]) * i;
    o[6] = c2 * i; o[7] = (m[1] * m[6] - m[0] * m[7]) * i; o[8] = (m[0] * m[4] - m[1] * m[3]) * i;
}
__device__ __forceinline__ bool i_finite9(const float (&m)[9]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && i_finite(m[k]);
    return ok;
}
__device__ __forceinline__ void i_tmatrix(const float *nrm, float (&T)[9]) {  // Normalize's T (:763-768)
    T[0] = nrm[2]; T[1] = 0.0f; T[2] = -nrm[0] * nrm[2];
    T[3] = 0.0f; T[4] = nrm[3]; T[5] = -nrm[1] * nrm[3];
    T[6] = 0.0f; T[7] = 0.0f; T[8] = 1.0f;
}

// the rotation of S2 (k_sim3.hip): false = the pair is skipped
__device__ __forceinline__ bool i_rotation(double app, double aqq, double apq, double &c, double &s, double &t) {
    if (apq == 0.0) return false;
    const double g = fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
    return true;
}

// I2: one rotation of the 3 x 3, compile-time indices: everything stays in registers
template <int P, int Q>
__device__ __forceinline__ bool i_rotate3(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q], app = a[P][P], aqq = a[Q][Q];
    double c, s, t;
    if (!i_rotation(app, aqq, apq, c, s, t)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
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
    for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
    return true;
}

template <int I, int K>
__device__ __forceinline__ void i_order3(double (&d)[3], double (&v)[3][3]) {
    if (d[I] < d[K]) {
        const double td = d[I]; d[I] = d[K]; d[K] = td;
#pragma unroll
        for (int r = 0; r < 3; ++r) { const double tv = v[r][I]; v[r][I] = v[r][K]; v[r][K] = tv; }
    }
}

// I2: U, w, V of a row-major 3 x 3 (the COLUMNS of U and V are the vectors)
__device__ __forceinline__ void i_svd3(const float (&A)[9], float (&U)[9], float (&w)[3], float (&V)[9]) {
    double a[3][3], m[3][3], v[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[r][c] = (double)A[3 * r + c]; v[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) s = s + a[r][i] * a[r][j];
            m[i][j] = s;
        }
    for (int sweep = 0; sweep < INIT_SWEEPS; ++sweep) {
        bool any = i_rotate3<0, 1>(m, v);
        any |= i_rotate3<0, 2>(m, v);
        any |= i_rotate3<1, 2>(m, v);
        if (!any) break;
    }
    double d[3] = {m[0][0], m[1][1], m[2][2]};
    i_order3<0, 1>(d, v);
    i_order3<0, 2>(d, v);
    i_order3<1, 2>(d, v);
    double b[3][3], wd[3];  // b[k] = A v_k
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int r = 0; r < 3; ++r) b[k][r] = (a[r][0] * v[0][k] + a[r][1] * v[1][k]) + a[r][2] * v[2][k];
        wd[k] = sqrt((b[k][0] * b[k][0] + b[k][1] * b[k][1]) + b[k][2] * b[k][2]);
    }
    double u[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { u[0][r] = b[0][r] / wd[0]; u[1][r] = b[1][r] / wd[1]; }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    const bool flip = (b[2][0] * u[2][0] + b[2][1] * u[2][1]) + b[2][2] * u[2][2] < 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            U[3 * r + c] = (float)u[c][r];
            V[3 * r + c] = (float)((c == 2 && flip) ? -v[r][c] : v[r][c]);
        }
        w[r] = (float)wd[r];
    }
}

__device__ __forceinline__ float i_block_sum(float v, float *red, int tid) {  // I5: the halving tree over AFV_INIT_PREP_T partial sums
    red[tid] = v;
    __syncthreads();
    for (int s = AFV_INIT_PREP_T / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(AFV_INIT_PREP_T) void k_init_prepare(const DevInitArgs A) {
    __shared__ int s_wave[AFV_INIT_PREP_T / 64];
    __shared__ float s_red[AFV_INIT_PREP_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < A.n1; i0 += AFV_INIT_PREP_T) {  // :52-61
        const int i1 = i0 + tid;
        const int m = i1 < A.n1 ? A.matches12[i1] : -1;
        const bool keep = m >= 0 && m < A.n2;
        const unsigned long long b = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int rank = base + __popcll(b & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < AFV_INIT_PREP_T / 64; ++w) {
            if (w < wave) rank += s_wave[w];
            total += s_wave[w];
        }
        if (keep) { A.pairs[2 * rank] = i1; A.pairs[2 * rank + 1] = m; }
        base += total;
        __syncthreads();
    }
    const int N = base;
    if (tid == 0) A.n[0] = N;
    for (int f = 0; f < 2; ++f) {  // Normalize (:728-770) over all keypoints of the frame
        const float *x = f ? A.x2 : A.x1, *y = f ? A.y2 : A.y1;
        const int n = f ? A.n2 : A.n1;
        const float nf = (float)n;
        float px = 0.0f, py = 0.0f;
        for (int i0 = 0; i0 < n; i0 += AFV_INIT_PREP_T) {
            const int i = i0 + tid;
            px = px + (i < n ? x[i] : 0.0f);
            py = py + (i < n ? y[i] : 0.0f);
        }
        const float mx = i_block_sum(px, s_red, tid) / nf, my = i_block_sum(py, s_red, tid) / nf;
        px = 0.0f; py = 0.0f;
        for (int i0 = 0; i0 < n; i0 += AFV_INIT_PREP_T) {
            const int i = i0 + tid;
            px = px + (i < n ? fabsf(x[i] - mx) : 0.0f);
            py = py + (i < n ? fabsf(y[i] - my) : 0.0f);
        }
        const float dx = i_block_sum(px, s_red, tid) / nf, dy = i_block_sum(py, s_red, tid) / nf;
        if (tid == 0) {
            A.norm[4 * f] = mx; A.norm[4 * f + 1] = my;
            A.norm[4 * f + 2] = 1.0f / dx; A.norm[4 * f + 3] = 1.0f / dy;
        }
    }
    if (N < 8) return;  // I7
    for (int h = tid; h < A.iterations; h += AFV_INIT_PREP_T) {  // I4 (:74-91)
        const unsigned long long key = i_sm(i_sm(A.seed) ^ (unsigned long long)(h + 1));
        int pos[8], val[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int r = (int)(i_sm(key + (unsigned long long)(d + 1) * 0xD1342543DE82EF95ull) % (unsigned long long)(N - d));
            const int b = N - 1 - d;
            int pick = r, back = b, slot = -1;
#pragma unroll
            for (int j = 0; j < d; ++j) {
                if (pos[j] == r) { pick = val[j]; slot = j; }
                if (pos[j] == b) back = val[j];
            }
            A.sets[8 * h + d] = pick;
            pos[d] = slot < 0 ? r : -1;  // availableIndices[randi] = availableIndices.back()
            val[d] = back;
#pragma unroll
            for (int j = 0; j < d; ++j)
                if (j == slot) val[j] = back;
        }
    }
}

__global__ __launch_bounds__(64) void k_init_hypotheses(const DevInitArgs A) {
    __shared__ float s_A[16][9];
    __shared__ double s_M[9][9], s_V[9][9];
    const int lane = threadIdx.x, h = blockIdx.x, model = blockIdx.y;
    const size_t ho = (size_t)model * A.iterations + h;
    const int N = min(A.n[0], A.n1), chunks = (A.mask_words + 1) >> 1;
    uint32_t *words = A.inliers + ho * A.mask_words;
    bool ok = N >= 8;  // I7
    bool deficient = false;
    float Mo[9], Mi[9];  // H21 and H12, or F21
#pragma unroll
    for (int k = 0; k < 9; ++k) { Mo[k] = 0.0f; Mi[k] = 0.0f; }
    if (ok) {  // block-uniform
        const int nrows = model == AFV_INIT_ROUTE_H ? 16 : 8;
        if (lane < 8) {
            const int k = A.sets[8 * h + lane];
            const int i1 = A.pairs[2 * k], i2 = A.pairs[2 * k + 1];
            const float u1 = (A.x1[i1] - A.norm[0]) * A.norm[2], v1 = (A.y1[i1] - A.norm[1]) * A.norm[3];
            const float u2 = (A.x2[i2] - A.norm[4]) * A.norm[6], v2 = (A.y2[i2] - A.norm[5]) * A.norm[7];
            if (model == AFV_INIT_ROUTE_H) {  // ComputeH21 (:223-251)
                float *r0 = s_A[2 * lane], *r1 = s_A[2 * lane + 1];
                r0[0] = 0.0f; r0[1] = 0.0f; r0[2] = 0.0f; r0[3] = -u1; r0[4] = -v1; r0[5] = -1.0f; r0[6] = v2 * u1; r0[7] = v2 * v1; r0[8] = v2;
                r1[0] = u1; r1[1] = v1; r1[2] = 1.0f; r1[3] = 0.0f; r1[4] = 0.0f; r1[5] = 0.0f; r1[6] = -u2 * u1; r1[7] = -u2 * v1; r1[8] = -u2;
            } else {  // ComputeF21 (:265-281)
                float *r0 = s_A[lane];
                r0[0] = u2 * u1; r0[1] = u2 * v1; r0[2] = u2; r0[3] = v2 * u1; r0[4] = v2 * v1; r0[5] = v2; r0[6] = u1; r0[7] = v1; r0[8] = 1.0f;
            }
        }
        __syncthreads();
        for (int e = lane; e < 81; e += 64) {  // I1: A^T A, running sums over the rows
            const int i = e / 9, j = e - 9 * i;
            double s = 0.0;
            for (int r = 0; r < nrows; ++r) s = s + (double)s_A[r][i] * (double)s_A[r][j];
            s_M[i][j] = s;
            s_V[i][j] = i == j ? 1.0 : 0.0;
        }
        __syncthreads();
        for (int sweep = 0; sweep < INIT_SWEEPS; ++sweep) {
            bool rotated = false;
            for (int p = 0; p < 8; ++p)
                for (int q = p + 1; q < 9; ++q) {
                    const double apq = s_M[p][q], app = s_M[p][p], aqq = s_M[q][q];
                    double c, s, t;
                    const bool turn = i_rotation(app, aqq, apq, c, s, t);  // wavefront-uniform
                    __syncthreads();
                    if (turn) {
                        rotated = true;
                        if (lane < 9) {  // row / column `lane` of the matrix
                            if (lane != p && lane != q) {
                                const double akp = s_M[lane][p], akq = s_M[lane][q];
                                const double np = c * akp - s * akq, nq = s * akp + c * akq;
                                s_M[lane][p] = np; s_M[p][lane] = np;
                                s_M[lane][q] = nq; s_M[q][lane] = nq;
                            }
                        } else if (lane < 18) {  // row lane - 9 of V
                            const int k = lane - 9;
                            const double vkp = s_V[k][p], vkq = s_V[k][q];
                            s_V[k][p] = c * vkp - s * vkq;
                            s_V[k][q] = s * vkp + c * vkq;
                        } else if (lane == 18) {
                            s_M[p][p] = app - t * apq;
                            s_M[q][q] = aqq + t * apq;
                            s_M[p][q] = 0.0; s_M[q][p] = 0.0;
                        }
                    }
                    __syncthreads();
                }
            if (!rotated) break;
        }
        int lo = 0;
        double dlo = s_M[0][0], largest = s_M[0][0];
        for (int k = 1; k < 9; ++k) {
            const double d = s_M[k][k];
            if (d < dlo) { dlo = d; lo = k; }
            if (d > largest) largest = d;
        }
        double second = 0.0;
        bool have = false;
        for (int k = 0; k < 9; ++k) {
            const double d = s_M[k][k];
            if (k != lo && (!have || d < second)) { second = d; have = true; }
        }
        deficient = !(second > INIT_RANK_GAP * largest);  // I8
        float nv[9], T1[9], T2[9], X[9], Y[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) nv[k] = (float)s_V[k][lo];
        i_tmatrix(A.norm, T1);
        i_tmatrix(A.norm + 4, T2);
        if (model == AFV_INIT_ROUTE_H) {  // :151-153
            i_inv3(T2, X);
            i_mm(X, nv, Y);
            i_mm(Y, T1, Mo);
            i_inv3(Mo, Mi);
            ok = !deficient && i_finite9(Mo) && i_finite9(Mi);
        } else {  // :285-292, :203
            float U[9], w[3], V[9], UD[9], Vt[9], Fn[9];
            i_svd3(nv, U, w, V);
#pragma unroll
            for (int r = 0; r < 3; ++r) { UD[3 * r] = U[3 * r] * w[0]; UD[3 * r + 1] = U[3 * r + 1] * w[1]; UD[3 * r + 2] = U[3 * r + 2] * 0.0f; }
            i_transpose(V, Vt);
            i_mm(UD, Vt, Fn);
            i_transpose(T2, X);
            i_mm(X, Fn, Y);
            i_mm(Y, T1, Mo);
            ok = !deficient && i_finite9(Mo);
        }
    }
    if (lane == 0) A.degenerate[ho] = (N >= 8 && !ok) ? 1 : 0;
    if (lane < 9) {
        float val = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            if (lane == k && ok) val = Mo[k];
        A.model[ho * 9 + lane] = val;
    }
    const float inv_s2 = 1.0f / (A.sigma * A.sigma);
    float part = 0.0f;
    for (int j = 0; j < chunks; ++j) {
        const int k = j * 64 + lane;
        bool in = false;
        float e = 0.0f;
        if (ok && k < N) {
            const int i1 = A.pairs[2 * k], i2 = A.pairs[2 * k + 1];
            const float u1 = A.x1[i1], v1 = A.y1[i1], u2 = A.x2[i2], v2 = A.y2[i2];
            float chi1, chi2, gate, th;
            if (model == AFV_INIT_ROUTE_H) {  // CheckHomography (:324-372)
                float w = 1.0f / i_sum3(Mi[6] * u2, Mi[7] * v2, Mi[8]);
                float a = i_sum3(Mi[0] * u2, Mi[1] * v2, Mi[2]) * w, b = i_sum3(Mi[3] * u2, Mi[4] * v2, Mi[5]) * w;
                chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2;
                w = 1.0f / i_sum3(Mo[6] * u1, Mo[7] * v1, Mo[8]);
                a = i_sum3(Mo[0] * u1, Mo[1] * v1, Mo[2]) * w; b = i_sum3(Mo[3] * u1, Mo[4] * v1, Mo[5]) * w;
                chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2;
                gate = 5.991f; th = 5.991f;
            } else {  // CheckFundamental (:396-448)
                const float a2 = i_sum3(Mo[0] * u1, Mo[1] * v1, Mo[2]), b2 = i_sum3(Mo[3] * u1, Mo[4] * v1, Mo[5]), c2 = i_sum3(Mo[6] * u1, Mo[7] * v1, Mo[8]);
                const float num2 = i_sum3(a2 * u2, b2 * v2, c2);
                chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_s2;
                const float a1 = i_sum3(Mo[0] * u2, Mo[3] * v2, Mo[6]), b1 = i_sum3(Mo[1] * u2, Mo[4] * v2, Mo[7]), c1 = i_sum3(Mo[2] * u2, Mo[5] * v2, Mo[8]);
                const float num1 = i_sum3(a1 * u1, b1 * v1, c1);
                chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_s2;
                gate = 3.841f; th = 5.991f;
            }
            const bool in1 = i_finite(chi1) && !(chi1 > gate), in2 = i_finite(chi2) && !(chi2 > gate);  // I8
            e = (in1 ? th - chi1 : 0.0f) + (in2 ? th - chi2 : 0.0f);
            in = in1 && in2;
        }
        part = part + e;  // I5
        const unsigned long long m = __ballot(in);
        if (lane == 0) words[2 * j] = (uint32_t)m;
        if (lane == 1 && 2 * j + 1 < A.mask_words) words[2 * j + 1] = (uint32_t)(m >> 32);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) part = part + __shfl_down(part, s);
    if (lane == 0) A.score[ho] = ok ? part : 0.0f;
}

// CheckRT (:773-884) of motion hypothesis w, first half: the lanes stride over the matches; wavefront `sub` of the `waves` that share the
// hypothesis takes every waves-th chunk of 64 matches (the matches are independent of each other).  -> this wavefront's part of nGood
__device__ __forceinline__ int i_check_rt(const DevInitArgs &A, const float *R, const float *t, const uint32_t *words, int N, int chunks, int w,
                                          int sub, int waves, int lane) {
    const float th2 = 4.0f * (A.sigma * A.sigma);
    const float K[9] = {A.fx, 0.0f, A.cx, 0.0f, A.fy, A.cy, 0.0f, 0.0f, 1.0f};
    const float P1[3][4] = {{A.fx, 0.0f, A.cx, 0.0f}, {0.0f, A.fy, A.cy, 0.0f}, {0.0f, 0.0f, 1.0f, 0.0f}};
    float P2[3][4], O2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float r0 = c < 3 ? R[c] : t[0], r1 = c < 3 ? R[3 + c] : t[1], r2 = c < 3 ? R[6 + c] : t[2];
            P2[r][c] = i_sum3(K[3 * r] * r0, K[3 * r + 1] * r1, K[3 * r + 2] * r2);
        }
#pragma unroll
    for (int r = 0; r < 3; ++r) O2[r] = i_sum3(-R[r] * t[0], -R[3 + r] * t[1], -R[6 + r] * t[2]);
    const size_t row = (size_t)w * A.n1;
    int n_good = 0;
    for (int j = sub; j < chunks; j += waves) {
        const int k = j * 64 + lane;
        unsigned st = 0;
        if (k < N && words && ((words[k >> 5] >> (k & 31)) & 1u)) {
            const int i1 = A.pairs[2 * k], i2 = A.pairs[2 * k + 1];
            const float kx1 = A.x1[i1], ky1 = A.y1[i1], kx2 = A.x2[i2], ky2 = A.y2[i2];
            float At[4][4], v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {  // Triangulate (:709-713), A transposed
                At[c][0] = kx1 * P1[2][c] - P1[0][c];
                At[c][1] = ky1 * P1[2][c] - P1[1][c];
                At[c][2] = kx2 * P2[2][c] - P2[0][c];
                At[c][3] = ky2 * P2[2][c] - P2[1][c];
            }
            tri_null_vector(At, v);
            bool go = v[3] != 0;  // I10
            const float p0 = v[0] / v[3], p1 = v[1] / v[3], p2 = v[2] / v[3];
            go = go && i_finite(p0) && i_finite(p1) && i_finite(p2);
            const float dist1 = sqrtf(i_sum3(p0 * p0, p1 * p1, p2 * p2));
            const float n0 = p0 - O2[0], n1 = p1 - O2[1], n2 = p2 - O2[2];
            const float dist2 = sqrtf(i_sum3(n0 * n0, n1 * n1, n2 * n2));
            const float cosp = i_sum3(p0 * n0, p1 * n1, p2 * n2) / (dist1 * dist2);
            go = go && i_finite(cosp);  // I10
            go = go && !(p2 <= 0 && cosp < 0.99998f);
            const float q0 = i_sum3(R[0] * p0, R[1] * p1, R[2] * p2) + t[0], q1 = i_sum3(R[3] * p0, R[4] * p1, R[5] * p2) + t[1];
            const float q2 = i_sum3(R[6] * p0, R[7] * p1, R[8] * p2) + t[2];
            go = go && !(q2 <= 0 && cosp < 0.99998f);
            float iz = 1.0f / p2;
            float ex = (A.fx * p0 * iz + A.cx) - kx1, ey = (A.fy * p1 * iz + A.cy) - ky1;
            go = go && !(ex * ex + ey * ey > th2);
            iz = 1.0f / q2;
            ex = (A.fx * q0 * iz + A.cx) - kx2; ey = (A.fy * q1 * iz + A.cy) - ky2;
            go = go && !(ex * ex + ey * ey > th2);
            if (go) {
                st = cosp < 0.99998f ? 3u : 1u;  // nGood counts it either way (:865-870)
                A.cosv[row + k] = cosp;
                A.p3dk[3 * (row + k)] = p0; A.p3dk[3 * (row + k) + 1] = p1; A.p3dk[3 * (row + k) + 2] = p2;
            }
        }
        if (k < N) A.status[row + k] = (uint8_t)st;
        n_good += __popcll(__ballot(st != 0));
    }
    return n_good;
}

// a float as a 32-bit key of the same order, and back
__device__ __forceinline__ unsigned i_key(float f) {
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float i_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }

// :157 / :207 over all iterations by one wavefront: the lowest index that holds the maximum above 0, -1 = none (I9)
__device__ __forceinline__ void i_select(const float *score, int iterations, int lane, int &best, float &S) {
    best = -1; S = 0.0f;
    for (int h = lane; h < iterations; h += 64) {
        const float s = score[h];
        if (s > S) { S = s; best = h; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float so = __shfl_down(S, d);
        const int bo = __shfl_down(best, d);
        if (bo >= 0 && (so > S || (so == S && (best < 0 || bo < best)))) { S = so; best = bo; }
    }
    best = __shfl(best, 0);
    S = __shfl(S, 0);
}

__global__ __launch_bounds__(AFV_INIT_REC_T) void k_init_reconstruct(const DevInitArgs A) {
    __shared__ float s_R[AFV_INIT_MAX_MOTIONS][9], s_t[AFV_INIT_MAX_MOTIONS][3], s_cos[AFV_INIT_MAX_MOTIONS], s_S[2], s_model[2][9];
    __shared__ int s_good[AFV_INIT_MAX_MOTIONS], s_part[AFV_INIT_REC_T / 64], s_best[2], s_nm, s_route, s_reason, s_pick, s_ninl;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int N = min(A.n[0], A.n1), chunks = (A.mask_words + 1) >> 1;
    afv_init_trace &T = *A.trace;
    if (w < 2) {
        int best = -1;
        float S = 0.0f;
        if (N >= 8) i_select(A.score + (size_t)w * A.iterations, A.iterations, lane, best, S);
        if (lane == 0) { s_best[w] = best; s_S[w] = S; }
        if (lane < 9) s_model[w][lane] = best >= 0 ? A.model[((size_t)w * A.iterations + best) * 9 + lane] : 0.0f;
    }
    if (tid == 0) { s_nm = 0; s_route = AFV_INIT_ROUTE_F; s_reason = AFV_INIT_TOO_FEW_MATCHES; s_pick = -1; s_ninl = 0; }
    __syncthreads();
    const int route = (N >= 8 && s_S[0] / (s_S[0] + s_S[1]) > 0.4f) ? AFV_INIT_ROUTE_H : AFV_INIT_ROUTE_F;  // :105-112
    const int best = s_best[route];
    const uint32_t *words = best >= 0 ? A.inliers + ((size_t)route * A.iterations + best) * A.mask_words : nullptr;
    if (tid == 0 && N >= 8) {
        int ninl = 0;
        if (words)
            for (int k = 0; k < A.mask_words; ++k) ninl += __popc(words[k]);
        float M[9], Km[9] = {A.fx, 0.0f, A.cx, 0.0f, A.fy, A.cy, 0.0f, 0.0f, 1.0f}, X[9], Y[9], U[9], wv[3], V[9], Vt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) M[k] = s_model[route][k];
        int nm = 0, reason = AFV_INIT_OK;
        if (route == AFV_INIT_ROUTE_F) {  // ReconstructF (:466-472), DecomposeE (:886-908)
            float E[9], UW[9];
            i_transpose(Km, X);
            i_mm(X, M, Y);
            i_mm(Y, Km, E);
            i_svd3(E, U, wv, V);
            i_transpose(V, Vt);
            float t0 = U[2], t1 = U[5], t2 = U[8];
            const float nrm = sqrtf(i_sum3(t0 * t0, t1 * t1, t2 * t2));
            t0 = t0 / nrm; t1 = t1 / nrm; t2 = t2 / nrm;
            for (int v = 0; v < 2; ++v) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {  // U * W, U * W^T
                    UW[3 * r] = v ? -U[3 * r + 1] : U[3 * r + 1];
                    UW[3 * r + 1] = v ? U[3 * r] : -U[3 * r];
                    UW[3 * r + 2] = U[3 * r + 2];
                }
                float Rv[9];
                i_mm(UW, Vt, Rv);
                const bool flip = i_det3(Rv) < 0;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const float val = flip ? -Rv[k] : Rv[k];
                    s_R[v][k] = val; s_R[v + 2][k] = val;
                }
            }
            for (int v = 0; v < 2; ++v) {
                s_t[v][0] = t0; s_t[v][1] = t1; s_t[v][2] = t2;
                s_t[v + 2][0] = -t0; s_t[v + 2][1] = -t1; s_t[v + 2][2] = -t2;
            }
            nm = 4;
        } else {  // ReconstructH (:567-655)
            float Am[9];
            i_inv3(Km, X);
            i_mm(X, M, Y);
            i_mm(Y, Km, Am);
            if (i_det3(Am) < 0) {  // I3
#pragma unroll
                for (int k = 0; k < 9; ++k) Am[k] = -Am[k];
            }
            i_svd3(Am, U, wv, V);
            i_transpose(V, Vt);
            const float s = i_det3(U) * i_det3(Vt);
            const float d1 = wv[0], d2 = wv[1], d3 = wv[2];
            if (d1 / d2 < 1.00001f || d2 / d3 < 1.00001f) {
                reason = AFV_INIT_D_RATIO;
            } else {
                const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
                const float aux_st = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
                const float ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
                const float aux_sp = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
                const float cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
                float sU[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) sU[k] = s * U[k];
                for (int i = 0; i < 8; ++i) {
                    const int e = i & 3;
                    const float x1 = e < 2 ? aux1 : -aux1, x3 = (e & 1) ? -aux3 : aux3;
                    const bool second = i >= 4;
                    const float st = (e == 0 || e == 3) ? (second ? aux_sp : aux_st) : (second ? -aux_sp : -aux_st);
                    float Rp[9] = {ct, 0.0f, -st, 0.0f, 1.0f, 0.0f, st, 0.0f, ct};
                    if (second) { Rp[0] = cp; Rp[2] = st; Rp[4] = -1.0f; Rp[6] = st; Rp[8] = -cp; }
                    float Rv[9];
                    i_mm(sU, Rp, X);
                    i_mm(X, Vt, Rv);
                    const float m = second ? d1 + d3 : d1 - d3;
                    const float tp0 = x1 * m, tp1 = 0.0f * m, tp2 = (second ? x3 : -x3) * m;
                    float tv[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) tv[r] = i_sum3(U[3 * r] * tp0, U[3 * r + 1] * tp1, U[3 * r + 2] * tp2);
                    const float nrm = sqrtf(i_sum3(tv[0] * tv[0], tv[1] * tv[1], tv[2] * tv[2]));
#pragma unroll
                    for (int k = 0; k < 9; ++k) s_R[i][k] = Rv[k];
#pragma unroll
                    for (int r = 0; r < 3; ++r) s_t[i][r] = tv[r] / nrm;
                }
                nm = 8;
            }
        }
        s_nm = nm; s_route = route; s_reason = reason; s_ninl = ninl;
    }
    __syncthreads();
    const int nm = s_nm;
    const int waves = nm > 0 ? (AFV_INIT_REC_T / 64) / nm : 1;  // wavefronts per motion hypothesis: 2 of ReconstructF's 4, 1 of ReconstructH's 8
    const int hyp = w / waves, sub = w - hyp * waves;
    {
        int part = 0;
        if (hyp < nm) part = i_check_rt(A, s_R[hyp], s_t[hyp], words, N, chunks, hyp, sub, waves, lane);
        if (lane == 0) s_part[w] = part;
    }
    __syncthreads();
    if (hyp < nm && sub == 0) {
        // I6: the min(50, n - 1)-th smallest of the pushed cosines.  The cosines as order-preserving 32-bit keys; the key of that entry is
        // the largest K with fewer than want + 1 keys below it, found bit by bit from the top: 32 counting passes over the wavefront's rows
        const size_t row = (size_t)hyp * A.n1;
        int n_good = 0;
        for (int k = 0; k < waves; ++k) n_good += s_part[hyp * waves + k];
        const int want = min(50, n_good - 1);
        unsigned prefix = 0;
        if (n_good > 0)
            for (int b = 31; b >= 0; --b) {
                const unsigned trial = prefix | (1u << b);
                int below = 0;
                for (int j = 0; j < chunks; ++j) {
                    const int k = j * 64 + lane;
                    if (k < N && (A.status[row + k] & 1)) below += i_key(A.cosv[row + k]) < trial ? 1 : 0;
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) below += __shfl_xor(below, d);
                if (below <= want) prefix = trial;
            }
        if (lane == 0) {
            s_good[hyp] = n_good;
            s_cos[hyp] = n_good > 0 ? i_unkey(prefix) : 1.0f;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int reason = s_reason, pick = -1;
        if (N >= 8 && reason == AFV_INIT_OK) {
            if (s_route == AFV_INIT_ROUTE_F) {  // :459-463, :484-547
                float Nf = 0.0f;
                for (int k = 0; k < s_ninl; ++k) Nf = Nf + 1.0f;
                const int g[4] = {s_good[0], s_good[1], s_good[2], s_good[3]};
                const int max_good = max(g[0], max(g[1], max(g[2], g[3])));
                const int n_min_good = max((int)(0.9f * Nf), 50);
                int nsimilar = 0, first = 3;
#pragma unroll
                for (int k = 3; k >= 0; --k) {
                    if ((float)g[k] > 0.7f * (float)max_good) nsimilar++;
                    if (g[k] == max_good) first = k;
                }
                if (max_good < n_min_good) reason = max_good < 50 ? AFV_INIT_MIN_TRIANGULATED : AFV_INIT_MIN_GOOD;
                else if (nsimilar > 1) reason = AFV_INIT_AMBIGUOUS;
                else if (s_cos[first] < INIT_COS_MIN_PARALLAX) pick = first;
                else reason = AFV_INIT_PARALLAX;
            } else {  // :658-703
                int best_good = 0, second = 0, bi = -1;
                float best_cos = 2.0f;
                for (int i = 0; i < 8; ++i) {
                    const int g = s_good[i];
                    if (g > best_good) { second = best_good; best_good = g; bi = i; best_cos = s_cos[i]; }
                    else if (g > second) second = g;
                }
                if (!((float)second < 0.75f * (float)best_good)) reason = AFV_INIT_AMBIGUOUS;
                else if (!(best_cos <= INIT_COS_MIN_PARALLAX)) reason = AFV_INIT_PARALLAX;
                else if (!((float)best_good > (float)50)) reason = AFV_INIT_MIN_TRIANGULATED;
                else if (!((float)best_good > 0.9f * (float)s_ninl)) reason = AFV_INIT_MIN_GOOD;
                else pick = bi;
            }
        }
        s_pick = pick;
        const bool live = N >= 8;
        T.n = N;
        T.sh = live ? s_S[0] : 0.0f; T.sf = live ? s_S[1] : 0.0f;
        T.rh = live ? s_S[0] / (s_S[0] + s_S[1]) : 0.0f;
        T.best_h = live ? s_best[0] : -1; T.best_f = live ? s_best[1] : -1;
        float T1[9], T2[9];
        i_tmatrix(A.norm, T1);
        i_tmatrix(A.norm + 4, T2);
        for (int k = 0; k < 9; ++k) {
            T.h21[k] = live ? s_model[0][k] : 0.0f; T.f21[k] = live ? s_model[1][k] : 0.0f;
            T.T1[k] = live ? T1[k] : 0.0f; T.T2[k] = live ? T2[k] : 0.0f;
        }
        T.route = s_route; T.n_inliers = s_ninl; T.n_motion = nm; T.best_motion = pick; T.reason = reason;
        for (int i = 0; i < AFV_INIT_MAX_MOTIONS; ++i) {
            const bool have = i < nm;
            T.n_good[i] = have ? s_good[i] : 0;
            T.cos_parallax[i] = have ? s_cos[i] : 0.0f;
            for (int k = 0; k < 9; ++k) T.R[i][k] = have ? s_R[i][k] : 0.0f;
            for (int k = 0; k < 3; ++k) T.t[i][k] = have ? s_t[i][k] : 0.0f;
        }
        A.answer[0] = pick >= 0 ? 1 : 0;
        A.answer[1] = s_route;
        for (int k = 0; k < 9; ++k) A.Rt[k] = pick >= 0 ? s_R[pick][k] : 0.0f;
        for (int k = 0; k < 3; ++k) A.Rt[9 + k] = pick >= 0 ? s_t[pick][k] : 0.0f;
    }
    __syncthreads();
    const int pick = s_pick;  // I11
    for (int i = tid; i < A.n1; i += AFV_INIT_REC_T) {
        const int m = A.matches12[i];
        if (!(m >= 0 && m < A.n2)) {  // rows of matched features are written below: no row is written twice
            A.p3d[3 * i] = 0.0f; A.p3d[3 * i + 1] = 0.0f; A.p3d[3 * i + 2] = 0.0f;
            A.triangulated[i] = 0;
        }
    }
    for (int k = tid; k < N; k += AFV_INIT_REC_T) {
        const int i1 = A.pairs[2 * k];
        unsigned st = 0;
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
        if (pick >= 0) {
            const size_t o = (size_t)pick * A.n1 + k;
            st = A.status[o];
            if (st & 1) { p0 = A.p3dk[3 * o]; p1 = A.p3dk[3 * o + 1]; p2 = A.p3dk[3 * o + 2]; }
        }
        A.p3d[3 * i1] = p0; A.p3d[3 * i1 + 1] = p1; A.p3d[3 * i1 + 2] = p2;
        A.triangulated[i1] = (uint8_t)((st >> 1) & 1);
    }
}

extern "C" void afv_launch_init(const DevInitArgs *args, hipStream_t stream) {
    hipLaunchKernelGGL(k_init_prepare, dim3(1), dim3(AFV_INIT_PREP_T), 0, stream, *args);
    hipLaunchKernelGGL(k_init_hypotheses, dim3(args->iterations, 2), dim3(64), 0, stream, *args);
    hipLaunchKernelGGL(k_init_reconstruct, dim3(1), dim3(AFV_INIT_REC_T), 0, stream, *args);
}
