// k_pnp.hip — PnPsolver (src/PnPsolver.cc:67-950) over a resident frame and ids of the map-point store: the constructor, ALL EPnP RANSAC
// hypotheses and the refinement of every record, for every candidate of a relocalisation (include/afv_hip.h, "PnPsolver"; host side:
// afv_pnp.hip).
//
//   k_pnp_gather      one workgroup per candidate.  Keeps feature i when pts[c][i] >= 0, was set in the store and is not bad, compacts the
//                     survivors in feature order (ballot + popcount ranks, a workgroup prefix, no atomics: k_sim3_gather's compaction,
//                     restated here because sharing it would mean editing k_sim3.hip) and writes mvKeyPointIndices, mvP2D, mvP3Dw,
//                     mvMaxError, N and mRansacMinInliers.
//   k_pnp_hypotheses  one wavefront per (candidate, hypothesis h): the four draws from the device-side N, EPnP on them, then the lanes
//                     stride over the N correspondences: a ballot is a 64-bit inlier word, its popcount the count.
//   k_pnp_refine      one wavefront per (candidate, hypothesis h): the lanes take the maximum of count[c][0 .. h) and the wavefront leaves
//                     unless h is a record (count >= min_inliers and > every earlier count); else EPnP over h's inliers, enumerated in
//                     correspondence order from its inlier words, and CheckInliers again.  The stream orders the three launches: no
//                     flag, no spinning, no grid barrier.
//
// One EPnP (p_epnp) serves both callers: a device function over "the selected correspondences" (4, or up to N).  alphas and pcs are not
// stored per correspondence; they are recomputed where they are used, which yields the same bits each time.  Everything between the sums
// is wavefront-uniform double arithmetic; the 12 x 12 Jacobi keeps the matrix and V in LDS and deals the element updates of a rotation to
// lanes as k_init_hypotheses does for its 9 x 9.
//
// The arithmetic is the restatement's (tests/_pnp_ref.py), statement for statement: double, one rounding per operator (the build's
// -ffp-contract=off; correctly rounded divide and square root), scalar expressions left to right as written.  PARITY UNPINNED.
// Quirks restated as written:
//   Q1-Q4  the loop of iterate, pow(epsilon, 3), > / > / >= and Refine on the best set: host (the Python class)
//   Q5  CheckInliers: Xc, Yc, invZc are floats of double expressions, ue / ve double, distX / distY / error2 float
//   Q6  solve_for_sign looks at the first selected correspondence only
// Deliberate deviations:
//   E1  eigenvectors of M^T M: cyclic Jacobi on the symmetric 12 x 12 in double, pairs (0,1) (0,2) ... (10,11), + - * / sqrt only, at
//       most 30 sweeps, S2's skip and stop rules; columns by descending diagonal entry, ties to the lowest index; signs as left
//   E2  PCA of the points: the same Jacobi on the 3 x 3       E3  the inverse of CC by cofactors
//   E4  the three least-squares systems through qr_solve (:860-950), as Gauss-Newton's
//   E5  the SVD of ABt: V from the Jacobi on A^T A, u_0, u_1 = A v / |A v|, u_2 = u_0 x u_1, v_2 negated when (A v_2) . u_2 < 0
//   E6  draws: key_h = sm(sm(seed) ^ (h + 1)), draw d = sm(key_h + (d + 1) * DRAW_STEP) % (N - d), swap-with-back
//   E7  every sum over the selected correspondences: 64 partial sums (lane l: elements l, l + 64, ...), then p[l] += p[l + s], s = 32 .. 1
//   E8  degenerate: qr_solve meets eta == 0, a betas[0] that is divided by is 0, R or t of the chosen approximation not finite: 0
//       inliers, flagged, pose and words 0; an error that is not finite loses the comparison / is no inlier.  Coplanar 4-sets: no rule
//   E9  N < 4: nothing is evaluated    E10 what is not written reads 0
#include "afv_device.h"
#include "afv_runtime.h"

#define PNP_T AFV_PNP_T
#define PNP_WAVES (PNP_T / 64)
#define PNP_SWEEPS 30
#define PNP_MAX_SEL (32 * AFV_PNP_MAX_MASK_WORDS)

__device__ __forceinline__ bool p_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ unsigned long long p_sm(unsigned long long x) {  // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(PNP_T) void k_pnp_gather(const DevPnpArgs A) {
    __shared__ int s_wave[PNP_WAVES];
    const int tid = threadIdx.x, c = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const DevPnpCand &J = A.cands[c];
    const size_t row0 = (size_t)c * A.nf;
    int base = 0;
    for (int i0 = 0; i0 < A.nf; i0 += PNP_T) {
        const int i = i0 + tid;
        int p = -1;
        bool keep = false;
        if (i < A.nf) {
            p = A.pts[row0 + i];
            keep = p >= 0 && p < A.pcap;
            if (keep) {
                const unsigned f = A.flags[p];
                keep = (f & AFV_PTF_SET) && !(f & AFV_PTF_BAD);
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int rank = base + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < PNP_WAVES; ++w) {
            if (w < wave) rank += s_wave[w];
            total += s_wave[w];
        }
        if (keep) {
            const size_t o = row0 + rank;
            A.index[o] = i;
            A.p2d[2 * o] = A.x[i]; A.p2d[2 * o + 1] = A.y[i];
            A.p3dw[3 * o] = A.pos[0][p]; A.p3dw[3 * o + 1] = A.pos[1][p]; A.p3dw[3 * o + 2] = A.pos[2][p];
            A.max_err[o] = A.sigma2[i] * J.th2;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) {
        A.n[c] = base;
        const float prod = (float)base * J.epsilon;  // :134, the product in float, truncated
        int n_min = !(prod < 2147483648.0f) ? 2147483647 : (int)prod;
        n_min = max(n_min, J.min_inliers);
        A.min_inliers[c] = max(n_min, 4);
    }
    for (int k = base + tid; k < A.nf; k += PNP_T) {  // what the outputs read from N on
        const size_t o = row0 + k;
        A.index[o] = -1;
        A.p3dw[3 * o] = 0.0f; A.p3dw[3 * o + 1] = 0.0f; A.p3dw[3 * o + 2] = 0.0f;
        A.max_err[o] = 0.0f;
    }
}

// ---- EPnP ----
struct PnpLds {          // one wavefront's
    double M[12][12];    // M^T M, then what the Jacobi leaves of it
    double V[12][12];    // its eigenvectors by column
    double L[60];        // L_6x10
};
struct PnpSel {          // the selected correspondences: sel[0 .. n) index the candidate's compacted rows
    const float *p2d, *p3dw;
    const unsigned short *sel;
    int n;
    double fu, fv, uc, vc;
};

// E7: the halving tree over the 64 partial sums; every lane returns p[0]
__device__ __forceinline__ double p_tree(double p) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p = p + __shfl_down(p, s, 64);
    return __shfl(p, 0, 64);
}
template <int K>
__device__ __forceinline__ void p_tree(double (&acc)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = p_tree(acc[k]);
}

__device__ __forceinline__ void p_load(const PnpSel &S, int j, double (&pw)[3], double &u, double &v) {
    const int i = S.sel[j];
    pw[0] = (double)S.p3dw[3 * i]; pw[1] = (double)S.p3dw[3 * i + 1]; pw[2] = (double)S.p3dw[3 * i + 2];
    u = (double)S.p2d[2 * i]; v = (double)S.p2d[2 * i + 1];
}
__device__ __forceinline__ double p_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ double p_dist2(const double *a, const double *b) {
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}
__device__ __forceinline__ double p_pick(const double (&a)[4], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3])); }
__device__ __forceinline__ int p_pick_i(const int (&a)[4], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3])); }
__device__ __forceinline__ double p_pick3(const double (&a)[3], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : a[2]); }

// compute_barycentric_coordinates (:423-433) of one point
__device__ __forceinline__ void p_alphas(const double (&c0)[3], const double (&ci)[9], const double (&pw)[3], double (&a)[4]) {
    const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

__device__ __forceinline__ bool p_rotation(double app, double aqq, double apq, double &c, double &s, double &t) {
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
template <int P, int Q>
__device__ __forceinline__ bool p_rotate3(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q], app = a[P][P], aqq = a[Q][Q];
    double c, s, t;
    if (!p_rotation(app, aqq, apq, c, s, t)) return false;
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
// E2 / E5: the Jacobi on a symmetric 3 x 3; d = the diagonal, vk[k] = the eigenvector of rank k (descending, ties to the lowest index)
__device__ __forceinline__ void p_eig3(double (&a)[3][3], double (&d)[3], double (&vk)[3][3]) {
    double v[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < PNP_SWEEPS; ++sweep) {
        bool any = p_rotate3<0, 1>(a, v);
        any |= p_rotate3<0, 2>(a, v);
        any |= p_rotate3<1, 2>(a, v);
        if (!any) break;
    }
    const double dg[3] = {a[0][0], a[1][1], a[2][2]};
    int col[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) rank += (dg[j] > dg[i] || (dg[j] == dg[i] && j < i)) ? 1 : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (rank == k) col[k] = i;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = p_pick3(dg, col[k]);
#pragma unroll
        for (int r = 0; r < 3; ++r) vk[k][r] = p_pick3(v[r], col[k]);
    }
}

// qr_solve (:860-950) as written, on registers.  false: eta == 0 (E8; X reads 0)
template <int NC>
__device__ __forceinline__ bool p_qr_solve(double (&A)[6 * NC], double (&b)[6], double (&X)[NC]) {
    double A1[NC], A2[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) X[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        double eta = fabs(A[k * NC + k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double elt = fabs(A[i * NC + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0.0) return false;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
#pragma unroll
        for (int i = k; i < 6; ++i) {
            A[i * NC + k] = A[i * NC + k] * inv_eta;
            sum = sum + A[i * NC + k] * A[i * NC + k];
        }
        double sigma = sqrt(sum);
        if (A[k * NC + k] < 0.0) sigma = -sigma;
        A[k * NC + k] = A[k * NC + k] + sigma;
        A1[k] = sigma * A[k * NC + k];
        A2[k] = -eta * sigma;
#pragma unroll
        for (int j = k + 1; j < NC; ++j) {
            double s2 = 0.0;
#pragma unroll
            for (int i = k; i < 6; ++i) s2 = s2 + A[i * NC + k] * A[i * NC + j];
            const double tau = s2 / A1[k];
#pragma unroll
            for (int i = k; i < 6; ++i) A[i * NC + j] = A[i * NC + j] - tau * A[i * NC + k];
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        double tau = 0.0;
#pragma unroll
        for (int i = j; i < 6; ++i) tau = tau + A[i * NC + j] * b[i];
        tau = tau / A1[j];
#pragma unroll
        for (int i = j; i < 6; ++i) b[i] = b[i] - tau * A[i * NC + j];
    }
    X[NC - 1] = b[NC - 1] / A2[NC - 1];
#pragma unroll
    for (int i = NC - 2; i >= 0; --i) {
        double sum = 0.0;
#pragma unroll
        for (int j = i + 1; j < NC; ++j) sum = sum + A[i * NC + j] * X[j];
        X[i] = (b[i] - sum) / A2[i];
    }
    return true;
}

// find_betas_approx_2 / _3 (:714-722, :748-755): betas[0], betas[1] from b[0], b[1], b[2]
__device__ __forceinline__ void p_b01(double b0, double b1, double b2, double &o0, double &o1) {
    if (b0 < 0.0) {
        o0 = sqrt(-b0);
        o1 = (b2 < 0.0) ? sqrt(-b2) : 0.0;
    } else {
        o0 = sqrt(b0);
        o1 = (b2 > 0.0) ? sqrt(b2) : 0.0;
    }
    if (b1 < 0.0) o0 = -o0;
}

// compute_pose (:477-525) over the selected correspondences.  Every lane of the wavefront calls it with the same arguments and leaves with
// the same R (row-major) and t.  false: degenerate (E8)
__device__ __forceinline__ bool p_epnp(const PnpSel &S, PnpLds &W, int lane, double (&R)[9], double (&t)[3]) {
    const int n = S.n;
    const double fn = (double)n, fu = S.fu, fv = S.fv, uc = S.uc, vc = S.vc;
    bool bad = false;
    // choose_control_points (:375-409)
    double c0[3], cws[4][3];
    {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int j = lane; j < n; j += 64) {
            double pw[3], u, v;
            p_load(S, j, pw, u, v);
            acc[0] = acc[0] + pw[0]; acc[1] = acc[1] + pw[1]; acc[2] = acc[2] + pw[2];
        }
        p_tree(acc);
#pragma unroll
        for (int k = 0; k < 3; ++k) { c0[k] = acc[k] / fn; cws[0][k] = c0[k]; }
    }
    {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        for (int j = lane; j < n; j += 64) {
            double pw[3], u, v;
            p_load(S, j, pw, u, v);
            const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
            acc[0] = acc[0] + d0 * d0; acc[1] = acc[1] + d0 * d1; acc[2] = acc[2] + d0 * d2;
            acc[3] = acc[3] + d1 * d1; acc[4] = acc[4] + d1 * d2; acc[5] = acc[5] + d2 * d2;
        }
        p_tree(acc);
        double a[3][3] = {{acc[0], acc[1], acc[2]}, {acc[1], acc[3], acc[4]}, {acc[2], acc[4], acc[5]}};
        double dc[3], vk[3][3];
        p_eig3(a, dc, vk);
#pragma unroll
        for (int i = 1; i < 4; ++i) {
            const double k = sqrt(dc[i - 1] / fn);
#pragma unroll
            for (int j = 0; j < 3; ++j) cws[i][j] = c0[j] + k * vk[i - 1][j];
        }
    }
    // compute_barycentric_coordinates (:411-421), E3
    double ci[9];
    {
        double m[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 1; j < 4; ++j) m[3 * i + j - 1] = cws[j][i] - cws[0][i];
        const double k0 = m[4] * m[8] - m[5] * m[7], k1 = m[5] * m[6] - m[3] * m[8], k2 = m[3] * m[7] - m[4] * m[6];
        const double inv = 1.0 / (m[0] * k0 + m[1] * k1 + m[2] * k2);
        ci[0] = k0 * inv; ci[1] = (m[2] * m[7] - m[1] * m[8]) * inv; ci[2] = (m[1] * m[5] - m[2] * m[4]) * inv;
        ci[3] = k1 * inv; ci[4] = (m[0] * m[8] - m[2] * m[6]) * inv; ci[5] = (m[2] * m[3] - m[0] * m[5]) * inv;
        ci[6] = k2 * inv; ci[7] = (m[1] * m[6] - m[0] * m[7]) * inv; ci[8] = (m[0] * m[4] - m[1] * m[3]) * inv;
    }
    // M^T M (:482-492): one pass per pair (i, k) of alpha indices, seven sums each
    __syncthreads();
    for (int e = lane; e < 144; e += 64) {
        W.M[e / 12][e % 12] = 0.0;
        W.V[e / 12][e % 12] = (e / 12 == e % 12) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int i = 0; i < 4; ++i)
        for (int k = i; k < 4; ++k) {
            double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int j = lane; j < n; j += 64) {
                double pw[3], u, v, a[4];
                p_load(S, j, pw, u, v);
                p_alphas(c0, ci, pw, a);
                const double ai = p_pick(a, i), ak = p_pick(a, k), du = uc - u, dv = vc - v;
                const double Ai = ai * fu, Ak = ak * fu, Bi = ai * fv, Bk = ak * fv, Ci = ai * du, Ck = ak * du, Di = ai * dv, Dk = ak * dv;
                acc[0] = acc[0] + Ai * Ak;
                acc[1] = acc[1] + Ai * Ck;
                acc[2] = acc[2] + Bi * Bk;
                acc[3] = acc[3] + Bi * Dk;
                acc[4] = acc[4] + (Ci * Ck + Di * Dk);
                acc[5] = acc[5] + Ci * Ak;
                acc[6] = acc[6] + Di * Bk;
            }
            p_tree(acc);
            if (lane == 0) {
                const int r = 3 * i, c = 3 * k;
                W.M[r][c] = acc[0]; W.M[c][r] = acc[0];
                W.M[r][c + 2] = acc[1]; W.M[c + 2][r] = acc[1];
                W.M[r + 1][c + 1] = acc[2]; W.M[c + 1][r + 1] = acc[2];
                W.M[r + 1][c + 2] = acc[3]; W.M[c + 2][r + 1] = acc[3];
                W.M[r + 2][c + 2] = acc[4]; W.M[c + 2][r + 2] = acc[4];
                if (i < k) {
                    W.M[r + 2][c] = acc[5]; W.M[c][r + 2] = acc[5];
                    W.M[r + 2][c + 1] = acc[6]; W.M[c + 1][r + 2] = acc[6];
                }
            }
        }
    __syncthreads();
    // E1
    for (int sweep = 0; sweep < PNP_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 11; ++p)
            for (int q = p + 1; q < 12; ++q) {
                const double apq = W.M[p][q], app = W.M[p][p], aqq = W.M[q][q];
                double c, s, tt;
                const bool turn = p_rotation(app, aqq, apq, c, s, tt);  // wavefront-uniform
                __syncthreads();
                if (turn) {
                    rotated = true;
                    if (lane < 12) {  // row / column `lane` of the matrix
                        if (lane != p && lane != q) {
                            const double akp = W.M[lane][p], akq = W.M[lane][q];
                            const double np = c * akp - s * akq, nq = s * akp + c * akq;
                            W.M[lane][p] = np; W.M[p][lane] = np;
                            W.M[lane][q] = nq; W.M[q][lane] = nq;
                        }
                    } else if (lane < 24) {  // row lane - 12 of V
                        const int k = lane - 12;
                        const double vkp = W.V[k][p], vkq = W.V[k][q];
                        W.V[k][p] = c * vkp - s * vkq;
                        W.V[k][q] = s * vkp + c * vkq;
                    } else if (lane == 24) {
                        W.M[p][p] = app - tt * apq;
                        W.M[q][q] = aqq + tt * apq;
                        W.M[p][q] = 0.0; W.M[q][p] = 0.0;
                    }
                }
                __syncthreads();
            }
        if (!rotated) break;
    }
    int vc4[4] = {0, 0, 0, 0};  // the column of v[i] = ut row 11 - i
    for (int i = 0; i < 12; ++i) {
        const double di = W.M[i][i];
        int rank = 0;
        for (int j = 0; j < 12; ++j) {
            const double dj = W.M[j][j];
            rank += (dj > di || (dj == di && j < i)) ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (11 - rank == k) vc4[k] = i;
    }
    // compute_L_6x10 (:760-800): entry e = (pair row, column) on lane e
    if (lane < 60) {
        const int row = lane / 10, cc = lane - 10 * row;
        const int a = (int)((0x211000u >> (4 * row)) & 15u), b = (int)((0x332321u >> (4 * row)) & 15u);
        const int k1 = (int)((0x3210210100ull >> (4 * cc)) & 15ull), k2 = (int)((0x3333222110ull >> (4 * cc)) & 15ull);
        const int c1 = p_pick_i(vc4, k1), c2 = p_pick_i(vc4, k2);
        double d1[3], d2[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            d1[x] = W.V[3 * a + x][c1] - W.V[3 * b + x][c1];
            d2[x] = W.V[3 * a + x][c2] - W.V[3 * b + x][c2];
        }
        const double d = p_dot3(d1, d2);
        W.L[lane] = k1 == k2 ? d : 2.0 * d;
    }
    __syncthreads();
    double rho[6];
    rho[0] = p_dist2(cws[0], cws[1]); rho[1] = p_dist2(cws[0], cws[2]); rho[2] = p_dist2(cws[0], cws[3]);
    rho[3] = p_dist2(cws[1], cws[2]); rho[4] = p_dist2(cws[1], cws[3]); rho[5] = p_dist2(cws[2], cws[3]);

    double best_e = 0.0;
    // The two loops below stay rolled on purpose.  The kernels already fill the register file (256 VGPRs + about 240 AGPRs: the compiler
    // parks values in AGPRs, so "no scratch" is not "no pressure"); unrolling either loop would multiply the fully unrolled p_qr_solve
    // instances and may tip the allocation into scratch: read the compiler's resource report after any change here
#pragma unroll 1
    for (int ap = 0; ap < 3; ++ap) {
        double betas[4];
        {   // find_betas_approx_1 / _2 / _3 (:667-758), E4
            double b[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) b[i] = rho[i];
            if (ap == 0) {
                double A4[24], X[4];
#pragma unroll
                for (int i = 0; i < 6; ++i) { A4[4 * i] = W.L[10 * i]; A4[4 * i + 1] = W.L[10 * i + 1]; A4[4 * i + 2] = W.L[10 * i + 3]; A4[4 * i + 3] = W.L[10 * i + 6]; }
                if (!p_qr_solve<4>(A4, b, X)) bad = true;
                if (X[0] < 0.0) {
                    betas[0] = sqrt(-X[0]);
                    betas[1] = -X[1] / betas[0]; betas[2] = -X[2] / betas[0]; betas[3] = -X[3] / betas[0];
                } else {
                    betas[0] = sqrt(X[0]);
                    betas[1] = X[1] / betas[0]; betas[2] = X[2] / betas[0]; betas[3] = X[3] / betas[0];
                }
                if (betas[0] == 0.0) bad = true;
            } else if (ap == 1) {
                double A3[18], X[3];
#pragma unroll
                for (int i = 0; i < 6; ++i) { A3[3 * i] = W.L[10 * i]; A3[3 * i + 1] = W.L[10 * i + 1]; A3[3 * i + 2] = W.L[10 * i + 2]; }
                if (!p_qr_solve<3>(A3, b, X)) bad = true;
                p_b01(X[0], X[1], X[2], betas[0], betas[1]);
                betas[2] = 0.0; betas[3] = 0.0;
            } else {
                double A5[30], X[5];
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int k = 0; k < 5; ++k) A5[5 * i + k] = W.L[10 * i + k];
                if (!p_qr_solve<5>(A5, b, X)) bad = true;
                p_b01(X[0], X[1], X[2], betas[0], betas[1]);
                if (betas[0] == 0.0) bad = true;
                betas[2] = X[3] / betas[0];
                betas[3] = 0.0;
            }
        }
#pragma unroll 1
        for (int it = 0; it < 5; ++it) {  // gauss_newton (:812-858)
            double A4[24], b[6], X[4];
            const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double r[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) r[k] = W.L[10 * i + k];
                A4[4 * i] = 2.0 * r[0] * b0 + r[1] * b1 + r[3] * b2 + r[6] * b3;
                A4[4 * i + 1] = r[1] * b0 + 2.0 * r[2] * b1 + r[4] * b2 + r[7] * b3;
                A4[4 * i + 2] = r[3] * b0 + r[4] * b1 + 2.0 * r[5] * b2 + r[8] * b3;
                A4[4 * i + 3] = r[6] * b0 + r[7] * b1 + r[8] * b2 + 2.0 * r[9] * b3;
                b[i] = rho[i] - (r[0] * b0 * b0 + r[1] * b0 * b1 + r[2] * b1 * b1 + r[3] * b0 * b2 + r[4] * b1 * b2 + r[5] * b2 * b2 +
                                 r[6] * b0 * b3 + r[7] * b1 * b3 + r[8] * b2 * b3 + r[9] * b3 * b3);
            }
            if (!p_qr_solve<4>(A4, b, X)) bad = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) betas[k] = betas[k] + X[k];
        }
        // compute_R_and_t (:651-662)
        double ccs[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) ccs[j][k] = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) ccs[j][k] = ccs[j][k] + betas[i] * W.V[3 * j + k][vc4[i]];
        {   // solve_for_sign (:636-649), Q6
            double pw[3], u, v, a[4];
            p_load(S, 0, pw, u, v);
            p_alphas(c0, ci, pw, a);
            const double z = a[0] * ccs[0][2] + a[1] * ccs[1][2] + a[2] * ccs[2][2] + a[3] * ccs[3][2];
            if (z < 0.0) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int k = 0; k < 3; ++k) ccs[j][k] = -ccs[j][k];
            }
        }
        // estimate_R_and_t (:569-627); pw0 is cws[0]: the same sum of the same shape
        double pc0[3];
        {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int j = lane; j < n; j += 64) {
                double pw[3], u, v, a[4];
                p_load(S, j, pw, u, v);
                p_alphas(c0, ci, pw, a);
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[k] = acc[k] + (a[0] * ccs[0][k] + a[1] * ccs[1][k] + a[2] * ccs[2][k] + a[3] * ccs[3][k]);
            }
            p_tree(acc);
#pragma unroll
            for (int k = 0; k < 3; ++k) pc0[k] = acc[k] / fn;
        }
        double Ra[9], ta[3];
        {
            double A[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int j = lane; j < n; j += 64) {
                double pw[3], u, v, a[4];
                p_load(S, j, pw, u, v);
                p_alphas(c0, ci, pw, a);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double pc = a[0] * ccs[0][r] + a[1] * ccs[1][r] + a[2] * ccs[2][r] + a[3] * ccs[3][r];
                    const double dp = pc - pc0[r];
                    A[3 * r] = A[3 * r] + dp * (pw[0] - c0[0]);
                    A[3 * r + 1] = A[3 * r + 1] + dp * (pw[1] - c0[1]);
                    A[3 * r + 2] = A[3 * r + 2] + dp * (pw[2] - c0[2]);
                }
            }
            p_tree(A);
            double ata[3][3], dd[3], vk[3][3];  // E5
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = i; j < 3; ++j) {
                    ata[i][j] = A[i] * A[j] + A[3 + i] * A[3 + j] + A[6 + i] * A[6 + j];
                    ata[j][i] = ata[i][j];
                }
            p_eig3(ata, dd, vk);
            double Av[3][3], uk[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int i = 0; i < 3; ++i) Av[k][i] = A[3 * i] * vk[k][0] + A[3 * i + 1] * vk[k][1] + A[3 * i + 2] * vk[k][2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double nrm = sqrt(Av[k][0] * Av[k][0] + Av[k][1] * Av[k][1] + Av[k][2] * Av[k][2]);
#pragma unroll
                for (int i = 0; i < 3; ++i) uk[k][i] = Av[k][i] / nrm;
            }
            uk[2][0] = uk[0][1] * uk[1][2] - uk[0][2] * uk[1][1];
            uk[2][1] = uk[0][2] * uk[1][0] - uk[0][0] * uk[1][2];
            uk[2][2] = uk[0][0] * uk[1][1] - uk[0][1] * uk[1][0];
            if (p_dot3(Av[2], uk[2]) < 0.0) { vk[2][0] = -vk[2][0]; vk[2][1] = -vk[2][1]; vk[2][2] = -vk[2][2]; }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Ra[3 * i + j] = uk[0][i] * vk[0][j] + uk[1][i] * vk[1][j] + uk[2][i] * vk[2][j];
            const double det = Ra[0] * Ra[4] * Ra[8] + Ra[1] * Ra[5] * Ra[6] + Ra[2] * Ra[3] * Ra[7] - Ra[2] * Ra[4] * Ra[6] - Ra[1] * Ra[3] * Ra[8] -
                               Ra[0] * Ra[5] * Ra[7];
            if (det < 0.0) { Ra[6] = -Ra[6]; Ra[7] = -Ra[7]; Ra[8] = -Ra[8]; }
#pragma unroll
            for (int i = 0; i < 3; ++i) ta[i] = pc0[i] - p_dot3(Ra + 3 * i, c0);
        }
        double err;
        {   // reprojection_error (:550-567)
            double acc = 0.0;
            for (int j = lane; j < n; j += 64) {
                double pw[3], u, v;
                p_load(S, j, pw, u, v);
                const double Xc = p_dot3(Ra, pw) + ta[0], Yc = p_dot3(Ra + 3, pw) + ta[1], inv_Zc = 1.0 / (p_dot3(Ra + 6, pw) + ta[2]);
                const double ue = uc + fu * Xc * inv_Zc, ve = vc + fv * Yc * inv_Zc;
                acc = acc + sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
            }
            err = p_tree(acc) / fn;
        }
        if (ap == 0 || (p_finite(err) && (!p_finite(best_e) || err < best_e))) {  // :518-522; E8: an error that is not finite loses
            best_e = err;
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = Ra[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = ta[k];
        }
    }
    bool ok = !bad;
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && p_finite(R[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && p_finite(t[k]);
    return ok;
}

// CheckInliers (:308-339, Q5) over the candidate's N correspondences + the outputs of one hypothesis; ok false: everything reads 0
__device__ __forceinline__ int p_check(const DevPnpArgs &A, size_t row0, int N, bool ok, const double (&R)[9], const double (&t)[3], int lane,
                                       float *pose, uint32_t *words) {
    const double fu = (double)A.fx, fv = (double)A.fy, uc = (double)A.cx, vc = (double)A.cy;
    const int pairs = (A.mask_words + 1) >> 1;
    if (lane < 12) {
        double val = 0.0;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (lane == k) val = R[k];
            if (lane == 9) val = t[0];
            if (lane == 10) val = t[1];
            if (lane == 11) val = t[2];
        }
        pose[lane] = (float)val;
    }
    int count = 0;
    for (int j = 0; j < pairs; ++j) {
        const int k = j * 64 + lane;
        bool in = false;
        if (ok && k < N) {
            const size_t o = row0 + k;
            const double X = (double)A.p3dw[3 * o], Y = (double)A.p3dw[3 * o + 1], Z = (double)A.p3dw[3 * o + 2];
            const float Xc = (float)(R[0] * X + R[1] * Y + R[2] * Z + t[0]);
            const float Yc = (float)(R[3] * X + R[4] * Y + R[5] * Z + t[1]);
            const float invZc = (float)(1.0 / (R[6] * X + R[7] * Y + R[8] * Z + t[2]));
            const double ue = uc + fu * (double)Xc * (double)invZc;
            const double ve = vc + fv * (double)Yc * (double)invZc;
            const float distX = (float)((double)A.p2d[2 * o] - ue);
            const float distY = (float)((double)A.p2d[2 * o + 1] - ve);
            const float error2 = distX * distX + distY * distY;
            in = error2 < A.max_err[o];
        }
        const unsigned long long m = __ballot(in);
        count += __popcll(m);
        if (lane == 0) words[2 * j] = (uint32_t)m;
        if (lane == 1 && 2 * j + 1 < A.mask_words) words[2 * j + 1] = (uint32_t)(m >> 32);
    }
    return count;
}

__global__ __launch_bounds__(64) void k_pnp_hypotheses(const DevPnpArgs A) {
    __shared__ PnpLds W;
    __shared__ unsigned short s_sel[4];
    const int lane = threadIdx.x, h = blockIdx.x, c = blockIdx.y;
    const DevPnpCand &J = A.cands[c];
    const size_t row0 = (size_t)c * A.nf, ho = (size_t)c * A.nhyp + h;
    const int N = min(A.n[c], min(A.nf, PNP_MAX_SEL));
    bool ok = N >= 4;  // E9
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0.0;
    t[0] = 0.0; t[1] = 0.0; t[2] = 0.0;
    if (ok) {  // block-uniform
        // E6: the four draws on vAvailableIndices with swap-with-back, without the list: the entries a removal overwrote are remembered
        const unsigned long long key = p_sm(p_sm(J.seed) ^ (unsigned long long)(h + 1));
        const unsigned long long step = 0xD1342543DE82EF95ull;
        int wpos[4] = {-1, -1, -1, -1}, wval[4] = {0, 0, 0, 0}, pick[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int size = N - d;
            const int r = (int)(p_sm(key + (unsigned long long)(d + 1) * step) % (unsigned long long)size);
            int at_r = r, at_back = size - 1;
#pragma unroll
            for (int w = 0; w < 4; ++w) {  // later writes win
                if (w < d && wpos[w] == r) at_r = wval[w];
                if (w < d && wpos[w] == size - 1) at_back = wval[w];
            }
            pick[d] = at_r;
            wpos[d] = r; wval[d] = at_back;
        }
        if (lane < 4) s_sel[lane] = (unsigned short)(lane == 0 ? pick[0] : (lane == 1 ? pick[1] : (lane == 2 ? pick[2] : pick[3])));
        __syncthreads();
        PnpSel S{A.p2d + 2 * row0, A.p3dw + 3 * row0, s_sel, 4, (double)A.fx, (double)A.fy, (double)A.cx, (double)A.cy};
        ok = p_epnp(S, W, lane, R, t);
    }
    if (lane == 0) A.degenerate[ho] = (N >= 4 && !ok) ? 1 : 0;
    const int count = p_check(A, row0, N, ok, R, t, lane, A.pose + ho * 12, A.inliers + ho * A.mask_words);
    if (lane == 0) A.count[ho] = count;
}

__global__ __launch_bounds__(64) void k_pnp_refine(const DevPnpArgs A) {
    __shared__ PnpLds W;
    __shared__ unsigned short s_sel[PNP_MAX_SEL];
    const int lane = threadIdx.x, h = blockIdx.x, c = blockIdx.y;
    const size_t row0 = (size_t)c * A.nf, ho = (size_t)c * A.nhyp + h;
    const int N = min(A.n[c], min(A.nf, PNP_MAX_SEL));
    const int pairs = (A.mask_words + 1) >> 1;
    const int *counts = A.count + (size_t)c * A.nhyp;
    const int mine = counts[h];
    int before = 0;
    for (int g = lane; g < h; g += 64) before = max(before, counts[g]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) before = max(before, __shfl_xor(before, s, 64));
    const bool record = N >= 4 && mine >= A.min_inliers[c] && mine > before;  // block-uniform
    bool ok = false;
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0.0;
    t[0] = 0.0; t[1] = 0.0; t[2] = 0.0;
    if (record) {
        const uint32_t *words = A.inliers + ho * A.mask_words;
        int base = 0;
        for (int j = 0; j < pairs; ++j) {  // Refine's vIndices (:265-271): the inliers in correspondence order
            const int k = j * 64 + lane, w = k >> 5;
            const bool in = k < N && w < A.mask_words && ((words[w] >> (k & 31)) & 1u);
            const unsigned long long m = __ballot(in);
            if (in) s_sel[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)k;
            base += __popcll(m);
        }
        __syncthreads();
        PnpSel S{A.p2d + 2 * row0, A.p3dw + 3 * row0, s_sel, base, (double)A.fx, (double)A.fy, (double)A.cx, (double)A.cy};
        ok = p_epnp(S, W, lane, R, t);
    }
    if (lane == 0) A.refined[ho] = record ? (ok ? 1 : 2) : 0;
    const int count = p_check(A, row0, N, ok, R, t, lane, A.refined_pose + ho * 12, A.refined_inliers + ho * A.mask_words);
    if (lane == 0) A.refined_count[ho] = count;
}

extern "C" void afv_launch_pnp(const DevPnpArgs *args, hipStream_t stream) {
    hipLaunchKernelGGL(k_pnp_gather, dim3(args->nc), dim3(PNP_T), 0, stream, *args);
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(args->nhyp, args->nc), dim3(64), 0, stream, *args);
    hipLaunchKernelGGL(k_pnp_refine, dim3(args->nhyp, args->nc), dim3(64), 0, stream, *args);
}
