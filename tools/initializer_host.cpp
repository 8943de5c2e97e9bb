// initializer_host — Initializer::Initialize as tests/_init_ref.py restates it (the semantics of afv_frame_initializer, include/afv_hip.h,
// "Initializer": quirks, deviations I1-I11), as a scalar host program: what the device's answers are compared with, bit for bit, and timed
// against by tools/time_initializer.py.  Build: g++ -O3 -ffp-contract=off -std=c++17 -I include.  One thread; the reference spends two on
// the RANSAC half (FindHomography / FindFundamental), which the timing tool's report says.
//
// Input (binary, argv[1]): int32 n1, n2, iterations, calls; uint64 seed; float fx, fy, cx, cy, sigma; float x1[n1], y1[n1], x2[n2], y2[n2];
// int32 matches12[n1].
// Output (binary, argv[2]): int32 ok, route; float R21[9], t21[3], p3d[n1][3]; uint8 triangulated[n1]; afv_init_trace; float
// score[2][iterations], model[2][iterations][9]; uint8 degenerate[2][iterations]; uint32 inliers[2][iterations][(n1 + 31) / 32].
// stdout: one line "median_ms min_ms max_ms" over the calls.
// Triangulate's 4 x 4 null vector is tri_null_vector of csrc/k_tri_match.h (tests/_tri_ref.py jacobi_null_vector) written for the host.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "afv_hip.h"

static inline float sum3(float a0, float a1, float a2) { return a0 + (a1 + a2); }
static inline bool finite_f(float v) { return std::fabs(v) <= 3.402823466e38f; }
static inline uint64_t sm(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void mm(const float *A, const float *B, float *C) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = sum3(A[3 * r] * B[c], A[3 * r + 1] * B[3 + c], A[3 * r + 2] * B[6 + c]);
}
static void transpose(const float *A, float *T) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T[3 * r + c] = A[3 * c + r];
}
static float det3(const float *m) {
    const float c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    return sum3(m[0] * c0, m[1] * c1, m[2] * c2);
}
static void inv3(const float *m, float *o) {
    const float c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const float i = 1.0f / sum3(m[0] * c0, m[1] * c1, m[2] * c2);
    o[0] = c0 * i; o[1] = (m[2] * m[7] - m[1] * m[8]) * i; o[2] = (m[1] * m[5] - m[2] * m[4]) * i;
    o[3] = c1 * i; o[4] = (m[0] * m[8] - m[2] * m[6]) * i; o[5] = (m[2] * m[3] - m[0] * m[5]) * i;
    o[6] = c2 * i; o[7] = (m[1] * m[6] - m[0] * m[7]) * i; o[8] = (m[0] * m[4] - m[1] * m[3]) * i;
}
static bool finite9(const float *m) {
    for (int k = 0; k < 9; ++k)
        if (!finite_f(m[k])) return false;
    return true;
}
static void tmatrix(const float *nrm, float *T) {
    T[0] = nrm[2]; T[1] = 0.0f; T[2] = -nrm[0] * nrm[2];
    T[3] = 0.0f; T[4] = nrm[3]; T[5] = -nrm[1] * nrm[3];
    T[6] = 0.0f; T[7] = 0.0f; T[8] = 1.0f;
}

// I1 / I2: the cyclic Jacobi on a symmetric n x n in double (a, v: n x n row-major)
static void jacobi(double *a, double *v, int n) {
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) v[n * r + c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[n * p + q], app = a[n * p + p], aqq = a[n * q + q];
                if (apq == 0.0) continue;
                const double g = std::fabs(apq);
                if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) continue;
                const double theta = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = a[n * k + p], akq = a[n * k + q];
                    const double np = c * akp - s * akq, nq = s * akp + c * akq;
                    a[n * k + p] = np; a[n * p + k] = np;
                    a[n * k + q] = nq; a[n * q + k] = nq;
                }
                a[n * p + p] = app - t * apq;
                a[n * q + q] = aqq + t * apq;
                a[n * p + q] = 0.0; a[n * q + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[n * k + p], vkq = v[n * k + q];
                    v[n * k + p] = c * vkp - s * vkq;
                    v[n * k + q] = s * vkp + c * vkq;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
}

static void svd3(const float *A, float *U, float *w, float *V) {  // I2
    double a[9], m[9], v[9];
    for (int k = 0; k < 9; ++k) a[k] = (double)A[k];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int r = 0; r < 3; ++r) s = s + a[3 * r + i] * a[3 * r + j];
            m[3 * i + j] = s;
        }
    jacobi(m, v, 3);
    double d[3] = {m[0], m[4], m[8]};
    for (int i = 0; i < 2; ++i)
        for (int k = i + 1; k < 3; ++k)
            if (d[i] < d[k]) {
                std::swap(d[i], d[k]);
                for (int r = 0; r < 3; ++r) std::swap(v[3 * r + i], v[3 * r + k]);
            }
    double b[3][3], wd[3], u[3][3];
    for (int k = 0; k < 3; ++k) {
        for (int r = 0; r < 3; ++r) b[k][r] = (a[3 * r] * v[k] + a[3 * r + 1] * v[3 + k]) + a[3 * r + 2] * v[6 + k];
        wd[k] = std::sqrt((b[k][0] * b[k][0] + b[k][1] * b[k][1]) + b[k][2] * b[k][2]);
    }
    for (int r = 0; r < 3; ++r) { u[0][r] = b[0][r] / wd[0]; u[1][r] = b[1][r] / wd[1]; }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    const bool flip = (b[2][0] * u[2][0] + b[2][1] * u[2][1]) + b[2][2] * u[2][2] < 0.0;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) {
            U[3 * r + c] = (float)u[c][r];
            V[3 * r + c] = (float)((c == 2 && flip) ? -v[3 * r + c] : v[3 * r + c]);
        }
        w[r] = (float)wd[r];
    }
}

// vt.row(3) of cv::SVD::compute(A) as csrc/k_tri_match.h tri_null_vector computes it: At holds A transposed on entry
static void tri_null_vector(float At[4][4], float v[4]) {
    float Vt[4][4];
    double W[4];
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double t = (double)At[i][k];
            sd = sd + t * t;
            Vt[i][k] = i == k ? 1.0f : 0.0f;
        }
        W[i] = sd;
    }
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = false;
        for (int i = 0; i < 3; ++i)
            for (int j = i + 1; j < 4; ++j) {
                double a = W[i], b = W[j], p = 0.0;
                for (int k = 0; k < 4; ++k) p = p + (double)At[i][k] * (double)At[j][k];
                if (std::fabs(p) <= (double)(__FLT_EPSILON__ * 2.0f) * std::sqrt(a * b)) continue;
                p = p * 2.0;
                const double beta = a - b, gamma = std::sqrt(p * p + beta * beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)std::sqrt(delta / gamma);
                    c = (float)(p / (gamma * (double)s * 2.0));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2.0));
                    s = (float)(p / (gamma * (double)c * 2.0));
                }
                a = b = 0.0;
                const float ms = -s;
                for (int k = 0; k < 4; ++k) {
                    const float t0 = c * At[i][k] + s * At[j][k];
                    const float t1 = ms * At[i][k] + c * At[j][k];
                    At[i][k] = t0; At[j][k] = t1;
                    a = a + (double)t0 * (double)t0;
                    b = b + (double)t1 * (double)t1;
                }
                W[i] = a; W[j] = b;
                for (int k = 0; k < 4; ++k) {
                    const float t0 = c * Vt[i][k] + s * Vt[j][k];
                    const float t1 = ms * Vt[i][k] + c * Vt[j][k];
                    Vt[i][k] = t0; Vt[j][k] = t1;
                }
                changed = true;
            }
        if (!changed) break;
    }
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double t = (double)At[i][k];
            sd = sd + t * t;
        }
        W[i] = std::sqrt(sd);
    }
    int at[4] = {0, 1, 2, 3};
    for (int i = 0; i < 3; ++i) {
        int j = i;
        for (int k = i + 1; k < 4; ++k)
            if (W[j] < W[k]) j = k;
        if (i != j) { std::swap(W[i], W[j]); std::swap(at[i], at[j]); }
    }
    for (int k = 0; k < 4; ++k) v[k] = Vt[at[3]][k];
}

static float tree_sum(const float *e, int n, int width) {  // I5
    std::vector<float> p((size_t)width, 0.0f);
    const int rows = (n + width - 1) / width;
    for (int r = 0; r < rows; ++r)
        for (int t = 0; t < width; ++t) {
            const int i = r * width + t;
            p[(size_t)t] = p[(size_t)t] + (i < n ? e[i] : 0.0f);
        }
    for (int s = width / 2; s >= 1; s >>= 1)
        for (int t = 0; t < s; ++t) p[(size_t)t] = p[(size_t)t] + p[(size_t)(t + s)];
    return p[0];
}

struct Scene {
    int n1, n2, iterations;
    uint64_t seed;
    float fx, fy, cx, cy, sigma;
    std::vector<float> x1, y1, x2, y2;
    std::vector<int32_t> matches;
};
struct Answer {
    int32_t ok = 0, route = AFV_INIT_ROUTE_F;
    float R21[9] = {}, t21[3] = {};
    std::vector<float> p3d, score, model;
    std::vector<uint8_t> tri, degenerate;
    std::vector<uint32_t> inliers;
    afv_init_trace trace;
};
struct Check {
    int n_good = 0;
    float cos = 1.0f;
    std::vector<float> p3d;
    std::vector<uint8_t> status;
};

static void normalize(const std::vector<float> &x, const std::vector<float> &y, float *nrm, std::vector<float> &tmp) {
    const int n = (int)x.size();
    const float nf = (float)n;
    const float mx = tree_sum(x.data(), n, 256) / nf, my = tree_sum(y.data(), n, 256) / nf;
    tmp.resize((size_t)n);
    for (int i = 0; i < n; ++i) tmp[(size_t)i] = std::fabs(x[(size_t)i] - mx);
    const float dx = tree_sum(tmp.data(), n, 256) / nf;
    for (int i = 0; i < n; ++i) tmp[(size_t)i] = std::fabs(y[(size_t)i] - my);
    const float dy = tree_sum(tmp.data(), n, 256) / nf;
    nrm[0] = mx; nrm[1] = my; nrm[2] = 1.0f / dx; nrm[3] = 1.0f / dy;
}

static void check_rt(const Scene &S, const std::vector<int> &pairs, const uint32_t *words, int N, const float *R, const float *t, Check &C) {
    const float th2 = 4.0f * (S.sigma * S.sigma);
    const float K[9] = {S.fx, 0.0f, S.cx, 0.0f, S.fy, S.cy, 0.0f, 0.0f, 1.0f};
    const float P1[3][4] = {{S.fx, 0.0f, S.cx, 0.0f}, {0.0f, S.fy, S.cy, 0.0f}, {0.0f, 0.0f, 1.0f, 0.0f}};
    float P2[3][4], O2[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const float r0 = c < 3 ? R[c] : t[0], r1 = c < 3 ? R[3 + c] : t[1], r2 = c < 3 ? R[6 + c] : t[2];
            P2[r][c] = sum3(K[3 * r] * r0, K[3 * r + 1] * r1, K[3 * r + 2] * r2);
        }
    for (int r = 0; r < 3; ++r) O2[r] = sum3(-R[r] * t[0], -R[3 + r] * t[1], -R[6 + r] * t[2]);
    C.n_good = 0;
    C.p3d.assign((size_t)N * 3, 0.0f);
    C.status.assign((size_t)N, 0);
    std::vector<float> cosv;
    for (int k = 0; k < N; ++k) {
        if (!words || !((words[k >> 5] >> (k & 31)) & 1u)) continue;
        const int i1 = pairs[(size_t)2 * k], i2 = pairs[(size_t)2 * k + 1];
        const float kx1 = S.x1[(size_t)i1], ky1 = S.y1[(size_t)i1], kx2 = S.x2[(size_t)i2], ky2 = S.y2[(size_t)i2];
        float At[4][4], v[4];
        for (int c = 0; c < 4; ++c) {
            At[c][0] = kx1 * P1[2][c] - P1[0][c];
            At[c][1] = ky1 * P1[2][c] - P1[1][c];
            At[c][2] = kx2 * P2[2][c] - P2[0][c];
            At[c][3] = ky2 * P2[2][c] - P2[1][c];
        }
        tri_null_vector(At, v);
        if (v[3] == 0) continue;  // I10
        const float p0 = v[0] / v[3], p1 = v[1] / v[3], p2 = v[2] / v[3];
        if (!finite_f(p0) || !finite_f(p1) || !finite_f(p2)) continue;
        const float dist1 = std::sqrt(sum3(p0 * p0, p1 * p1, p2 * p2));
        const float n0 = p0 - O2[0], n1 = p1 - O2[1], n2 = p2 - O2[2];
        const float dist2 = std::sqrt(sum3(n0 * n0, n1 * n1, n2 * n2));
        const float cosp = sum3(p0 * n0, p1 * n1, p2 * n2) / (dist1 * dist2);
        if (!finite_f(cosp)) continue;  // I10
        if (p2 <= 0 && cosp < 0.99998f) continue;
        const float q0 = sum3(R[0] * p0, R[1] * p1, R[2] * p2) + t[0], q1 = sum3(R[3] * p0, R[4] * p1, R[5] * p2) + t[1];
        const float q2 = sum3(R[6] * p0, R[7] * p1, R[8] * p2) + t[2];
        if (q2 <= 0 && cosp < 0.99998f) continue;
        float iz = 1.0f / p2;
        float ex = (S.fx * p0 * iz + S.cx) - kx1, ey = (S.fy * p1 * iz + S.cy) - ky1;
        if (ex * ex + ey * ey > th2) continue;
        iz = 1.0f / q2;
        ex = (S.fx * q0 * iz + S.cx) - kx2; ey = (S.fy * q1 * iz + S.cy) - ky2;
        if (ex * ex + ey * ey > th2) continue;
        cosv.push_back(cosp);
        C.p3d[(size_t)3 * k] = p0; C.p3d[(size_t)3 * k + 1] = p1; C.p3d[(size_t)3 * k + 2] = p2;
        C.status[(size_t)k] = cosp < 0.99998f ? 3 : 1;
        C.n_good++;
    }
    if (C.n_good > 0) {
        std::sort(cosv.begin(), cosv.end());
        C.cos = cosv[(size_t)std::min(50, (int)cosv.size() - 1)];
    } else {
        C.cos = 1.0f;
    }
}

static void initialize(const Scene &S, Answer &A) {
    const int n1 = S.n1, it = S.iterations, mw = (n1 + 31) / 32;
    A.ok = 0; A.route = AFV_INIT_ROUTE_F;
    std::fill(A.R21, A.R21 + 9, 0.0f);
    std::fill(A.t21, A.t21 + 3, 0.0f);
    A.p3d.assign((size_t)n1 * 3, 0.0f);
    A.tri.assign((size_t)n1, 0);
    A.score.assign((size_t)2 * it, 0.0f);
    A.model.assign((size_t)2 * it * 9, 0.0f);
    A.degenerate.assign((size_t)2 * it, 0);
    A.inliers.assign((size_t)2 * it * mw, 0u);
    afv_init_trace &T = A.trace;
    std::memset(&T, 0, sizeof(T));
    T.struct_size = (uint32_t)sizeof(T);
    T.best_h = T.best_f = T.best_motion = -1;
    T.route = AFV_INIT_ROUTE_F;
    T.reason = AFV_INIT_TOO_FEW_MATCHES;
    std::vector<int> pairs;
    for (int i = 0; i < n1; ++i)
        if (S.matches[(size_t)i] >= 0) { pairs.push_back(i); pairs.push_back(S.matches[(size_t)i]); }
    const int N = (int)pairs.size() / 2;
    T.n = N;
    if (N < 8) return;  // I7
    float nrm[8], T1[9], T2[9];
    std::vector<float> tmp;
    normalize(S.x1, S.y1, nrm, tmp);
    normalize(S.x2, S.y2, nrm + 4, tmp);
    tmatrix(nrm, T1);
    tmatrix(nrm + 4, T2);
    std::vector<float> e((size_t)N);
    std::vector<int> avail((size_t)N);
    const float inv_s2 = 1.0f / (S.sigma * S.sigma);
    for (int h = 0; h < it; ++h) {
        int set8[8];
        for (int k = 0; k < N; ++k) avail[(size_t)k] = k;  // :78-90, literally
        const uint64_t key = sm(sm(S.seed) ^ (uint64_t)(h + 1));
        for (int d = 0; d < 8; ++d) {
            const int r = (int)(sm(key + (uint64_t)(d + 1) * 0xD1342543DE82EF95ull) % (uint64_t)(N - d));
            set8[d] = avail[(size_t)r];
            avail[(size_t)r] = avail[(size_t)(N - 1 - d)];
        }
        float u1[8], v1[8], u2[8], v2[8];
        for (int j = 0; j < 8; ++j) {
            const int i1 = pairs[(size_t)2 * set8[j]], i2 = pairs[(size_t)2 * set8[j] + 1];
            u1[j] = (S.x1[(size_t)i1] - nrm[0]) * nrm[2]; v1[j] = (S.y1[(size_t)i1] - nrm[1]) * nrm[3];
            u2[j] = (S.x2[(size_t)i2] - nrm[4]) * nrm[6]; v2[j] = (S.y2[(size_t)i2] - nrm[5]) * nrm[7];
        }
        for (int model = 0; model < 2; ++model) {
            const size_t ho = (size_t)model * it + h;
            float Am[16][9];
            const int nrows = model == AFV_INIT_ROUTE_H ? 16 : 8;
            for (int j = 0; j < 8; ++j) {
                if (model == AFV_INIT_ROUTE_H) {
                    const float r0[9] = {0.0f, 0.0f, 0.0f, -u1[j], -v1[j], -1.0f, v2[j] * u1[j], v2[j] * v1[j], v2[j]};
                    const float r1[9] = {u1[j], v1[j], 1.0f, 0.0f, 0.0f, 0.0f, -u2[j] * u1[j], -u2[j] * v1[j], -u2[j]};
                    std::memcpy(Am[2 * j], r0, sizeof(r0));
                    std::memcpy(Am[2 * j + 1], r1, sizeof(r1));
                } else {
                    const float r0[9] = {u2[j] * u1[j], u2[j] * v1[j], u2[j], v2[j] * u1[j], v2[j] * v1[j], v2[j], u1[j], v1[j], 1.0f};
                    std::memcpy(Am[j], r0, sizeof(r0));
                }
            }
            double M[81], V[81];
            for (int i = 0; i < 9; ++i)
                for (int j = 0; j < 9; ++j) {
                    double s = 0.0;
                    for (int r = 0; r < nrows; ++r) s = s + (double)Am[r][i] * (double)Am[r][j];
                    M[9 * i + j] = s;
                }
            jacobi(M, V, 9);
            int lo = 0;
            double dlo = M[0], largest = M[0];
            for (int k = 1; k < 9; ++k) {
                const double d = M[10 * k];
                if (d < dlo) { dlo = d; lo = k; }
                if (d > largest) largest = d;
            }
            double second = 0.0;
            bool have = false;
            for (int k = 0; k < 9; ++k) {
                const double d = M[10 * k];
                if (k != lo && (!have || d < second)) { second = d; have = true; }
            }
            const bool deficient = !(second > 1e-12 * largest);  // I8
            float nv[9], X[9], Y[9], Mo[9], Mi[9];
            for (int k = 0; k < 9; ++k) nv[k] = (float)V[9 * k + lo];
            bool ok;
            if (model == AFV_INIT_ROUTE_H) {
                inv3(T2, X);
                mm(X, nv, Y);
                mm(Y, T1, Mo);
                inv3(Mo, Mi);
                ok = !deficient && finite9(Mo) && finite9(Mi);
            } else {
                float U[9], w[3], Vv[9], UD[9], Vt[9], Fn[9];
                svd3(nv, U, w, Vv);
                for (int r = 0; r < 3; ++r) { UD[3 * r] = U[3 * r] * w[0]; UD[3 * r + 1] = U[3 * r + 1] * w[1]; UD[3 * r + 2] = U[3 * r + 2] * 0.0f; }
                transpose(Vv, Vt);
                mm(UD, Vt, Fn);
                transpose(T2, X);
                mm(X, Fn, Y);
                mm(Y, T1, Mo);
                ok = !deficient && finite9(Mo);
            }
            A.degenerate[ho] = ok ? 0 : 1;
            if (!ok) continue;
            std::memcpy(&A.model[ho * 9], Mo, sizeof(Mo));
            uint32_t *words = &A.inliers[ho * (size_t)mw];
            for (int k = 0; k < N; ++k) {
                const int i1 = pairs[(size_t)2 * k], i2 = pairs[(size_t)2 * k + 1];
                const float a1x = S.x1[(size_t)i1], a1y = S.y1[(size_t)i1], a2x = S.x2[(size_t)i2], a2y = S.y2[(size_t)i2];
                float chi1, chi2, gate;
                const float th = 5.991f;
                if (model == AFV_INIT_ROUTE_H) {
                    float w = 1.0f / sum3(Mi[6] * a2x, Mi[7] * a2y, Mi[8]);
                    float a = sum3(Mi[0] * a2x, Mi[1] * a2y, Mi[2]) * w, b = sum3(Mi[3] * a2x, Mi[4] * a2y, Mi[5]) * w;
                    chi1 = ((a1x - a) * (a1x - a) + (a1y - b) * (a1y - b)) * inv_s2;
                    w = 1.0f / sum3(Mo[6] * a1x, Mo[7] * a1y, Mo[8]);
                    a = sum3(Mo[0] * a1x, Mo[1] * a1y, Mo[2]) * w; b = sum3(Mo[3] * a1x, Mo[4] * a1y, Mo[5]) * w;
                    chi2 = ((a2x - a) * (a2x - a) + (a2y - b) * (a2y - b)) * inv_s2;
                    gate = 5.991f;
                } else {
                    const float a2 = sum3(Mo[0] * a1x, Mo[1] * a1y, Mo[2]), b2 = sum3(Mo[3] * a1x, Mo[4] * a1y, Mo[5]), c2 = sum3(Mo[6] * a1x, Mo[7] * a1y, Mo[8]);
                    const float num2 = sum3(a2 * a2x, b2 * a2y, c2);
                    chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_s2;
                    const float a1 = sum3(Mo[0] * a2x, Mo[3] * a2y, Mo[6]), b1 = sum3(Mo[1] * a2x, Mo[4] * a2y, Mo[7]), c1 = sum3(Mo[2] * a2x, Mo[5] * a2y, Mo[8]);
                    const float num1 = sum3(a1 * a1x, b1 * a1y, c1);
                    chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_s2;
                    gate = 3.841f;
                }
                const bool in1 = finite_f(chi1) && !(chi1 > gate), in2 = finite_f(chi2) && !(chi2 > gate);
                e[(size_t)k] = (in1 ? th - chi1 : 0.0f) + (in2 ? th - chi2 : 0.0f);
                if (in1 && in2) words[k >> 5] |= 1u << (k & 31);
            }
            A.score[ho] = tree_sum(e.data(), N, 64);
        }
    }
    int best[2];
    float Sc[2];
    for (int m = 0; m < 2; ++m) {
        best[m] = -1; Sc[m] = 0.0f;
        for (int h = 0; h < it; ++h)
            if (A.score[(size_t)m * it + h] > Sc[m]) { Sc[m] = A.score[(size_t)m * it + h]; best[m] = h; }
    }
    const float RH = Sc[0] / (Sc[0] + Sc[1]);
    const int route = RH > 0.4f ? AFV_INIT_ROUTE_H : AFV_INIT_ROUTE_F;
    const uint32_t *words = best[route] >= 0 ? &A.inliers[((size_t)route * it + best[route]) * (size_t)mw] : nullptr;
    int ninl = 0;
    if (words)
        for (int k = 0; k < mw; ++k) ninl += __builtin_popcount(words[k]);
    T.sh = Sc[0]; T.sf = Sc[1]; T.rh = RH; T.best_h = best[0]; T.best_f = best[1];
    for (int k = 0; k < 9; ++k) {
        T.h21[k] = best[0] >= 0 ? A.model[((size_t)best[0]) * 9 + k] : 0.0f;
        T.f21[k] = best[1] >= 0 ? A.model[((size_t)it + best[1]) * 9 + k] : 0.0f;
        T.T1[k] = T1[k]; T.T2[k] = T2[k];
    }
    T.route = route; T.n_inliers = ninl;
    A.route = route;
    float Mm[9], Km[9] = {S.fx, 0.0f, S.cx, 0.0f, S.fy, S.cy, 0.0f, 0.0f, 1.0f}, X[9], Y[9], U[9], wv[3], V[9], Vt[9];
    for (int k = 0; k < 9; ++k) Mm[k] = route == AFV_INIT_ROUTE_H ? T.h21[k] : T.f21[k];
    float Rm[8][9], tm[8][3];
    int nm = 0, reason = AFV_INIT_OK, pick = -1;
    if (route == AFV_INIT_ROUTE_F) {
        float E[9], UW[9];
        transpose(Km, X);
        mm(X, Mm, Y);
        mm(Y, Km, E);
        svd3(E, U, wv, V);
        transpose(V, Vt);
        float t0 = U[2], t1 = U[5], t2 = U[8];
        const float nrm = std::sqrt(sum3(t0 * t0, t1 * t1, t2 * t2));
        t0 = t0 / nrm; t1 = t1 / nrm; t2 = t2 / nrm;
        for (int v = 0; v < 2; ++v) {
            for (int r = 0; r < 3; ++r) {
                UW[3 * r] = v ? -U[3 * r + 1] : U[3 * r + 1];
                UW[3 * r + 1] = v ? U[3 * r] : -U[3 * r];
                UW[3 * r + 2] = U[3 * r + 2];
            }
            float Rv[9];
            mm(UW, Vt, Rv);
            const bool flip = det3(Rv) < 0;
            for (int k = 0; k < 9; ++k) Rm[v][k] = Rm[v + 2][k] = flip ? -Rv[k] : Rv[k];
            tm[v][0] = t0; tm[v][1] = t1; tm[v][2] = t2;
            tm[v + 2][0] = -t0; tm[v + 2][1] = -t1; tm[v + 2][2] = -t2;
        }
        nm = 4;
    } else {
        float Am[9];
        inv3(Km, X);
        mm(X, Mm, Y);
        mm(Y, Km, Am);
        if (det3(Am) < 0)  // I3
            for (int k = 0; k < 9; ++k) Am[k] = -Am[k];
        svd3(Am, U, wv, V);
        transpose(V, Vt);
        const float s = det3(U) * det3(Vt);
        const float d1 = wv[0], d2 = wv[1], d3 = wv[2];
        if (d1 / d2 < 1.00001f || d2 / d3 < 1.00001f) {
            reason = AFV_INIT_D_RATIO;
        } else {
            const float aux1 = std::sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = std::sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
            const float aux_st = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
            const float ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
            const float aux_sp = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
            const float cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
            float sU[9];
            for (int k = 0; k < 9; ++k) sU[k] = s * U[k];
            for (int i = 0; i < 8; ++i) {
                const int e4 = i & 3;
                const float x1 = e4 < 2 ? aux1 : -aux1, x3 = (e4 & 1) ? -aux3 : aux3;
                const bool second = i >= 4;
                const float st = (e4 == 0 || e4 == 3) ? (second ? aux_sp : aux_st) : (second ? -aux_sp : -aux_st);
                float Rp[9] = {ct, 0.0f, -st, 0.0f, 1.0f, 0.0f, st, 0.0f, ct};
                if (second) { Rp[0] = cp; Rp[2] = st; Rp[4] = -1.0f; Rp[6] = st; Rp[8] = -cp; }
                mm(sU, Rp, X);
                mm(X, Vt, Rm[i]);
                const float m = second ? d1 + d3 : d1 - d3;
                const float tp0 = x1 * m, tp1 = 0.0f * m, tp2 = (second ? x3 : -x3) * m;
                float tv[3];
                for (int r = 0; r < 3; ++r) tv[r] = sum3(U[3 * r] * tp0, U[3 * r + 1] * tp1, U[3 * r + 2] * tp2);
                const float nrm = std::sqrt(sum3(tv[0] * tv[0], tv[1] * tv[1], tv[2] * tv[2]));
                for (int r = 0; r < 3; ++r) tm[i][r] = tv[r] / nrm;
            }
            nm = 8;
        }
    }
    std::vector<Check> checks((size_t)nm);
    for (int i = 0; i < nm; ++i) check_rt(S, pairs, words, N, Rm[i], tm[i], checks[(size_t)i]);
    if (reason == AFV_INIT_OK) {
        if (route == AFV_INIT_ROUTE_F) {
            float Nf = 0.0f;
            for (int k = 0; k < ninl; ++k) Nf = Nf + 1.0f;
            int g[4], max_good = 0, nsimilar = 0, first = 3;
            for (int k = 0; k < 4; ++k) { g[k] = checks[(size_t)k].n_good; max_good = std::max(max_good, g[k]); }
            const int n_min_good = std::max((int)(0.9f * Nf), 50);
            for (int k = 3; k >= 0; --k) {
                if ((float)g[k] > 0.7f * (float)max_good) nsimilar++;
                if (g[k] == max_good) first = k;
            }
            if (max_good < n_min_good) reason = max_good < 50 ? AFV_INIT_MIN_TRIANGULATED : AFV_INIT_MIN_GOOD;
            else if (nsimilar > 1) reason = AFV_INIT_AMBIGUOUS;
            else if (checks[(size_t)first].cos < 0.99984770f) pick = first;
            else reason = AFV_INIT_PARALLAX;
        } else {
            int best_good = 0, second = 0, bi = -1;
            float best_cos = 2.0f;
            for (int i = 0; i < 8; ++i) {
                const int g = checks[(size_t)i].n_good;
                if (g > best_good) { second = best_good; best_good = g; bi = i; best_cos = checks[(size_t)i].cos; }
                else if (g > second) second = g;
            }
            if (!((float)second < 0.75f * (float)best_good)) reason = AFV_INIT_AMBIGUOUS;
            else if (!(best_cos <= 0.99984770f)) reason = AFV_INIT_PARALLAX;
            else if (!((float)best_good > (float)50)) reason = AFV_INIT_MIN_TRIANGULATED;
            else if (!((float)best_good > 0.9f * (float)ninl)) reason = AFV_INIT_MIN_GOOD;
            else pick = bi;
        }
    }
    T.n_motion = nm; T.best_motion = pick; T.reason = reason;
    for (int i = 0; i < nm; ++i) {
        T.n_good[i] = checks[(size_t)i].n_good;
        T.cos_parallax[i] = checks[(size_t)i].cos;
        std::memcpy(T.R[i], Rm[i], 36);
        std::memcpy(T.t[i], tm[i], 12);
    }
    if (pick >= 0) {
        A.ok = 1;
        std::memcpy(A.R21, Rm[pick], 36);
        std::memcpy(A.t21, tm[pick], 12);
        const Check &C = checks[(size_t)pick];
        for (int k = 0; k < N; ++k) {
            const int i1 = pairs[(size_t)2 * k];
            if (C.status[(size_t)k] & 1) std::memcpy(&A.p3d[(size_t)3 * i1], &C.p3d[(size_t)3 * k], 12);
            A.tri[(size_t)i1] = (uint8_t)((C.status[(size_t)k] >> 1) & 1);
        }
    }
}

template <class Tv>
static bool rd(FILE *f, Tv *p, size_t n) { return n == 0 || std::fread(p, sizeof(Tv), n, f) == n; }
template <class Tv>
static void wr(FILE *f, const Tv *p, size_t n) { if (n) std::fwrite(p, sizeof(Tv), n, f); }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    Scene S;
    int32_t head[4];
    float k5[5];
    if (!rd(f, head, 4) || !rd(f, &S.seed, 1) || !rd(f, k5, 5)) return 2;
    S.n1 = head[0]; S.n2 = head[1]; S.iterations = head[2];
    const int calls = std::max(head[3], 1);
    S.fx = k5[0]; S.fy = k5[1]; S.cx = k5[2]; S.cy = k5[3]; S.sigma = k5[4];
    S.x1.resize((size_t)S.n1); S.y1.resize((size_t)S.n1); S.x2.resize((size_t)S.n2); S.y2.resize((size_t)S.n2); S.matches.resize((size_t)S.n1);
    if (!rd(f, S.x1.data(), S.x1.size()) || !rd(f, S.y1.data(), S.y1.size()) || !rd(f, S.x2.data(), S.x2.size()) ||
        !rd(f, S.y2.data(), S.y2.size()) || !rd(f, S.matches.data(), S.matches.size()))
        return 2;
    std::fclose(f);
    Answer A;
    std::vector<double> ms;
    for (int c = 0; c < calls; ++c) {
        const auto t0 = std::chrono::steady_clock::now();
        initialize(S, A);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("%.6f %.6f %.6f\n", ms[ms.size() / 2], ms.front(), ms.back());
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    wr(o, &A.ok, 1); wr(o, &A.route, 1); wr(o, A.R21, 9); wr(o, A.t21, 3);
    wr(o, A.p3d.data(), A.p3d.size()); wr(o, A.tri.data(), A.tri.size()); wr(o, &A.trace, 1);
    wr(o, A.score.data(), A.score.size()); wr(o, A.model.data(), A.model.size()); wr(o, A.degenerate.data(), A.degenerate.size());
    wr(o, A.inliers.data(), A.inliers.size());
    std::fclose(o);
    return 0;
}
