// pnp_host.cpp — the restatement of PnPsolver (tests/_pnp_ref.py: the constructor, every EPnP RANSAC hypothesis and the Refine of every
// record of every candidate, quirks Q5 / Q6, deviations E1-E10 of include/afv_hip.h) as a scalar host program: what
// afv_frame_pnp_hypotheses is timed against (tools/time_pnp.py compiles it with g++ -O3 -ffp-contract=off and checks its answers
// bit-equal to the device's in the same run; tests/test_pnp_host_cpu.py holds it to the restatement).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

const int SWEEPS = 30;

inline uint64_t sm(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Sum {  // E7: 64 partial sums, then the halving tree
    double p[64];
    int j = 0;
    Sum() { for (double &v : p) v = 0.0; }
    void add(double v) { p[j & 63] = p[j & 63] + v; ++j; }
    double done() {
        for (int s = 32; s >= 1; s >>= 1)
            for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
        return p[0];
    }
};

bool rotation(double app, double aqq, double apq, double &c, double &s, double &t) {
    if (apq == 0.0) return false;
    const double g = std::fabs(apq);
    if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    c = 1.0 / std::sqrt(t * t + 1.0);
    s = t * c;
    return true;
}

// E1 / E2: a, v are n x n row-major
void jacobi(double *a, double *v, int n) {
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) v[r * n + c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[p * n + q], app = a[p * n + p], aqq = a[q * n + q];
                double c, s, t;
                if (!rotation(app, aqq, apq, c, s, t)) continue;
                for (int k = 0; k < n; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = a[k * n + p], akq = a[k * n + q];
                    const double np = c * akp - s * akq, nq = s * akp + c * akq;
                    a[k * n + p] = np; a[p * n + k] = np;
                    a[k * n + q] = nq; a[q * n + k] = nq;
                }
                a[p * n + p] = app - t * apq;
                a[q * n + q] = aqq + t * apq;
                a[p * n + q] = 0.0; a[q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[k * n + p], vkq = v[k * n + q];
                    v[k * n + p] = c * vkp - s * vkq;
                    v[k * n + q] = s * vkp + c * vkq;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
}

void order_desc(const double *a, int n, int *col) {
    for (int k = 0; k < n; ++k) col[k] = 0;
    for (int i = 0; i < n; ++i) {
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (a[j * n + j] > a[i * n + i] || (a[j * n + j] == a[i * n + i] && j < i)) ? 1 : 0;
        col[rank] = i;
    }
}

inline double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline double dist2(const double *a, const double *b) {
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// qr_solve (:860-950) on copies; false: eta == 0 (E8; X reads 0)
bool qr_solve(const double *A0, const double *b0, int nc, double *X) {
    double A[30], b[6], A1[5], A2[5];
    std::memcpy(A, A0, sizeof(double) * 6 * nc);
    std::memcpy(b, b0, sizeof(double) * 6);
    for (int k = 0; k < nc; ++k) X[k] = 0.0;
    for (int k = 0; k < nc; ++k) {
        double eta = std::fabs(A[k * nc + k]);
        for (int i = k + 1; i < 6; ++i) {
            const double elt = std::fabs(A[i * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0.0) return false;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
        for (int i = k; i < 6; ++i) {
            A[i * nc + k] = A[i * nc + k] * inv_eta;
            sum = sum + A[i * nc + k] * A[i * nc + k];
        }
        double sigma = std::sqrt(sum);
        if (A[k * nc + k] < 0.0) sigma = -sigma;
        A[k * nc + k] = A[k * nc + k] + sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double s2 = 0.0;
            for (int i = k; i < 6; ++i) s2 = s2 + A[i * nc + k] * A[i * nc + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < 6; ++i) A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; ++j) {
        double tau = 0.0;
        for (int i = j; i < 6; ++i) tau = tau + A[i * nc + j] * b[i];
        tau = tau / A1[j];
        for (int i = j; i < 6; ++i) b[i] = b[i] - tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; --i) {
        double sum = 0.0;
        for (int j = i + 1; j < nc; ++j) sum = sum + A[i * nc + j] * X[j];
        X[i] = (b[i] - sum) / A2[i];
    }
    return true;
}

void b01(double b0, double b1, double b2, double &o0, double &o1) {
    if (b0 < 0.0) {
        o0 = std::sqrt(-b0);
        o1 = (b2 < 0.0) ? std::sqrt(-b2) : 0.0;
    } else {
        o0 = std::sqrt(b0);
        o1 = (b2 > 0.0) ? std::sqrt(b2) : 0.0;
    }
    if (b1 < 0.0) o0 = -o0;
}

struct Cand {
    int N;
    const float *p2d, *p3dw, *max_err;
    double fu, fv, uc, vc;
};

// compute_pose (:477-525) over sel[0 .. n); false: degenerate (E8)
bool epnp(const Cand &C, const int *sel, int n, double *R, double *t) {
    const double fn = (double)n, fu = C.fu, fv = C.fv, uc = C.uc, vc = C.vc;
    bool bad = false;
    auto pw = [&](int j, int k) { return (double)C.p3dw[3 * sel[j] + k]; };
    auto us = [&](int j, int k) { return (double)C.p2d[2 * sel[j] + k]; };
    double c0[3], cws[4][3];
    for (int k = 0; k < 3; ++k) {
        Sum s;
        for (int j = 0; j < n; ++j) s.add(pw(j, k));
        c0[k] = s.done() / fn;
        cws[0][k] = c0[k];
    }
    {
        double a[9], v[9];
        for (int x = 0; x < 3; ++x)
            for (int y = x; y < 3; ++y) {
                Sum s;
                for (int j = 0; j < n; ++j) s.add((pw(j, x) - c0[x]) * (pw(j, y) - c0[y]));
                a[3 * x + y] = a[3 * y + x] = s.done();
            }
        jacobi(a, v, 3);
        int col[3];
        order_desc(a, 3, col);
        for (int i = 1; i < 4; ++i) {
            const double k = std::sqrt(a[4 * col[i - 1]] / fn);
            for (int j = 0; j < 3; ++j) cws[i][j] = c0[j] + k * v[3 * j + col[i - 1]];
        }
    }
    double ci[9];
    {
        double m[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 1; j < 4; ++j) m[3 * i + j - 1] = cws[j][i] - cws[0][i];
        const double k0 = m[4] * m[8] - m[5] * m[7], k1 = m[5] * m[6] - m[3] * m[8], k2 = m[3] * m[7] - m[4] * m[6];
        const double inv = 1.0 / (m[0] * k0 + m[1] * k1 + m[2] * k2);
        ci[0] = k0 * inv; ci[1] = (m[2] * m[7] - m[1] * m[8]) * inv; ci[2] = (m[1] * m[5] - m[2] * m[4]) * inv;
        ci[3] = k1 * inv; ci[4] = (m[0] * m[8] - m[2] * m[6]) * inv; ci[5] = (m[2] * m[3] - m[0] * m[5]) * inv;
        ci[6] = k2 * inv; ci[7] = (m[1] * m[6] - m[0] * m[7]) * inv; ci[8] = (m[0] * m[4] - m[1] * m[3]) * inv;
    }
    auto alphas = [&](int j, double *a) {
        const double d0 = pw(j, 0) - c0[0], d1 = pw(j, 1) - c0[1], d2 = pw(j, 2) - c0[2];
        for (int k = 0; k < 3; ++k) a[1 + k] = ci[3 * k] * d0 + ci[3 * k + 1] * d1 + ci[3 * k + 2] * d2;
        a[0] = 1.0 - a[1] - a[2] - a[3];
    };
    double M[144], V[144];
    for (double &x : M) x = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int k = i; k < 4; ++k) {
            Sum s[7];
            for (int j = 0; j < n; ++j) {
                double a[4];
                alphas(j, a);
                const double ai = a[i], ak = a[k], du = uc - us(j, 0), dv = vc - us(j, 1);
                const double Ai = ai * fu, Ak = ak * fu, Bi = ai * fv, Bk = ak * fv, Ci = ai * du, Ck = ak * du, Di = ai * dv, Dk = ak * dv;
                s[0].add(Ai * Ak); s[1].add(Ai * Ck); s[2].add(Bi * Bk); s[3].add(Bi * Dk); s[4].add(Ci * Ck + Di * Dk); s[5].add(Ci * Ak); s[6].add(Di * Bk);
            }
            const int r = 3 * i, c = 3 * k;
            auto put = [&](int x, int y, double val) { M[12 * x + y] = val; M[12 * y + x] = val; };
            put(r, c, s[0].done()); put(r, c + 2, s[1].done()); put(r + 1, c + 1, s[2].done()); put(r + 1, c + 2, s[3].done());
            put(r + 2, c + 2, s[4].done());
            if (i < k) { put(r + 2, c, s[5].done()); put(r + 2, c + 1, s[6].done()); }
        }
    jacobi(M, V, 12);
    int col[12];
    order_desc(M, 12, col);
    double v[4][12];
    for (int i = 0; i < 4; ++i)
        for (int r = 0; r < 12; ++r) v[i][r] = V[12 * r + col[11 - i]];
    double L[60], rho[6];
    {
        double dv[4][6][3];
        for (int i = 0; i < 4; ++i) {
            int a = 0, b = 1;
            for (int j = 0; j < 6; ++j) {
                for (int x = 0; x < 3; ++x) dv[i][j][x] = v[i][3 * a + x] - v[i][3 * b + x];
                if (++b > 3) { ++a; b = a + 1; }
            }
        }
        for (int i = 0; i < 6; ++i) {
            double *row = L + 10 * i;
            row[0] = dot3(dv[0][i], dv[0][i]); row[1] = 2.0 * dot3(dv[0][i], dv[1][i]); row[2] = dot3(dv[1][i], dv[1][i]);
            row[3] = 2.0 * dot3(dv[0][i], dv[2][i]); row[4] = 2.0 * dot3(dv[1][i], dv[2][i]); row[5] = dot3(dv[2][i], dv[2][i]);
            row[6] = 2.0 * dot3(dv[0][i], dv[3][i]); row[7] = 2.0 * dot3(dv[1][i], dv[3][i]); row[8] = 2.0 * dot3(dv[2][i], dv[3][i]);
            row[9] = dot3(dv[3][i], dv[3][i]);
        }
        rho[0] = dist2(cws[0], cws[1]); rho[1] = dist2(cws[0], cws[2]); rho[2] = dist2(cws[0], cws[3]);
        rho[3] = dist2(cws[1], cws[2]); rho[4] = dist2(cws[1], cws[3]); rho[5] = dist2(cws[2], cws[3]);
    }
    double best_e = 0.0;
    for (int ap = 0; ap < 3; ++ap) {
        double betas[4], A[30], X[5];
        if (ap == 0) {
            for (int i = 0; i < 6; ++i) { A[4 * i] = L[10 * i]; A[4 * i + 1] = L[10 * i + 1]; A[4 * i + 2] = L[10 * i + 3]; A[4 * i + 3] = L[10 * i + 6]; }
            if (!qr_solve(A, rho, 4, X)) bad = true;
            if (X[0] < 0.0) {
                betas[0] = std::sqrt(-X[0]);
                betas[1] = -X[1] / betas[0]; betas[2] = -X[2] / betas[0]; betas[3] = -X[3] / betas[0];
            } else {
                betas[0] = std::sqrt(X[0]);
                betas[1] = X[1] / betas[0]; betas[2] = X[2] / betas[0]; betas[3] = X[3] / betas[0];
            }
            if (betas[0] == 0.0) bad = true;
        } else if (ap == 1) {
            for (int i = 0; i < 6; ++i) { A[3 * i] = L[10 * i]; A[3 * i + 1] = L[10 * i + 1]; A[3 * i + 2] = L[10 * i + 2]; }
            if (!qr_solve(A, rho, 3, X)) bad = true;
            b01(X[0], X[1], X[2], betas[0], betas[1]);
            betas[2] = 0.0; betas[3] = 0.0;
        } else {
            for (int i = 0; i < 6; ++i)
                for (int k = 0; k < 5; ++k) A[5 * i + k] = L[10 * i + k];
            if (!qr_solve(A, rho, 5, X)) bad = true;
            b01(X[0], X[1], X[2], betas[0], betas[1]);
            if (betas[0] == 0.0) bad = true;
            betas[2] = X[3] / betas[0];
            betas[3] = 0.0;
        }
        for (int it = 0; it < 5; ++it) {
            double b[6];
            const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
            for (int i = 0; i < 6; ++i) {
                const double *r = L + 10 * i;
                A[4 * i] = 2.0 * r[0] * b0 + r[1] * b1 + r[3] * b2 + r[6] * b3;
                A[4 * i + 1] = r[1] * b0 + 2.0 * r[2] * b1 + r[4] * b2 + r[7] * b3;
                A[4 * i + 2] = r[3] * b0 + r[4] * b1 + 2.0 * r[5] * b2 + r[8] * b3;
                A[4 * i + 3] = r[6] * b0 + r[7] * b1 + r[8] * b2 + 2.0 * r[9] * b3;
                b[i] = rho[i] - (r[0] * b0 * b0 + r[1] * b0 * b1 + r[2] * b1 * b1 + r[3] * b0 * b2 + r[4] * b1 * b2 + r[5] * b2 * b2 +
                                 r[6] * b0 * b3 + r[7] * b1 * b3 + r[8] * b2 * b3 + r[9] * b3 * b3);
            }
            if (!qr_solve(A, b, 4, X)) bad = true;
            for (int k = 0; k < 4; ++k) betas[k] = betas[k] + X[k];
        }
        double ccs[4][3];
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < 3; ++k) ccs[j][k] = 0.0;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
                for (int k = 0; k < 3; ++k) ccs[j][k] = ccs[j][k] + betas[i] * v[i][3 * j + k];
        auto pc = [&](const double *a, int k) { return a[0] * ccs[0][k] + a[1] * ccs[1][k] + a[2] * ccs[2][k] + a[3] * ccs[3][k]; };
        {
            double a[4];
            alphas(0, a);
            if (pc(a, 2) < 0.0)  // Q6
                for (int j = 0; j < 4; ++j)
                    for (int k = 0; k < 3; ++k) ccs[j][k] = -ccs[j][k];
        }
        double pc0[3];
        for (int k = 0; k < 3; ++k) {
            Sum s;
            for (int j = 0; j < n; ++j) {
                double a[4];
                alphas(j, a);
                s.add(pc(a, k));
            }
            pc0[k] = s.done() / fn;
        }
        double Am[9], Ra[9], ta[3];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) {
                Sum s;
                for (int j = 0; j < n; ++j) {
                    double a[4];
                    alphas(j, a);
                    s.add((pc(a, r) - pc0[r]) * (pw(j, k) - c0[k]));
                }
                Am[3 * r + k] = s.done();
            }
        {
            double ata[9], VV[9];
            for (int i = 0; i < 3; ++i)
                for (int j = i; j < 3; ++j) ata[3 * i + j] = ata[3 * j + i] = Am[i] * Am[j] + Am[3 + i] * Am[3 + j] + Am[6 + i] * Am[6 + j];
            jacobi(ata, VV, 3);
            int cl[3];
            order_desc(ata, 3, cl);
            double vk[3][3], Av[3][3], uk[3][3];
            for (int k = 0; k < 3; ++k)
                for (int r = 0; r < 3; ++r) vk[k][r] = VV[3 * r + cl[k]];
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < 3; ++i) Av[k][i] = Am[3 * i] * vk[k][0] + Am[3 * i + 1] * vk[k][1] + Am[3 * i + 2] * vk[k][2];
            for (int k = 0; k < 2; ++k) {
                const double nrm = std::sqrt(Av[k][0] * Av[k][0] + Av[k][1] * Av[k][1] + Av[k][2] * Av[k][2]);
                for (int i = 0; i < 3; ++i) uk[k][i] = Av[k][i] / nrm;
            }
            uk[2][0] = uk[0][1] * uk[1][2] - uk[0][2] * uk[1][1];
            uk[2][1] = uk[0][2] * uk[1][0] - uk[0][0] * uk[1][2];
            uk[2][2] = uk[0][0] * uk[1][1] - uk[0][1] * uk[1][0];
            if (dot3(Av[2], uk[2]) < 0.0) { vk[2][0] = -vk[2][0]; vk[2][1] = -vk[2][1]; vk[2][2] = -vk[2][2]; }
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) Ra[3 * i + j] = uk[0][i] * vk[0][j] + uk[1][i] * vk[1][j] + uk[2][i] * vk[2][j];
            const double det = Ra[0] * Ra[4] * Ra[8] + Ra[1] * Ra[5] * Ra[6] + Ra[2] * Ra[3] * Ra[7] - Ra[2] * Ra[4] * Ra[6] - Ra[1] * Ra[3] * Ra[8] -
                               Ra[0] * Ra[5] * Ra[7];
            if (det < 0.0) { Ra[6] = -Ra[6]; Ra[7] = -Ra[7]; Ra[8] = -Ra[8]; }
            for (int i = 0; i < 3; ++i) ta[i] = pc0[i] - dot3(Ra + 3 * i, c0);
        }
        Sum se;
        for (int j = 0; j < n; ++j) {
            const double p[3] = {pw(j, 0), pw(j, 1), pw(j, 2)};
            const double Xc = dot3(Ra, p) + ta[0], Yc = dot3(Ra + 3, p) + ta[1], inv_Zc = 1.0 / (dot3(Ra + 6, p) + ta[2]);
            const double ue = uc + fu * Xc * inv_Zc, ve = vc + fv * Yc * inv_Zc, u = us(j, 0), w = us(j, 1);
            se.add(std::sqrt((u - ue) * (u - ue) + (w - ve) * (w - ve)));
        }
        const double err = se.done() / fn;
        if (ap == 0 || (std::isfinite(err) && (!std::isfinite(best_e) || err < best_e))) {
            best_e = err;
            std::memcpy(R, Ra, sizeof(Ra));
            std::memcpy(t, ta, sizeof(ta));
        }
    }
    bool ok = !bad;
    for (int k = 0; k < 9; ++k) ok = ok && std::isfinite(R[k]);
    for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(t[k]);
    return ok;
}

// CheckInliers (:308-339, Q5) + the outputs of one hypothesis
int check(const Cand &C, bool ok, const double *R, const double *t, int mask_words, float *pose, uint32_t *words) {
    for (int k = 0; k < 12; ++k) pose[k] = ok ? (float)(k < 9 ? R[k] : t[k - 9]) : 0.0f;
    for (int w = 0; w < mask_words; ++w) words[w] = 0;
    if (!ok) return 0;
    int count = 0;
    for (int k = 0; k < C.N; ++k) {
        const double X = (double)C.p3dw[3 * k], Y = (double)C.p3dw[3 * k + 1], Z = (double)C.p3dw[3 * k + 2];
        const float Xc = (float)(R[0] * X + R[1] * Y + R[2] * Z + t[0]);
        const float Yc = (float)(R[3] * X + R[4] * Y + R[5] * Z + t[1]);
        const float invZc = (float)(1.0 / (R[6] * X + R[7] * Y + R[8] * Z + t[2]));
        const double ue = C.uc + C.fu * (double)Xc * (double)invZc;
        const double ve = C.vc + C.fv * (double)Yc * (double)invZc;
        const float distX = (float)((double)C.p2d[2 * k] - ue);
        const float distY = (float)((double)C.p2d[2 * k + 1] - ve);
        const float error2 = distX * distX + distY * distY;
        if (error2 < C.max_err[k]) {
            words[k >> 5] |= 1u << (k & 31);
            ++count;
        }
    }
    return count;
}

}  // namespace

// cam = fx, fy, cx, cy; x / y / sigma2 [nf]: the frame; pos [P][3], flags [P] (1 = set, 2 = bad): the store; pts [nc][nf].
// stops: null, or per candidate the number of hypotheses to evaluate (at most nhyp; 0 = the candidate's constructor only): what a
// round-robin iterate loop that has returned left each solver at.  The rows keep the pitch of nhyp; those from the stop on are not written
extern "C" void pnp_host(int nc, int nf, int nhyp, int mask_words, const int32_t *stops, const float *cam, const uint64_t *seeds, int min_inliers_in, float epsilon,
                         float th2, const float *x, const float *y, const float *sigma2, const float *pos, const uint8_t *flags,
                         const int32_t *pts, int32_t *n_out, int32_t *min_inliers, int32_t *index, int32_t *count, uint8_t *degenerate,
                         float *pose, uint32_t *inliers, uint8_t *refined, int32_t *refined_count, float *refined_pose,
                         uint32_t *refined_inliers) {
    std::vector<float> p2d((size_t)nf * 2), p3dw((size_t)nf * 3), me((size_t)nf);
    std::vector<int> avail, sel;
    for (int c = 0; c < nc; ++c) {
        const size_t row0 = (size_t)c * nf;
        int N = 0;
        for (int i = 0; i < nf; ++i) {  // the constructor
            const int p = pts[row0 + i];
            index[row0 + i] = -1;
            if (p < 0 || !(flags[p] & 1) || (flags[p] & 2)) continue;
            index[row0 + N] = i;
            p2d[2 * N] = x[i]; p2d[2 * N + 1] = y[i];
            p3dw[3 * N] = pos[3 * p]; p3dw[3 * N + 1] = pos[3 * p + 1]; p3dw[3 * N + 2] = pos[3 * p + 2];
            me[N] = sigma2[i] * th2;
            ++N;
        }
        n_out[c] = N;
        const float prod = (float)N * epsilon;
        int n_min = !(prod < 2147483648.0f) ? 2147483647 : (int)prod;
        if (n_min < min_inliers_in) n_min = min_inliers_in;
        if (n_min < 4) n_min = 4;
        min_inliers[c] = n_min;
        const Cand C{N, p2d.data(), p3dw.data(), me.data(), (double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3]};
        int best = 0;
        const int stop = stops ? (stops[c] < nhyp ? stops[c] : nhyp) : nhyp;
        for (int h = 0; h < stop; ++h) {
            const size_t ho = (size_t)c * nhyp + h;
            float *ps = pose + ho * 12, *rps = refined_pose + ho * 12;
            uint32_t *w = inliers + ho * mask_words, *rw = refined_inliers + ho * mask_words;
            double R[9] = {0}, t[3] = {0};
            bool ok = false;
            if (N >= 4) {  // E9
                const uint64_t key = sm(sm(seeds[c]) ^ (uint64_t)(h + 1));
                avail.resize((size_t)N);
                for (int k = 0; k < N; ++k) avail[(size_t)k] = k;
                int pick[4];
                for (int d = 0; d < 4; ++d) {  // E6
                    const int r = (int)(sm(key + (uint64_t)(d + 1) * 0xD1342543DE82EF95ull) % (uint64_t)(N - d));
                    pick[d] = avail[(size_t)r];
                    avail[(size_t)r] = avail.back();
                    avail.pop_back();
                }
                ok = epnp(C, pick, 4, R, t);
            }
            degenerate[ho] = (N >= 4 && !ok) ? 1 : 0;
            count[ho] = check(C, ok, R, t, mask_words, ps, w);
            bool rok = false;
            const bool record = N >= 4 && count[ho] >= n_min && count[ho] > best;
            if (record) {
                best = count[ho];
                sel.clear();
                for (int k = 0; k < N; ++k)
                    if ((w[k >> 5] >> (k & 31)) & 1u) sel.push_back(k);
                rok = epnp(C, sel.data(), (int)sel.size(), R, t);
            }
            refined[ho] = record ? (rok ? 1 : 2) : 0;
            refined_count[ho] = check(C, rok, R, t, mask_words, rps, rw);
        }
    }
}
