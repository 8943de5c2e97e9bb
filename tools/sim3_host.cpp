// sim3_host.cpp — the restatement of Sim3Solver (tests/_sim3_ref.py: the constructor and every RANSAC hypothesis of every candidate, quirks
// Q1-Q3, deviations S1-S6 of include/afv_hip.h) as a scalar host program: what afv_table_sim3_hypotheses is timed against
// (tools/time_sim3.py compiles it with g++ -O3 -ffp-contract=off and checks its answers bit-equal to the device's in the same run).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

inline float sum3(float a0, float a1, float a2) { return a0 + (a1 + a2); }
inline float row(const float *R, const float *t, int r, const float *X) { return sum3(R[3 * r] * X[0], R[3 * r + 1] * X[1], R[3 * r + 2] * X[2]) + t[r]; }
inline float bound(float s2) { return (!(s2 >= 0.0f) || !std::isfinite(s2)) ? 0.0f : (float)std::trunc(9.210 * (double)s2); }
inline uint64_t sm(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

bool rotate(double (&a)[4][4], double (&v)[4][4], int p, int q) {
    const double apq = a[p][q], app = a[p][p], aqq = a[q][q];
    if (apq == 0.0) return false;
    const double g = std::fabs(apq);
    if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
    for (int k = 0; k < 4; ++k) {
        if (k == p || k == q) continue;
        const double akp = a[k][p], akq = a[k][q];
        const double np = c * akp - s * akq, nq = s * akp + c * akq;
        a[k][p] = a[p][k] = np;
        a[k][q] = a[q][k] = nq;
    }
    a[p][p] = app - t * apq;
    a[q][q] = aqq + t * apq;
    a[p][q] = a[q][p] = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
    }
    return true;
}

void centroid(const float (&P)[3][3], float (&Pr)[3][3], float (&C)[3]) {
    for (int r = 0; r < 3; ++r) {
        C[r] = sum3(P[r][0], P[r][1], P[r][2]) / 3.0f;
        for (int i = 0; i < 3; ++i) Pr[r][i] = P[r][i] - C[r];
    }
}

bool solve(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, float (&R)[9], float (&t)[3], float &s, float (&sR)[9], float (&sRi)[9],
           float (&ti)[3]) {
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3], M[3][3];
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[r][c] = sum3(Pr2[r][0] * Pr1[c][0], Pr2[r][1] * Pr1[c][1], Pr2[r][2] * Pr1[c][2]);
    const float n00 = M[0][0] + M[1][1] + M[2][2], n01 = M[1][2] - M[2][1], n02 = M[2][0] - M[0][2], n03 = M[0][1] - M[1][0];
    const float n11 = M[0][0] - M[1][1] - M[2][2], n12 = M[0][1] + M[1][0], n13 = M[2][0] + M[0][2];
    const float n22 = -M[0][0] + M[1][1] - M[2][2], n23 = M[1][2] + M[2][1], n33 = -M[0][0] - M[1][1] + M[2][2];
    double a[4][4] = {{n00, n01, n02, n03}, {n01, n11, n12, n13}, {n02, n12, n22, n23}, {n03, n13, n23, n33}};  // S1
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 12; ++sweep) {  // S2
        bool any = false;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) any |= rotate(a, v, p, q);
        if (!any) break;
    }
    int best = 0;
    for (int k = 1; k < 4; ++k)
        if (a[k][k] > a[best][best]) best = k;
    const double q0 = v[0][best], q1 = v[1][best], q2 = v[2][best], q3 = v[3][best];
    const double nrm = std::sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);  // S3
    const double w = q0 / nrm, x = q1 / nrm, y = q2 / nrm, z = q3 / nrm;
    R[0] = (float)(1.0 - 2.0 * (y * y + z * z)); R[1] = (float)(2.0 * (x * y - w * z)); R[2] = (float)(2.0 * (x * z + w * y));
    R[3] = (float)(2.0 * (x * y + w * z)); R[4] = (float)(1.0 - 2.0 * (x * x + z * z)); R[5] = (float)(2.0 * (y * z - w * x));
    R[6] = (float)(2.0 * (x * z - w * y)); R[7] = (float)(2.0 * (y * z + w * x)); R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
    bool ok = true;
    for (float r : R) ok = ok && std::isfinite(r);
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const float p3 = sum3(R[3 * r] * Pr2[0][c], R[3 * r + 1] * Pr2[1][c], R[3 * r + 2] * Pr2[2][c]);
                nom = nom + (double)Pr1[r][c] * (double)p3;
                const float sq = p3 * p3;
                den = den + (double)sq;
            }
        ok = ok && std::isfinite(den) && den != 0.0;
        s = (float)(nom / den);
    } else {
        s = 1.0f;
    }
    ok = ok && std::isfinite(s);
    const float inv_s = 1.0f / s;
    for (int k = 0; k < 9; ++k) sR[k] = s * R[k];
    for (int r = 0; r < 3; ++r) {
        t[r] = O1[r] - sum3(sR[3 * r] * O2[0], sR[3 * r + 1] * O2[1], sR[3 * r + 2] * O2[2]);
        ok = ok && std::isfinite(t[r]);
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) sRi[3 * r + c] = inv_s * R[3 * c + r];
    for (int r = 0; r < 3; ++r) ti[r] = sum3(-sRi[3 * r] * t[0], -sRi[3 * r + 1] * t[1], -sRi[3 * r + 2] * t[2]);
    return ok;
}

inline float err(const float *R, const float *t, const float *K, const float *X, const float *im, bool first_minus_projected) {
    const float x = row(R, t, 0, X), y = row(R, t, 1, X), z = row(R, t, 2, X);
    const float invz = 1.0f / z;
    const float u = K[0] * (x * invz) + K[2], v = K[1] * (y * invz) + K[3];
    const float d0 = first_minus_projected ? im[0] - u : u - im[0], d1 = first_minus_projected ? im[1] - v : v - im[1];
    return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}

}  // namespace

// cams [nc][32]: Rcw1[9] tcw1[3] fx1 fy1 cx1 cy1 Rcw2[9] tcw2[3] fx2 fy2 cx2 cy2; seeds [nc]; n1 [nc]; pos [npoints][3], flags [npoints] (1 = set,
// 2 = bad); sigma2_1 / sigma2_2 [nc][cap]; mp1 / mp2 / idx1 / idx2 [nc][cap].  Outputs as afv_table_sim3_hypotheses writes them.
extern "C" void sim3_host(int nc, int cap, int nhyp, int mask_words, int fix_scale, const float *cams, const uint64_t *seeds, const int32_t *n1s,
                          const float *pos, const uint8_t *flags, const float *sigma2_1, const float *sigma2_2, const int32_t *mp1,
                          const int32_t *mp2, const int32_t *idx1, const int32_t *idx2, int32_t *n_out, int32_t *index1, int32_t *count,
                          uint8_t *degenerate, float *sim3, uint32_t *inliers) {
    std::vector<float> x1((size_t)cap * 3), x2((size_t)cap * 3), im1((size_t)cap * 2), im2((size_t)cap * 2), me((size_t)cap * 2);
    std::vector<int> all, avail;
    for (int c = 0; c < nc; ++c) {
        const float *J = cams + (size_t)c * 32;
        const float *R1 = J, *t1 = J + 9, *K1 = J + 12, *R2 = J + 16, *t2 = J + 25, *K2 = J + 28;
        const size_t row0 = (size_t)c * cap;
        int N = 0;
        for (int i1 = 0; i1 < n1s[c]; ++i1) {  // the constructor
            const int p2 = mp2[row0 + i1], p1 = mp1[row0 + i1], k1 = idx1[row0 + i1], k2 = idx2[row0 + i1];
            if (p2 < 0 || p1 < 0) continue;
            if (!(flags[p1] & 1) || (flags[p1] & 2) || !(flags[p2] & 1) || (flags[p2] & 2)) continue;
            if (k1 < 0 || k2 < 0) continue;
            index1[row0 + N] = i1;
            for (int r = 0; r < 3; ++r) {
                x1[3 * N + r] = row(R1, t1, r, pos + 3 * (size_t)p1);
                x2[3 * N + r] = row(R2, t2, r, pos + 3 * (size_t)p2);
            }
            const float iz1 = 1.0f / x1[3 * N + 2], iz2 = 1.0f / x2[3 * N + 2];
            im1[2 * N] = K1[0] * (x1[3 * N] * iz1) + K1[2]; im1[2 * N + 1] = K1[1] * (x1[3 * N + 1] * iz1) + K1[3];
            im2[2 * N] = K2[0] * (x2[3 * N] * iz2) + K2[2]; im2[2 * N + 1] = K2[1] * (x2[3 * N + 1] * iz2) + K2[3];
            me[2 * N] = bound(sigma2_1[row0 + k1]);
            me[2 * N + 1] = bound(sigma2_2[row0 + k2]);
            ++N;
        }
        n_out[c] = N;
        for (int k = N; k < cap; ++k) index1[row0 + k] = -1;
        all.resize((size_t)N);
        for (int k = 0; k < N; ++k) all[(size_t)k] = k;
        for (int h = 0; h < nhyp; ++h) {
            const size_t ho = (size_t)c * nhyp + h;
            uint32_t *words = inliers + ho * mask_words;
            float *rec = sim3 + ho * 13;
            std::memset(words, 0, (size_t)mask_words * 4);
            std::memset(rec, 0, 13 * 4);
            count[ho] = 0;
            degenerate[ho] = 0;
            if (N < 3) continue;  // S6
            const uint64_t key = sm(sm(seeds[c]) ^ (uint64_t)(h + 1)), step = 0xD1342543DE82EF95ull;  // S4
            int picks[3];
            avail = all;  // vAvailableIndices = mvAllIndices (:161)
            for (int d = 0; d < 3; ++d) {
                const size_t r = (size_t)(sm(key + (uint64_t)(d + 1) * step) % (uint64_t)(N - d));
                picks[d] = avail[r];
                avail[r] = avail.back();
                avail.pop_back();
            }
            float P1[3][3], P2[3][3], R[9], t[3], s, sR[9], sRi[9], ti[3];
            for (int i = 0; i < 3; ++i)
                for (int r = 0; r < 3; ++r) { P1[r][i] = x1[3 * picks[i] + r]; P2[r][i] = x2[3 * picks[i] + r]; }
            if (!solve(P1, P2, fix_scale != 0, R, t, s, sR, sRi, ti)) {  // S5
                degenerate[ho] = 1;
                continue;
            }
            std::memcpy(rec, R, sizeof(R));
            std::memcpy(rec + 9, t, sizeof(t));
            rec[12] = s;
            int cnt = 0;
            for (int k = 0; k < N; ++k) {
                const float e1 = err(sR, t, K1, &x2[3 * k], &im1[2 * k], true), e2 = err(sRi, ti, K2, &x1[3 * k], &im2[2 * k], false);
                if (e1 < me[2 * k] && e2 < me[2 * k + 1]) { words[k >> 5] |= 1u << (k & 31); ++cnt; }
            }
            count[ho] = cnt;
        }
    }
}
