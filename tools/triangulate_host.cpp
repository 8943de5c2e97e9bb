// triangulate_host — the match loop of LocalMapping::CreateNewMapPoints as a scalar host program: the algorithm of csrc/k_triangulate.hip
// (tests/_tri_ref.py is the normative text), statement for statement, for tools/time_triangulate.py (g++ -O3 -ffp-contract=off).  Its
// answers equal the device's bit for bit; the points it creates come back as the packed arrays afv_points_set takes.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {
struct Job {  // afv_tri_points_job without struct_size
    float R1[9], t1[3], O1[3], R2[9], t2[3], O2[3];
    float fx1, fy1, cx1, cy1, invfx1, invfy1, fx2, fy2, cx2, cy2, invfx2, invfy2;
    float mb1, mb2, mbf1, ratio_factor, max_size1;
};
struct Planes {  // one keyframe: [8][cap] x, y, sigma2, u_right, size, depth, x_dist, y_dist
    const float *x, *y, *sigma2, *ur, *size, *depth, *xd, *yd;
};

inline float sum3(float a0, float a1, float a2) { return a0 + (a1 + a2); }
inline float cam(const float *R, const float *t, int row, const float *X) { return sum3(R[3 * row] * X[0], R[3 * row + 1] * X[1], R[3 * row + 2] * X[2]) + t[row]; }
inline float dist(const float *X, const float *O, float *n) {
    for (int k = 0; k < 3; ++k) n[k] = X[k] - O[k];
    return std::sqrt(sum3(n[0] * n[0], n[1] * n[1], n[2] * n[2]));
}
inline float cos_stereo(float mb, float d) {
    const float h = mb / 2.0f, dd = d * d, hh = h * h;
    return (dd - hh) / (dd + hh);
}
inline bool reproj_fails(float fx, float fy, float cx, float cy, float mbf, float x, float y, float invz, float kx, float ky, float kur, bool stereo,
                         float sigma2) {
    const float u = (fx * x) * invz + cx, v = (fy * y) * invz + cy, ex = u - kx, ey = v - ky;
    float e2 = ex * ex + ey * ey;
    if (!stereo) return (double)e2 > 5.991 * (double)sigma2;
    const float er = (u - mbf * invz) - kur;
    e2 = e2 + er * er;
    return (double)e2 > 7.8 * (double)sigma2;
}

void null_vector(float At[4][4], float *v) {
    float Vt[4][4];
    double W[4];
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double t = At[i][k];
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
                if (std::fabs(p) <= (double)(FLT_EPSILON * 2.0f) * std::sqrt(a * b)) continue;
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
                    const float t0 = c * At[i][k] + s * At[j][k], t1 = ms * At[i][k] + c * At[j][k];
                    At[i][k] = t0; At[j][k] = t1;
                    a = a + (double)t0 * (double)t0;
                    b = b + (double)t1 * (double)t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                for (int k = 0; k < 4; ++k) {
                    const float t0 = c * Vt[i][k] + s * Vt[j][k], t1 = ms * Vt[i][k] + c * Vt[j][k];
                    Vt[i][k] = t0; Vt[j][k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
        for (int k = 0; k < 4; ++k) {
            const double t = At[i][k];
            sd = sd + t * t;
        }
        W[i] = std::sqrt(sd);
    }
    int at[4] = {0, 1, 2, 3};
    for (int i = 0; i < 3; ++i) {
        int j = i;
        for (int k = i + 1; k < 4; ++k)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            const int ta = at[i]; at[i] = at[j]; at[j] = ta;
        }
    }
    for (int k = 0; k < 4; ++k) v[k] = Vt[at[3]][k];
}

// -> status; route and X are written
int one_match(const Job &J, const Planes &A, int i, const Planes &B, int j, int *route, float *X) {
    *route = 0;
    X[0] = X[1] = X[2] = 0.0f;
    const float kx1 = A.x[i], ky1 = A.y[i], ur1 = A.ur[i], kx2 = B.x[j], ky2 = B.y[j], ur2 = B.ur[j];
    const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
    const float xn1[3] = {(kx1 - J.cx1) * J.invfx1, (ky1 - J.cy1) * J.invfy1, 1.0f}, xn2[3] = {(kx2 - J.cx2) * J.invfx2, (ky2 - J.cy2) * J.invfy2, 1.0f};
    float r1[3], r2[3];
    for (int k = 0; k < 3; ++k) {
        r1[k] = sum3(J.R1[k] * xn1[0], J.R1[3 + k] * xn1[1], J.R1[6 + k] * xn1[2]);
        r2[k] = sum3(J.R2[k] * xn2[0], J.R2[3 + k] * xn2[1], J.R2[6 + k] * xn2[2]);
    }
    const float dot = sum3(r1[0] * r2[0], r1[1] * r2[1], r1[2] * r2[2]);
    const float nr1 = std::sqrt(sum3(r1[0] * r1[0], r1[1] * r1[1], r1[2] * r1[2])), nr2 = std::sqrt(sum3(r2[0] * r2[0], r2[1] * r2[1], r2[2] * r2[2]));
    const float cos_rays = dot / (nr1 * nr2);
    float cs = cos_rays + 1.0f, cs1 = cs, cs2 = cs;
    if (st1) cs1 = cos_stereo(J.mb1, A.depth[i]);
    else if (st2) cs2 = cos_stereo(J.mb2, B.depth[j]);
    cs = cs2 < cs1 ? cs2 : cs1;
    if (cos_rays < cs && cos_rays > 0 && (st1 || st2 || (double)cos_rays < 0.9998)) {
        float At[4][4], v[4];
        for (int col = 0; col < 4; ++col) {
            const float a2 = col < 3 ? J.R1[6 + col] : J.t1[2], a0 = col < 3 ? J.R1[col] : J.t1[0], a1 = col < 3 ? J.R1[3 + col] : J.t1[1];
            const float b2 = col < 3 ? J.R2[6 + col] : J.t2[2], b0 = col < 3 ? J.R2[col] : J.t2[0], b1 = col < 3 ? J.R2[3 + col] : J.t2[1];
            At[col][0] = xn1[0] * a2 - a0;
            At[col][1] = xn1[1] * a2 - a1;
            At[col][2] = xn2[0] * b2 - b0;
            At[col][3] = xn2[1] * b2 - b1;
        }
        null_vector(At, v);
        if (v[3] == 0) return 3;
        for (int k = 0; k < 3; ++k) X[k] = v[k] / v[3];
    } else if ((st1 && cs1 < cs2) || (st2 && cs2 < cs1)) {
        const bool a = st1 && cs1 < cs2;
        *route = a ? 1 : 2;
        const float z = a ? A.depth[i] : B.depth[j];
        const float *R = a ? J.R1 : J.R2, *O = a ? J.O1 : J.O2;
        if (z > 0) {
            const float u = a ? A.xd[i] : B.xd[j], v = a ? A.yd[i] : B.yd[j];
            const float x = ((u - (a ? J.cx1 : J.cx2)) * z) * (a ? J.invfx1 : J.invfx2), y = ((v - (a ? J.cy1 : J.cy2)) * z) * (a ? J.invfy1 : J.invfy2);
            for (int k = 0; k < 3; ++k) X[k] = sum3(R[k] * x, R[3 + k] * y, R[6 + k] * z) + O[k];
        } else {
            X[2] = -1.0f;
        }
    } else {
        return 2;
    }
    if (!(std::isfinite(X[0]) && std::isfinite(X[1]) && std::isfinite(X[2]))) return 10;
    const float z1 = cam(J.R1, J.t1, 2, X);
    if (z1 <= 0) return 4;
    const float z2 = cam(J.R2, J.t2, 2, X);
    if (z2 <= 0) return 5;
    if (reproj_fails(J.fx1, J.fy1, J.cx1, J.cy1, J.mbf1, cam(J.R1, J.t1, 0, X), cam(J.R1, J.t1, 1, X), 1.0f / z1, kx1, ky1, ur1, st1, A.sigma2[i])) return 6;
    if (reproj_fails(J.fx2, J.fy2, J.cx2, J.cy2, J.mbf1, cam(J.R2, J.t2, 0, X), cam(J.R2, J.t2, 1, X), 1.0f / z2, kx2, ky2, ur2, st2, B.sigma2[j])) return 7;
    float n1[3], n2[3];
    const float d1 = dist(X, J.O1, n1), d2 = dist(X, J.O2, n2);
    if (d1 == 0 || d2 == 0) return 8;
    const float ratio_dist = d2 / d1, ratio_octave = A.size[i] / B.size[j];
    if (ratio_dist * J.ratio_factor < ratio_octave || ratio_dist > ratio_octave * J.ratio_factor) return 9;
    return 1;
}

Planes planes(const float *base, int cap) {
    return Planes{base, base + cap, base + 2 * cap, base + 3 * cap, base + 4 * cap, base + 5 * cap, base + 6 * cap, base + 7 * cap};
}
}  // namespace

// planes_a: [8][cap] of the current keyframe (n_a features); planes_b: [npairs][8][cap]; jobs: [npairs][47]; match12: [npairs][cap].
// Outputs: status / route [npairs][cap], x3d [npairs][cap][3]; the created points in creation order: pos / normal [n][3], f5 [5][max_new]
// (min_d, max_d, ref_size, ref_dist, ref_sigma), feat [n] (feature of a).  Returns their number (points beyond max_new are counted, not kept).
extern "C" int triangulate_host(int npairs, int cap, int n_a, const float *planes_a, const float *planes_b, const float *jobs, const int32_t *match12,
                                uint8_t *status, uint8_t *route, float *x3d, int max_new, float *pos, float *normal, float *f5, int32_t *feat) {
    const Planes A = planes(planes_a, cap);
    int made = 0;
    for (int p = 0; p < npairs; ++p) {
        Job J;
        std::memcpy(&J, jobs + (size_t)p * 47, sizeof(J));
        const Planes B = planes(planes_b + (size_t)p * 8 * cap, cap);
        for (int i = 0; i < cap; ++i) {
            const size_t o = (size_t)p * cap + i;
            const int j = i < n_a ? match12[o] : -1;
            int r = 0;
            float X[3] = {0.0f, 0.0f, 0.0f};
            const int s = j >= 0 ? one_match(J, A, i, B, j, &r, X) : 0;
            status[o] = (uint8_t)s;
            route[o] = (uint8_t)r;
            std::memcpy(x3d + 3 * o, X, sizeof(X));
            if (s != 1) continue;
            if (made < max_new) {
                float n1[3], n2[3];
                const float d1 = dist(X, J.O1, n1), d2 = dist(X, J.O2, n2), size = A.size[i], max_d = d1 * size;
                for (int k = 0; k < 3; ++k) {
                    pos[3 * made + k] = X[k];
                    normal[3 * made + k] = ((0.0f + n1[k] / d1) + n2[k] / d2) / 2.0f;
                }
                f5[made] = max_d / J.max_size1;
                f5[max_new + made] = max_d;
                f5[2 * max_new + made] = size;
                f5[3 * max_new + made] = d1;
                f5[4 * max_new + made] = std::sqrt(A.sigma2[i]);
                feat[made] = i;
            }
            ++made;
        }
    }
    return made;
}
