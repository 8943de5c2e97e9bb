// k_tri_match.h - the judgement of ONE match of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:315-461) and the map point an accepted
// match becomes (MapPoint.cc:372-418).  One copy of the program text for the kernels that run it: k_tri_points / k_tri_store
// (k_triangulate.hip: matches arrive as match12 rows) and k_newpts_judge / k_newpts_store (k_newpoints.hip: the match comes out of the
// row search in the same lane).  The arithmetic, its quirks (Q1, Q2) and its deliberate deviations (T1 - T3) are described at the top of
// k_triangulate.hip.
#pragma once
#include "afv_device.h"
#include "afv_runtime.h"

#define TRI_T AFV_TRI_T
#define TRI_WAVES (TRI_T / 64)

enum { TS_NONE = 0, TS_ACCEPTED, TS_LOW_PARALLAX, TS_W_ZERO, TS_Z1, TS_Z2, TS_REPROJ1, TS_REPROJ2, TS_ZERO_DIST, TS_RATIO, TS_NOT_FINITE };
enum { TR_TRIANGULATED = 0, TR_UNPROJECT_A = 1, TR_UNPROJECT_B = 2 };

__device__ __forceinline__ float tri_sum3(float a0, float a1, float a2) { return a0 + (a1 + a2); }
__device__ __forceinline__ float tri_cam(const float *R, const float *t, int row, float X, float Y, float Z) {
    return tri_sum3(R[3 * row] * X, R[3 * row + 1] * Y, R[3 * row + 2] * Z) + t[row];
}
__device__ __forceinline__ float tri_dist(float X, float Y, float Z, const float *O, float *n) {
    n[0] = X - O[0]; n[1] = Y - O[1]; n[2] = Z - O[2];
    return sqrtf(tri_sum3(n[0] * n[0], n[1] * n[1], n[2] * n[2]));
}
__device__ __forceinline__ float tri_cos_stereo(float mb, float d) {  // T1
    const float h = mb / 2.0f, dd = d * d, hh = h * h;
    return (dd - hh) / (dd + hh);
}
__device__ __forceinline__ bool tri_reproj_fails(float fx, float fy, float cx, float cy, float mbf, float x, float y, float invz, float kx, float ky,
                                                 float kur, bool stereo, float sigma2) {
    const float u = (fx * x) * invz + cx, v = (fy * y) * invz + cy;
    const float ex = u - kx, ey = v - ky;
    float e2 = ex * ex + ey * ey;
    if (!stereo) return (double)e2 > 5.991 * (double)sigma2;
    const float er = (u - mbf * invz) - kur;
    e2 = e2 + er * er;
    return (double)e2 > 7.8 * (double)sigma2;
}

// one rotation of rows i and j (compile-time indices: everything stays in registers)
template <int I, int J>
__device__ __forceinline__ bool tri_rotate(float (&At)[4][4], float (&Vt)[4][4], double (&W)[4]) {
    double a = W[I], b = W[J], p = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) p = p + (double)At[I][k] * (double)At[J][k];
    if (fabs(p) <= (double)(__FLT_EPSILON__ * 2.0f) * sqrt(a * b)) return false;
    p = p * 2.0;
    const double beta = a - b, gamma = sqrt(p * p + beta * beta);  // T2
    float c, s;
    if (beta < 0) {
        const double delta = (gamma - beta) * 0.5;
        s = (float)sqrt(delta / gamma);
        c = (float)(p / (gamma * (double)s * 2.0));
    } else {
        c = (float)sqrt((gamma + beta) / (gamma * 2.0));
        s = (float)(p / (gamma * (double)c * 2.0));
    }
    a = b = 0.0;
    const float ms = -s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t0 = c * At[I][k] + s * At[J][k];
        const float t1 = ms * At[I][k] + c * At[J][k];
        At[I][k] = t0; At[J][k] = t1;
        a = a + (double)t0 * (double)t0;
        b = b + (double)t1 * (double)t1;
    }
    W[I] = a; W[J] = b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t0 = c * Vt[I][k] + s * Vt[J][k];
        const float t1 = ms * Vt[I][k] + c * Vt[J][k];
        Vt[I][k] = t0; Vt[J][k] = t1;
    }
    return true;
}

// vt.row(3) of cv::SVD::compute(A): At holds A transposed on entry
__device__ __forceinline__ void tri_null_vector(float (&At)[4][4], float (&v)[4]) {
    float Vt[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double t = (double)At[i][k];
            sd = sd + t * t;
            Vt[i][k] = i == k ? 1.0f : 0.0f;
        }
        W[i] = sd;
    }
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = tri_rotate<0, 1>(At, Vt, W);
        changed = tri_rotate<0, 2>(At, Vt, W) || changed;
        changed = tri_rotate<0, 3>(At, Vt, W) || changed;
        changed = tri_rotate<1, 2>(At, Vt, W) || changed;
        changed = tri_rotate<1, 3>(At, Vt, W) || changed;
        changed = tri_rotate<2, 3>(At, Vt, W) || changed;
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double t = (double)At[i][k];
            sd = sd + t * t;
        }
        W[i] = sqrt(sd);
    }
    // the descending selection sort: only the row that ends in place 3 is wanted, so the rows are followed through `at`
    int at[4] = {0, 1, 2, 3};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int j = i;
#pragma unroll
        for (int k = i + 1; k < 4; ++k)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            const int ta = at[i]; at[i] = at[j]; at[j] = ta;
        }
    }
    const int r = at[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = r == 0 ? Vt[0][k] : r == 1 ? Vt[1][k] : r == 2 ? Vt[2][k] : Vt[3][k];
}

// feature i of keyframe a against feature j of keyframe b (j < 0: no match): the status; route and x3D through the references
__device__ __forceinline__ int tri_judge(const DevTriPair &J, int i, int j, int &route, float &X, float &Y, float &Z) {
    int status = TS_NONE;
    route = TR_TRIANGULATED;
    X = 0.0f; Y = 0.0f; Z = 0.0f;
    if (j >= 0) {
        const float kx1 = J.x1[i], ky1 = J.y1[i], ur1 = J.ur1[i];
        const float kx2 = J.x2[j], ky2 = J.y2[j], ur2 = J.ur2[j];
        const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
        const float xn1x = (kx1 - J.cx1) * J.invfx1, xn1y = (ky1 - J.cy1) * J.invfy1;
        const float xn2x = (kx2 - J.cx2) * J.invfx2, xn2y = (ky2 - J.cy2) * J.invfy2;
        float r1[3], r2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            r1[k] = tri_sum3(J.R1[k] * xn1x, J.R1[3 + k] * xn1y, J.R1[6 + k] * 1.0f);
            r2[k] = tri_sum3(J.R2[k] * xn2x, J.R2[3 + k] * xn2y, J.R2[6 + k] * 1.0f);
        }
        const float dot = tri_sum3(r1[0] * r2[0], r1[1] * r2[1], r1[2] * r2[2]);
        const float nr1 = sqrtf(tri_sum3(r1[0] * r1[0], r1[1] * r1[1], r1[2] * r1[2]));
        const float nr2 = sqrtf(tri_sum3(r2[0] * r2[0], r2[1] * r2[1], r2[2] * r2[2]));
        const float cos_rays = dot / (nr1 * nr2);
        float cs = cos_rays + 1.0f, cs1 = cs, cs2 = cs;
        if (st1) cs1 = tri_cos_stereo(J.mb1, J.depth1[i]);
        else if (st2) cs2 = tri_cos_stereo(J.mb2, J.depth2[j]);
        cs = cs2 < cs1 ? cs2 : cs1;  // std::min(cs1, cs2)
        bool have = true;
        if (cos_rays < cs && cos_rays > 0 && (st1 || st2 || (double)cos_rays < 0.9998)) {
            float At[4][4], v[4];  // A transposed: At[col][row], row = xn(k) * Tcw.row(2) - Tcw.row(k) (:352-355)
#pragma unroll
            for (int col = 0; col < 4; ++col) {
                const float a2 = col < 3 ? J.R1[6 + col] : J.t1[2], a0 = col < 3 ? J.R1[col] : J.t1[0], a1 = col < 3 ? J.R1[3 + col] : J.t1[1];
                const float b2 = col < 3 ? J.R2[6 + col] : J.t2[2], b0 = col < 3 ? J.R2[col] : J.t2[0], b1 = col < 3 ? J.R2[3 + col] : J.t2[1];
                At[col][0] = xn1x * a2 - a0;
                At[col][1] = xn1y * a2 - a1;
                At[col][2] = xn2x * b2 - b0;
                At[col][3] = xn2y * b2 - b1;
            }
            tri_null_vector(At, v);
            if (v[3] == 0) {
                status = TS_W_ZERO;
                have = false;
            } else {
                X = v[0] / v[3]; Y = v[1] / v[3]; Z = v[2] / v[3];
            }
        } else if (st1 && cs1 < cs2) {
            route = TR_UNPROJECT_A;
            const float z = J.depth1[i];
            if (z > 0) {
                const float x = ((J.xd1[i] - J.cx1) * z) * J.invfx1, y = ((J.yd1[i] - J.cy1) * z) * J.invfy1;
                X = tri_sum3(J.R1[0] * x, J.R1[3] * y, J.R1[6] * z) + J.O1[0];
                Y = tri_sum3(J.R1[1] * x, J.R1[4] * y, J.R1[7] * z) + J.O1[1];
                Z = tri_sum3(J.R1[2] * x, J.R1[5] * y, J.R1[8] * z) + J.O1[2];
            } else {
                X = 0.0f; Y = 0.0f; Z = -1.0f;
            }
        } else if (st2 && cs2 < cs1) {
            route = TR_UNPROJECT_B;
            const float z = J.depth2[j];
            if (z > 0) {
                const float x = ((J.xd2[j] - J.cx2) * z) * J.invfx2, y = ((J.yd2[j] - J.cy2) * z) * J.invfy2;
                X = tri_sum3(J.R2[0] * x, J.R2[3] * y, J.R2[6] * z) + J.O2[0];
                Y = tri_sum3(J.R2[1] * x, J.R2[4] * y, J.R2[7] * z) + J.O2[1];
                Z = tri_sum3(J.R2[2] * x, J.R2[5] * y, J.R2[8] * z) + J.O2[2];
            } else {
                X = 0.0f; Y = 0.0f; Z = -1.0f;
            }
        } else {
            status = TS_LOW_PARALLAX;  // no stereo and very low parallax (:381)
            have = false;
        }
        if (have) {
            status = TS_ACCEPTED;
            float n1[3], n2[3];
            const float z1 = tri_cam(J.R1, J.t1, 2, X, Y, Z), z2 = tri_cam(J.R2, J.t2, 2, X, Y, Z);
            if (!(__builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z))) status = TS_NOT_FINITE;  // T3
            else if (z1 <= 0) status = TS_Z1;
            else if (z2 <= 0) status = TS_Z2;
            else if (tri_reproj_fails(J.fx1, J.fy1, J.cx1, J.cy1, J.mbf1, tri_cam(J.R1, J.t1, 0, X, Y, Z), tri_cam(J.R1, J.t1, 1, X, Y, Z), 1.0f / z1, kx1,
                                      ky1, ur1, st1, J.sigma2_1[i]))
                status = TS_REPROJ1;
            else if (tri_reproj_fails(J.fx2, J.fy2, J.cx2, J.cy2, J.mbf1 /* Q1 */, tri_cam(J.R2, J.t2, 0, X, Y, Z), tri_cam(J.R2, J.t2, 1, X, Y, Z),
                                      1.0f / z2, kx2, ky2, ur2, st2, J.sigma2_2[j]))
                status = TS_REPROJ2;
            else {
                const float d1 = tri_dist(X, Y, Z, J.O1, n1), d2 = tri_dist(X, Y, Z, J.O2, n2);
                if (d1 == 0 || d2 == 0) {
                    status = TS_ZERO_DIST;
                } else {
                    const float ratio_dist = d2 / d1, ratio_octave = J.size1[i] / J.size2[j];
                    if (ratio_dist * J.ratio_factor < ratio_octave || ratio_dist > ratio_octave * J.ratio_factor) status = TS_RATIO;
                }
            }
        }
    }
    return status;
}

// what the store holds for the accepted match of feature i with x3D = (X, Y, Z) under the new id (MapPoint::MapPoint + UpdateNormalAndDepth)
__device__ __forceinline__ void tri_store_point(const DevPointPlanes &P, const DevTriPair &J, int i, int id, float X, float Y, float Z) {
    float n1[3], n2[3];
    const float d1 = tri_dist(X, Y, Z, J.O1, n1), d2 = tri_dist(X, Y, Z, J.O2, n2);
    const float size = J.size1[i], max_d = d1 * size;
    P.pos[0][id] = X; P.pos[1][id] = Y; P.pos[2][id] = Z;
#pragma unroll
    for (int k = 0; k < 3; ++k) P.normal[k][id] = ((0.0f + n1[k] / d1) + n2[k] / d2) / 2.0f;  // MapPoint.cc:390-397, :416
    P.ref_dist[id] = d1;
    P.ref_size[id] = size;
    P.ref_sigma[id] = sqrtf(J.sigma2_1[i]);
    P.max_d[id] = max_d;
    P.min_d[id] = max_d / J.max_size1;
    P.flags[id] = (uint8_t)(AFV_PTF_SET | AFV_PTF_OBSERVED);
}

// the rows of a workgroup's new points, a thread per 16 bytes: row (first + l) of keyframe a for the id s_id[l] (-1: none)
// (afv_distinctive_descriptors recomputes it later)
__device__ __forceinline__ void tri_store_rows(const DevPointPlanes &P, const DevTriPair &J, const int *s_id, int first, int tid) {
    const int quads = P.words >> 2;
    for (int t = tid; t < TRI_T * quads; t += TRI_T) {
        const int l = t / quads, h = t - l * quads, d = s_id[l];
        if (d < 0) continue;
        const int f = first + l;
        reinterpret_cast<uint4 *>(P.desc + (size_t)d * P.words * 4)[h] = reinterpret_cast<const uint4 *>(J.rows1 + (size_t)f * P.words * 4)[h];
    }
}
