// points_host_loop — the loop an integrator runs on the host in front of SearchByProjection(F, vpMapPoints, th) when the map points are
// not resident: Frame::isInFrustum (Frame.cc:276-331) and the radius / size band / stereo gate of FeatureMatcher.cc:90-95, :116-117 per
// point, filling the query arrays of afv_proj_queries.  Compiled by tools/time_points.py (g++ -O2 -ffp-contract=off) as the C++ host
// baseline next to its numpy form; the statements and their order are the device kernel's (k_points_project), so the answers agree.
#include <cmath>
#include <cstdint>

struct HostPoint {  // what the loop reads from a MapPoint
    float pos[3], normal[3], min_d, max_d, ref_size, ref_dist, ref_sigma;
};

extern "C" int points_host_loop(const HostPoint *pts, int n, const float *Rcw, const float *tcw, const float *Ow, float fx, float fy, float cx,
                                float cy, float mbf, float min_x, float max_x, float min_y, float max_y, float rs_th, float cos_limit, float tol,
                                uint8_t *valid, float *qu, float *qv, float *qr, float *qmin, float *qmax, float *q_ur, float *q_er) {
    int in_view = 0;
    for (int i = 0; i < n; ++i) {
        const HostPoint &p = pts[i];
        const float X = p.pos[0], Y = p.pos[1], Z = p.pos[2];
        const float pcx = Rcw[0] * X + (Rcw[1] * Y + Rcw[2] * Z) + tcw[0];
        const float pcy = Rcw[3] * X + (Rcw[4] * Y + Rcw[5] * Z) + tcw[1];
        const float pcz = Rcw[6] * X + (Rcw[7] * Y + Rcw[8] * Z) + tcw[2];
        bool ok = !(pcz < 0.0f);
        const float invz = 1.0f / pcz;
        const float u = (fx * pcx) * invz + cx, v = (fy * pcy) * invz + cy;
        if (u < min_x || u > max_x || v < min_y || v > max_y) ok = false;
        const float p0 = X - Ow[0], p1 = Y - Ow[1], p2 = Z - Ow[2];
        const float dist = std::sqrt(p0 * p0 + (p1 * p1 + p2 * p2));
        if (dist < 0.8f * p.min_d || dist > 1.2f * p.max_d) ok = false;
        const float vcos = (p0 * p.normal[0] + (p1 * p.normal[1] + p2 * p.normal[2])) / dist;
        if (vcos < cos_limit) ok = false;
        const float size = (p.ref_size * p.ref_dist) / dist, sigma = (p.ref_sigma * p.ref_dist) / dist;
        const float r = (rs_th * ((double)vcos > 0.998 ? 2.5f : 4.0f)) * size;
        const float mn = size / tol, mx = size * tol;
        if (!(std::isfinite(u) && std::isfinite(v) && std::isfinite(r) && std::isfinite(mn) && std::isfinite(mx))) ok = false;
        valid[i] = ok;
        qu[i] = ok ? u : 0.0f; qv[i] = ok ? v : 0.0f; qr[i] = ok ? r : 0.0f; qmin[i] = ok ? mn : 0.0f; qmax[i] = ok ? mx : 0.0f;
        q_ur[i] = ok ? u - mbf * invz : 0.0f; q_er[i] = ok ? r * sigma : 0.0f;
        in_view += ok;
    }
    return in_view;
}
