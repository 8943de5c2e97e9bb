// kffuse_host — the projection loop of FeatureMatcher::Fuse (FeatureMatcher.cc:811-858) as scalar host code: what a caller WITHOUT
// afv_table_fuse_points runs per target keyframe before it hands the queries to afv_match_fuse as host arrays.  tools/time_kffuse.py times
// the device route against it and compares the answers in the same run.  The arithmetic is the restatement's (tests/_points_ref.py, FUSE):
// float, one rounding per operator (build with -ffp-contract=off), three-term sums as a0 + (a1 + a2); D1 (a non-finite query is not in view).
#include <cmath>
#include <cstdint>
#include <unordered_set>

namespace {
inline float sum3(float a0, float a1, float a2) { return a0 + (a1 + a2); }
}  // namespace

struct kffuse_host_store {  // the host's map points, SoA over `capacity` ids
    const float *pos, *normal;          // [capacity][3]
    const float *min_d, *max_d, *ref_size, *ref_dist;
    const uint8_t *flags;               // 1 set | 2 bad
    int32_t capacity;
};
struct kffuse_host_camera {
    float R[9], t[3], Ow[3], fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y, rs_th, tol;
};

// status[q]: 0 invalid, 1 already in the keyframe, 2 not in view, 255 goes into the search; the query arrays are 0 unless 255
extern "C" void kffuse_host_project(const kffuse_host_store *S, const kffuse_host_camera *C, const int32_t *ids, int nq, const int32_t *plane, int n,
                                    float *qu, float *qv, float *qr, float *qmin, float *qmax, float *q_ur, uint8_t *qvalid, uint8_t *status) {
    std::unordered_set<int32_t> held;
    for (int i = 0; i < n; ++i)
        if (plane[i] >= 0) held.insert(plane[i]);
    for (int q = 0; q < nq; ++q) {
        qu[q] = qv[q] = qr[q] = qmin[q] = qmax[q] = q_ur[q] = 0.0f;
        qvalid[q] = 0;
        const int32_t id = ids[q];
        if (id < 0 || id >= S->capacity || !(S->flags[id] & 1) || (S->flags[id] & 2)) { status[q] = 0; continue; }
        if (held.count(id)) { status[q] = 1; continue; }
        status[q] = 2;
        const float X = S->pos[3 * id], Y = S->pos[3 * id + 1], Z = S->pos[3 * id + 2];
        const float pcx = sum3(C->R[0] * X, C->R[1] * Y, C->R[2] * Z) + C->t[0];
        const float pcy = sum3(C->R[3] * X, C->R[4] * Y, C->R[5] * Z) + C->t[1];
        const float pcz = sum3(C->R[6] * X, C->R[7] * Y, C->R[8] * Z) + C->t[2];
        if (pcz < 0.0f) continue;
        const float invz = 1.0f / pcz;
        const float x = pcx * invz, y = pcy * invz;
        const float u = C->fx * x + C->cx, v = C->fy * y + C->cy;
        if (!(u >= C->min_x && u < C->max_x && v >= C->min_y && v < C->max_y)) continue;
        const float ur = u - C->mbf * invz;
        const float p0 = X - C->Ow[0], p1 = Y - C->Ow[1], p2 = Z - C->Ow[2];
        const float dist = std::sqrt(sum3(p0 * p0, p1 * p1, p2 * p2));
        if (dist < 0.8f * S->min_d[id] || dist > 1.2f * S->max_d[id]) continue;
        const float dot = sum3(p0 * S->normal[3 * id], p1 * S->normal[3 * id + 1], p2 * S->normal[3 * id + 2]);
        if (dot < 0.5f * dist) continue;
        const float size = (S->ref_size[id] * S->ref_dist[id]) / dist;
        const float r = C->rs_th * size, mn = size / C->tol, mx = size * C->tol;
        if (!(std::isfinite(u) && std::isfinite(v) && std::isfinite(r) && std::isfinite(mn) && std::isfinite(mx))) continue;
        qu[q] = u; qv[q] = v; qr[q] = r; qmin[q] = mn; qmax[q] = mx; q_ur[q] = ur;
        qvalid[q] = 1;
        status[q] = 255;
    }
}
