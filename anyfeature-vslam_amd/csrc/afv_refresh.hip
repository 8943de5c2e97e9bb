// afv_refresh.hip — host side of afv_table_refresh_points (include/afv_hip.h, "Refresh of resident map points"; kernels: k_refresh.hip).
//
// Reference call shape: MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth run on the host, point by point, after
// every bundle adjustment (Optimizer.cc:234, :766, :1029), at the end of LocalMapping::SearchInNeighbors (LocalMapping.cc:547-548), in
// LoopClosing::CorrectLoop (:515) and on every change of a point's observations (MapPoint.cc:120, :172, :249).  Here the observation
// lists go up in one copy - the arrays the caller has just given to afv_table_bundle_adjust - and one launch per part reads the rows,
// sizes and sigmas from the table and the positions from the store, and writes the store in place.
#include "afv_runtime.h"

#include <climits>

static_assert(sizeof(afv_refresh_params) == 12 && sizeof(afv_refresh_out) == 32, "afv_refresh records");

namespace {

struct RefreshCall {
    afv_table *t;
    afv_points *points;
    const int32_t *slots, *point_ids, *ref_kf, *obs_point, *obs_kf, *obs_idx;
    const float *centres, *max_size;
    const uint8_t *kf_bad;
    int nk, np, ne;
    afv_refresh_params prm;
};

int refresh_refuse(afv_ctx *c, const char *why, int rc = AFV_EINVAL) {
    c->last_error = std::string("afv_table_refresh_points: ") + why;
    return rc;
}

// everything that is malformed is refused here, before any launch; builds pt_ptr [np + 1].  (With at most AFV_LBA_MAX_KF keyframes and no
// keyframe observing a point twice, a point cannot reach 65536 observations: that bound is the kernel's precondition, restated last.)
int refresh_check(const RefreshCall &K, std::vector<int> &pt_ptr) {
    const afv_table *t = K.t;
    const afv_points *s = K.points;
    afv_ctx *c = t->c;
    if (t->float_dim != s->float_dim || t->desc_bytes != s->desc_bytes || t->words != s->words)
        return refresh_refuse(c, "the store's rows are of another kind or width than the table's", AFV_EUNSUPPORTED);
    if ((size_t)t->nsets * (size_t)t->cap > (size_t)INT_MAX) return refresh_refuse(c, "the table is too large", AFV_EUNSUPPORTED);
    for (int k = 0; k < K.nk; ++k) {
        const int sl = K.slots[k];
        if (sl < 0 || sl >= t->nsets) return refresh_refuse(c, "a slot is out of range");
        if (t->h_n[sl] > 0 && !t->has_geo[sl]) return refresh_refuse(c, "a slot lacks its geometry (afv_table_set_geometry)");
        if (K.prm.normals && t->h_n[sl] > 0 && !t->has_scale[sl]) return refresh_refuse(c, "a slot lacks its scale plane (afv_table_set_scale)");
    }
    {
        // one byte per id of the STORE, zeroed per call, as the bundle adjustment's check does: with a store that holds a whole map this is
        // part of the call's fixed cost (4 MB at the largest capacity); a list of the named ids, sorted, would cost O(np log np) instead
        std::vector<uint8_t> seen((size_t)s->cap, 0);
        for (int p = 0; p < K.np; ++p) {
            const int id = K.point_ids[p];
            if (id < 0 || id >= s->cap) return refresh_refuse(c, "a map-point id lies outside the store");
            if (seen[(size_t)id]) return refresh_refuse(c, "a map-point id is named twice");
            seen[(size_t)id] = 1;
            if (K.ref_kf[p] < -1 || K.ref_kf[p] >= K.nk) return refresh_refuse(c, "ref_kf is out of range");
        }
    }
    pt_ptr.assign((size_t)K.np + 1, 0);
    std::vector<int> last((size_t)std::max(K.nk, 1), -1);  // the last point that keyframe k observed: a repeat is a duplicate
    for (int e = 0; e < K.ne; ++e) {
        const int p = K.obs_point[e], k = K.obs_kf[e];
        if (p < 0 || p >= K.np) return refresh_refuse(c, "obs_point is out of range");
        if (e > 0 && p < K.obs_point[e - 1]) return refresh_refuse(c, "the observations are not grouped by point");
        if (k < 0 || k >= K.nk) return refresh_refuse(c, "obs_kf is out of range");
        if (K.obs_idx[e] < 0 || K.obs_idx[e] >= t->h_n[K.slots[k]]) return refresh_refuse(c, "obs_idx names a feature that does not exist");
        if (last[(size_t)k] == p) return refresh_refuse(c, "a point is observed twice by one keyframe");
        last[(size_t)k] = p;
        pt_ptr[(size_t)p + 1] = e + 1;
    }
    for (int p = 0; p < K.np; ++p) {
        if (pt_ptr[(size_t)p + 1] < pt_ptr[(size_t)p]) pt_ptr[(size_t)p + 1] = pt_ptr[(size_t)p];  // a point without observations
        if (pt_ptr[(size_t)p + 1] - pt_ptr[(size_t)p] > 65535) return refresh_refuse(c, "more than 65535 observations of one point");
    }
    return AFV_OK;
}

int refresh_impl(const RefreshCall &K, const afv_refresh_out &out) {
    afv_table *t = K.t;
    afv_ctx *c = t->c;
    std::vector<int> pt_ptr;
    const int rc0 = refresh_check(K, pt_ptr);
    if (rc0) return rc0;
    const int nk = K.nk, np = K.np, ne = K.ne;
    if (np == 0) return AFV_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t E = (size_t)std::max(ne, 1), P = (size_t)np, KF = (size_t)std::max(nk, 1);
    // the image: inputs first (one upload), then what the host reads back, then device-only scratch
    Blob b(c);
    const size_t o_slots = b.put(K.slots, KF * 4 * (nk > 0)), o_cen = b.put(K.centres, KF * 12 * (nk > 0)), o_max = b.put(K.max_size, KF * 4 * (nk > 0));
    const size_t o_bad = K.kf_bad ? b.put(K.kf_bad, KF * (nk > 0)) : b.reserve(KF);
    const size_t o_ids = b.put(K.point_ids, P * 4), o_ref = b.put(K.ref_kf, P * 4), o_ptp = b.put(pt_ptr.data(), pt_ptr.size() * 4);
    const size_t o_ekf = b.put(K.obs_kf, E * 4 * (ne > 0)), o_eidx = b.put(K.obs_idx, E * 4 * (ne > 0));
    const size_t in_bytes = b.h.size();
    const size_t o_status = b.reserve_scratch(P * 4), o_best = b.reserve_scratch(P * 4), o_med = b.reserve_scratch(P * 4);
    const size_t o_crow = b.reserve_scratch(E * 4), o_cobs = b.reserve_scratch(E * 4);
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    uint8_t *B = c->d_match;
    HIPCHK(c, b.upload(in_bytes));
    const size_t plane = (size_t)t->nsets * t->cap;
    DevRefresh A{};
    A.P = K.points->P;
    A.desc = t->d_desc;
    A.sigma2 = t->d_geo + 2 * plane;
    A.size = t->d_scale;  // plane 0: keyPtsSize (null without normals on a table that never had a scale plane: not read)
    A.cap = t->cap; A.desc_bytes = t->desc_bytes; A.float_dim = t->float_dim;
    A.slots = reinterpret_cast<const int *>(B + o_slots);
    A.centres = reinterpret_cast<const float *>(B + o_cen); A.max_size = reinterpret_cast<const float *>(B + o_max);
    A.kf_bad = B + o_bad;
    A.point_ids = reinterpret_cast<const int *>(B + o_ids); A.ref_kf = reinterpret_cast<const int *>(B + o_ref);
    A.pt_ptr = reinterpret_cast<const int *>(B + o_ptp);
    A.obs_kf = reinterpret_cast<const int *>(B + o_ekf); A.obs_idx = reinterpret_cast<const int *>(B + o_eidx);
    A.np = np;
    A.c_row = reinterpret_cast<int *>(B + o_crow); A.c_obs = reinterpret_cast<int *>(B + o_cobs);
    A.status = reinterpret_cast<int *>(B + o_status); A.best_obs = reinterpret_cast<int *>(B + o_best); A.best_median = reinterpret_cast<int *>(B + o_med);
    A.desc_writes_status = K.prm.normals ? 0 : 1;
    if (K.prm.descriptors) afv_launch_refresh_desc(&A, c->stream);
    else {  // R3: nothing was chosen
        HIPCHK(c, hipMemsetAsync(B + o_best, 0xff, P * 4, c->stream));
        HIPCHK(c, hipMemsetAsync(B + o_med, 0, P * 4, c->stream));
    }
    if (K.prm.normals) afv_launch_refresh_normals(&A, c->stream);
    else if (!K.prm.descriptors) HIPCHK(c, hipMemsetAsync(B + o_status, 0, P * 4, c->stream));
    HIPCHK(c, hipGetLastError());
    if (out.status) HIPCHK(c, b.fetch(out.status, o_status, P * 4, c->stream));
    if (out.best_obs) HIPCHK(c, b.fetch(out.best_obs, o_best, P * 4, c->stream));
    if (out.best_median) HIPCHK(c, b.fetch(out.best_median, o_med, P * 4, c->stream));
    HIPCHK(c, b.wait());
    return AFV_OK;
}

}  // namespace

extern "C" int afv_table_refresh_points(afv_table *t, afv_points *points, const int32_t *slots, int nk, const float *centres, const float *max_size,
                                        const uint8_t *kf_bad, const int32_t *point_ids, int np, const int32_t *ref_kf, const int32_t *obs_point,
                                        const int32_t *obs_kf, const int32_t *obs_idx, int ne, const afv_refresh_params *params, afv_refresh_out *out) {
    if (!t || !points || !slots || !centres || !max_size || !point_ids || !ref_kf || !obs_point || !obs_kf || !obs_idx || !params || !out) return AFV_EINVAL;
    if (nk < 0 || nk > AFV_LBA_MAX_KF || np < 0 || np > AFV_LBA_MAX_POINTS || ne < 0 || ne > AFV_LBA_MAX_EDGES) return AFV_EINVAL;
    if (!afv_points_is_live(points) || points->c != t->c) return AFV_EINVAL;
    return guarded(t->c, [&] {
        RefreshCall K{};
        K.t = t; K.points = points; K.slots = slots; K.centres = centres; K.max_size = max_size; K.kf_bad = kf_bad; K.point_ids = point_ids;
        K.ref_kf = ref_kf; K.obs_point = obs_point; K.obs_kf = obs_kf; K.obs_idx = obs_idx;
        K.nk = nk; K.np = np; K.ne = ne;
        std::vector<afv_refresh_params> prm;
        std::vector<afv_refresh_out> o;
        if (!afv_load_jobs(params, 1, sizeof(afv_refresh_params), prm) || !afv_load_jobs(out, 1, sizeof(afv_refresh_out), o)) return (int)AFV_EINVAL;
        K.prm = prm[0];
        if ((K.prm.descriptors != 0 && K.prm.descriptors != 1) || (K.prm.normals != 0 && K.prm.normals != 1)) return (int)AFV_EINVAL;
        return refresh_impl(K, o[0]);
    });
}
