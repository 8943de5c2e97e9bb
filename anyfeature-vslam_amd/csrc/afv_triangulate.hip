// afv_triangulate.hip — host side of afv_table_triangulate (include/afv_hip.h, "new map points"; kernels: k_triangulate.hip).
//
// Reference call shape: LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:265-472) triangulates the matches of SearchForTriangulation
// one by one on the host and creates a MapPoint per accepted match.  Here the matches of up to 64 (a, b) pairs of table slots go up as
// match12 rows, two launches run on the context's stream and the host waits once: k_tri_points judges every match, k_tri_store ranks the
// accepted ones and writes the new points into the resident store.
#include "afv_runtime.h"

AFV_LOCAL int tri_check_slot(const afv_table *t, int s) {
    if (t->h_n[s] > 0 && (!t->has_geo[s] || !t->has_scale[s])) {
        t->c->last_error = "afv_table_triangulate: set " + std::to_string(s) + " lacks its geometry (afv_table_set_geometry) or its scale planes (afv_table_set_scale)";
        return AFV_EINVAL;
    }
    return AFV_OK;
}

static void tri_side(const afv_table *t, int slot, const float **geo4, const float **scale4) {
    const size_t row0 = (size_t)slot * t->cap, plane = (size_t)t->nsets * t->cap;
    for (int k = 0; k < 4; ++k) {
        geo4[k] = t->d_geo + k * plane + row0;
        scale4[k] = t->d_scale + k * plane + row0;
    }
}

// the device record of one (a, b) pair: the caller's job and where the planes of the two slots start
AFV_LOCAL void tri_fill_pair(const afv_table *t, int a, int b, const afv_tri_points_job &j, DevTriPair &D) {
    const int cap = t->cap;
    D = DevTriPair{};
    std::memcpy(D.R1, j.Rcw1, sizeof(D.R1)); std::memcpy(D.t1, j.tcw1, sizeof(D.t1)); std::memcpy(D.O1, j.Ow1, sizeof(D.O1));
    std::memcpy(D.R2, j.Rcw2, sizeof(D.R2)); std::memcpy(D.t2, j.tcw2, sizeof(D.t2)); std::memcpy(D.O2, j.Ow2, sizeof(D.O2));
    D.fx1 = j.fx1; D.fy1 = j.fy1; D.cx1 = j.cx1; D.cy1 = j.cy1; D.invfx1 = j.invfx1; D.invfy1 = j.invfy1;
    D.fx2 = j.fx2; D.fy2 = j.fy2; D.cx2 = j.cx2; D.cy2 = j.cy2; D.invfx2 = j.invfx2; D.invfy2 = j.invfy2;
    D.mb1 = j.mb1; D.mb2 = j.mb2; D.mbf1 = j.mbf1; D.ratio_factor = j.ratio_factor; D.max_size1 = j.max_size1;
    D.n1 = t->h_n[a]; D.n2 = t->h_n[b];
    if (t->d_geo && t->d_scale) {
        const float *g[4], *s[4];
        tri_side(t, a, g, s);
        D.x1 = g[0]; D.y1 = g[1]; D.sigma2_1 = g[2]; D.ur1 = g[3]; D.size1 = s[0]; D.depth1 = s[1]; D.xd1 = s[2]; D.yd1 = s[3];
        tri_side(t, b, g, s);
        D.x2 = g[0]; D.y2 = g[1]; D.sigma2_2 = g[2]; D.ur2 = g[3]; D.size2 = s[0]; D.depth2 = s[1]; D.xd2 = s[2]; D.yd2 = s[3];
    } else {
        D.n1 = D.n2 = 0;
    }
    D.rows1 = t->d_desc + (size_t)a * cap * t->words * 4;
}

static int triangulate_impl(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, const afv_tri_points_job *caller_jobs, int npairs,
                            const int32_t *match12, afv_points *points, int32_t first_id, uint8_t *status, uint8_t *route, float *x3d,
                            int32_t *new_id, int32_t *n_new) {
    afv_ctx *c = t->c;
    std::vector<afv_tri_points_job> jobs;
    if (!afv_load_jobs(caller_jobs, npairs, sizeof(afv_tri_points_job), jobs)) return AFV_EINVAL;
    const int cap = t->cap;
    for (int p = 0; p < npairs; ++p) {
        const int a = pair_a[p], b = pair_b[p];
        if (a < 0 || a >= t->nsets || b < 0 || b >= t->nsets) return AFV_EINVAL;
        if (tri_check_slot(t, a) || tri_check_slot(t, b)) return AFV_EINVAL;
        const int n1 = t->h_n[a], n2 = t->h_n[b];
        const int32_t *row = match12 + (size_t)p * cap;
        for (int i = 0; i < cap; ++i)
            if (row[i] < -1 || row[i] >= n2 || (row[i] >= 0 && i >= n1)) {
                c->last_error = "afv_table_triangulate: match12 of pair " + std::to_string(p) + " names a feature that does not exist";
                return AFV_EINVAL;
            }
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int nblk = (cap + AFV_TRI_T - 1) / AFV_TRI_T;
    const size_t cells = (size_t)npairs * cap;
    std::vector<DevTriPair> dp((size_t)npairs);
    for (int p = 0; p < npairs; ++p) {
        tri_fill_pair(t, pair_a[p], pair_b[p], jobs[(size_t)p], dp[(size_t)p]);
    }
    Blob b(c);
    const size_t o_pairs = b.put(dp.data(), dp.size() * sizeof(DevTriPair));
    const size_t o_match = b.put(match12, cells * 4);
    const size_t in_bytes = b.h.size();
    const size_t o_status = b.reserve_scratch(cells), o_route = b.reserve_scratch(cells), o_x3d = b.reserve_scratch(cells * 12);
    const size_t o_id = b.reserve_scratch(cells * 4), o_nnew = b.reserve_scratch((size_t)npairs * 4), o_blk = b.reserve_scratch((size_t)npairs * nblk * 4);
    const size_t o_total = b.reserve_scratch(16);
    const int rc = ensure_match_buffer(c, b.h.size());
    if (rc) return rc;
    uint8_t *B = c->d_match;
    HIPCHK(c, b.upload(in_bytes));
    DevTriArgs A{};
    A.pairs = reinterpret_cast<const DevTriPair *>(B + o_pairs);
    A.match12 = reinterpret_cast<const int *>(B + o_match);
    A.npairs = npairs; A.cap = cap; A.nblk = nblk;
    A.status = B + o_status; A.route = B + o_route;
    A.x3d = reinterpret_cast<float *>(B + o_x3d);
    A.blk_count = reinterpret_cast<int *>(B + o_blk);
    A.new_id = reinterpret_cast<int *>(B + o_id);
    A.n_new = reinterpret_cast<int *>(B + o_nnew);
    A.total = reinterpret_cast<int *>(B + o_total);
    if (points) A.P = points->P;
    A.has_points = points ? 1 : 0;
    A.first_id = first_id;
    afv_launch_tri_points(&A, c->stream);
    afv_launch_tri_store(&A, c->stream);
    HIPCHK(c, hipGetLastError());
    int32_t total = 0;
    if (status) HIPCHK(c, b.fetch(status, o_status, cells, c->stream));
    if (route) HIPCHK(c, b.fetch(route, o_route, cells, c->stream));
    if (x3d) HIPCHK(c, b.fetch(x3d, o_x3d, cells * 12, c->stream));
    if (new_id) HIPCHK(c, b.fetch(new_id, o_id, cells * 4, c->stream));
    if (n_new) HIPCHK(c, b.fetch(n_new, o_nnew, (size_t)npairs * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.h.data() + o_total, B + o_total, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the call's one wait
    std::memcpy(&total, b.h.data() + o_total, 4);
    if (points && (long long)first_id + total > (long long)points->cap) {
        b.pending.clear();  // the caller's arrays stay as they are
        c->last_error = "afv_table_triangulate: " + std::to_string(total) + " new points from id " + std::to_string(first_id) + " exceed the store's capacity " +
                        std::to_string(points->cap) + "; the store is untouched";
        return AFV_ECAPACITY;
    }
    b.finish();
    return AFV_OK;
}

extern "C" int afv_table_triangulate(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, const afv_tri_points_job *jobs, int npairs,
                                     const int32_t *match12, afv_points *points, int32_t first_id, uint8_t *status, uint8_t *route, float *x3d,
                                     int32_t *new_id, int32_t *n_new) {
    if (!t || !pair_a || !pair_b || !jobs || !match12 || npairs < 1 || npairs > AFV_TRI_MAX_PAIRS || first_id < 0) return AFV_EINVAL;
    if (points) {
        if (!afv_points_is_live(points) || points->c != t->c) return AFV_EINVAL;
        if (points->float_dim != t->float_dim || points->desc_bytes != t->desc_bytes || points->words != t->words) return AFV_EUNSUPPORTED;
        if (first_id > points->cap) return AFV_ECAPACITY;
    }
    return guarded(t->c, [&] { return triangulate_impl(t, pair_a, pair_b, jobs, npairs, match12, points, first_id, status, route, x3d, new_id, n_new); });
}
