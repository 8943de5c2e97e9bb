// afv_newpoints.hip — host side of afv_table_create_new_points (include/afv_hip.h, "new map points"; kernels: k_newpoints.hip).
//
// Reference call shape: LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:265-472) walks the neighbours of the current keyframe one
// after the other: SearchForTriangulation, the judgement of its matches, a MapPoint per accepted match - and a feature that received a
// point is skipped by the searches of the later neighbours.  Here everything that does not depend on an earlier neighbour is staged for
// all of them at once (the FeatureVector joins, the feature -> shared node maps, the pair records, the masks, the first free id) and goes
// up in ONE copy; two launches per neighbour follow on the context's stream, whose order carries the mask of the current keyframe and the
// next free id from neighbour to neighbour; the host waits once.
#include "afv_runtime.h"

static const char *const WHO = "afv_table_create_new_points";

static int create_new_points_impl(afv_table *t, int32_t cur, const int32_t *neighbours, int nn, const afv_table_tri_job *caller_search,
                                  const afv_tri_points_job *caller_jobs, uint8_t *has_mp_cur, uint8_t *has_mp_nb, afv_points *points,
                                  int32_t first_id, int32_t *match12, uint8_t *status, uint8_t *route, float *x3d, int32_t *new_id,
                                  int32_t *n_new, int32_t *n_done) {
    afv_ctx *c = t->c;
    std::vector<afv_table_tri_job> geo;
    std::vector<afv_tri_points_job> jobs;
    if (!afv_load_jobs(caller_search, nn, offsetof(afv_table_tri_job, only_stereo), geo)) return AFV_EINVAL;
    if (!afv_load_jobs(caller_jobs, nn, sizeof(afv_tri_points_job), jobs)) return AFV_EINVAL;
    if (cur < 0 || cur >= t->nsets) return AFV_EINVAL;
    for (int k = 0; k < nn; ++k) {
        const int nb = neighbours[k];
        if (nb < 0 || nb >= t->nsets || nb == cur) return AFV_EINVAL;
        for (int l = 0; l < k; ++l)
            if (neighbours[l] == nb) {
                c->last_error = std::string(WHO) + ": set " + std::to_string(nb) + " is listed twice";
                return AFV_EINVAL;
            }
        if (geo[k].only_stereo != 0 && geo[k].only_stereo != 1) return AFV_EINVAL;
        if (geo[k].has_mp1 || geo[k].has_mp2) {
            c->last_error = std::string(WHO) + ": the masks travel as has_mp_cur / has_mp_nb; has_mp1 / has_mp2 of a search record must be NULL";
            return AFV_EINVAL;
        }
    }
    if (!t->d_idx || !t->d_geo) return AFV_EINVAL;  // no FeatureVector / no geometry was ever stored
    for (int k = -1; k < nn; ++k) {
        const int s = k < 0 ? cur : neighbours[k];
        if (check_slot_ready(t, s, true, WHO) || tri_check_slot(t, s)) return AFV_EINVAL;
    }
    const int cap = t->cap;
    const size_t cells = (size_t)nn * cap;
    // rows of the neighbours that did nothing (the capacity rule): no match, no point
    auto empty_rows = [&](int from) {
        const size_t o = (size_t)from * cap, n = cells - o;
        if (match12) std::fill(match12 + o, match12 + cells, -1);
        if (status) std::memset(status + o, 0, n);
        if (route) std::memset(route + o, 0, n);
        if (x3d) std::fill(x3d + 3 * o, x3d + 3 * cells, 0.0f);
        if (new_id) std::fill(new_id + o, new_id + cells, -1);
        std::fill(n_new + from, n_new + nn, 0);
    };
    if (points && first_id > points->cap) {  // (the first afv_table_triangulate of the loop answers the same)
        empty_rows(0);
        *n_done = 0;
        return AFV_ECAPACITY;
    }
    {
        const int rc = table_fetch_fv_body(t, cur);  // the row maps read the body of the current keyframe on the host
        if (rc) return rc;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int nblk = (cap + AFV_TRI_T - 1) / AFV_TRI_T;
    const MatchSide s1 = table_side(t, cur);
    std::vector<Seg> segs;
    std::vector<int> seg_first((size_t)nn + 1, 0), row_seg;
    std::vector<size_t> rowseg_off((size_t)nn, 0);
    std::vector<DevTriPair> dp((size_t)nn);
    Blob b(c);
    for (int k = 0; k < nn; ++k) {
        const MatchSide s2 = table_side(t, neighbours[k]);
        const int first = seg_first[(size_t)k];
        join_featvecs(s1, s2, false, segs);
        const int nseg = (int)segs.size() - first;
        seg_first[(size_t)k + 1] = first + nseg;
        const int rc = build_row_seg(s1, segs.data() + first, nseg, row_seg);
        if (rc) return rc;
        rowseg_off[(size_t)k] = b.put(row_seg.data(), row_seg.size() * sizeof(int));
        tri_fill_pair(t, cur, neighbours[k], jobs[(size_t)k], dp[(size_t)k]);
    }
    const size_t o_segs = b.put(segs.data(), segs.size() * sizeof(Seg));
    const size_t o_pairs = b.put(dp.data(), dp.size() * sizeof(DevTriPair));
    const size_t o_search = b.reserve((size_t)nn * sizeof(DevTriJob));
    const size_t o_cur = b.put(has_mp_cur, (size_t)cap), o_nb = b.put(has_mp_nb, cells);
    const size_t o_next = b.reserve(((size_t)nn + 1) * 4), o_stop = b.reserve(((size_t)nn + 1) * 4);  // stop[0] = 0
    std::memcpy(b.h.data() + o_next, &first_id, 4);
    const size_t in_bytes = b.h.size();
    const size_t o_match = b.reserve_scratch(cells * 4), o_status = b.reserve_scratch(cells), o_route = b.reserve_scratch(cells);
    const size_t o_x3d = b.reserve_scratch(cells * 12), o_id = b.reserve_scratch(cells * 4), o_nnew = b.reserve_scratch((size_t)nn * 4);
    const size_t o_blk = b.reserve_scratch((size_t)nn * nblk * 4);
    {
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
    }
    uint8_t *B = c->d_match;
    for (int k = 0; k < nn; ++k) {  // the search records: every pointer names the table or the blob on the device
        const MatchSide s2 = table_side(t, neighbours[k]);
        DevTriJob &T = reinterpret_cast<DevTriJob *>(b.h.data() + o_search)[k];
        DevMatchJob &d = T.m;
        d.d1 = reinterpret_cast<const uint32_t *>(s1.rows);
        d.d2 = reinterpret_cast<const uint32_t *>(s2.rows);
        d.n1 = s1.n;
        d.n2 = s2.n;
        d.words = s1.fdim ? 0 : s1.words;
        d.fdim = s1.fdim;
        d.segs = reinterpret_cast<const Seg *>(B + o_segs) + seg_first[(size_t)k];
        d.nseg = seg_first[(size_t)k + 1] - seg_first[(size_t)k];
        d.idx1 = s1.idx;
        d.idx2 = s2.idx;
        d.valid1 = B + o_cur;  // "already has a map point": the masks of the call, updated on the device between the neighbours
        d.valid2 = B + o_nb + (size_t)k * cap;
        d.ang_stride = 1;
        d.th = geo[(size_t)k].th_low;
        d.mode = (int)AFV_MATCH_KF_KF;
        T.x1 = s1.x; T.y1 = s1.y;
        T.x2 = s2.x; T.y2 = s2.y;
        T.sigma2_2 = s2.sigma2;
        std::memcpy(T.F, geo[(size_t)k].F12, sizeof(T.F));
        T.ex = geo[(size_t)k].ex;
        T.ey = geo[(size_t)k].ey;
        T.row_seg = reinterpret_cast<const int *>(B + rowseg_off[(size_t)k]);
        T.u_right1 = s1.u_right;
        T.u_right2 = s2.u_right;
        T.only_stereo = geo[(size_t)k].only_stereo != 0;
    }
    HIPCHK(c, b.upload(in_bytes));
    DevNewPtsArgs A{};
    A.search = reinterpret_cast<const DevTriJob *>(B + o_search);
    A.pairs = reinterpret_cast<const DevTriPair *>(B + o_pairs);
    A.nn = nn; A.cap = cap; A.nblk = nblk;
    A.mask_cur = B + o_cur; A.mask_nb = B + o_nb;
    A.match12 = reinterpret_cast<int *>(B + o_match);
    A.status = B + o_status; A.route = B + o_route;
    A.x3d = reinterpret_cast<float *>(B + o_x3d);
    A.new_id = reinterpret_cast<int *>(B + o_id);
    A.n_new = reinterpret_cast<int *>(B + o_nnew);
    A.blk_count = reinterpret_cast<int *>(B + o_blk);
    A.next_id = reinterpret_cast<int *>(B + o_next);
    A.stop = reinterpret_cast<int *>(B + o_stop);
    if (points) A.P = points->P;
    A.has_points = points ? 1 : 0;
    for (int k = 0; k < nn; ++k) {
        afv_launch_newpts_judge(&A, k, c->stream);
        afv_launch_newpts_store(&A, k, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    if (match12) HIPCHK(c, b.fetch(match12, o_match, cells * 4, c->stream));
    if (status) HIPCHK(c, b.fetch(status, o_status, cells, c->stream));
    if (route) HIPCHK(c, b.fetch(route, o_route, cells, c->stream));
    if (x3d) HIPCHK(c, b.fetch(x3d, o_x3d, cells * 12, c->stream));
    if (new_id) HIPCHK(c, b.fetch(new_id, o_id, cells * 4, c->stream));
    HIPCHK(c, b.fetch(n_new, o_nnew, (size_t)nn * 4, c->stream));
    HIPCHK(c, b.fetch(has_mp_cur, o_cur, (size_t)cap, c->stream));
    HIPCHK(c, b.fetch(has_mp_nb, o_nb, cells, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.h.data() + o_stop, B + o_stop, ((size_t)nn + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, b.wait());  // the call's one wait
    const int32_t *stop = reinterpret_cast<const int32_t *>(b.h.data() + o_stop);
    int done = nn;
    for (int k = nn; k >= 1; --k)
        if (stop[k]) done = k - 1;
    *n_done = done;
    if (done == nn) return AFV_OK;
    empty_rows(done);
    c->last_error = std::string(WHO) + ": the new points of neighbour " + std::to_string(done) + " exceed the store's capacity " +
                    std::to_string(points ? points->cap : 0) + "; the neighbours before it stand, it and the later ones did nothing";
    return AFV_ECAPACITY;
}

extern "C" int afv_table_create_new_points(afv_table *t, int32_t cur, const int32_t *neighbours, int nn, const afv_table_tri_job *search,
                                           const afv_tri_points_job *jobs, uint8_t *has_mp_cur, uint8_t *has_mp_nb, afv_points *points,
                                           int32_t first_id, int32_t *match12, uint8_t *status, uint8_t *route, float *x3d, int32_t *new_id,
                                           int32_t *n_new, int32_t *n_done) {
    if (!t || !neighbours || !search || !jobs || !has_mp_cur || !has_mp_nb || !n_new || !n_done || nn < 1 || nn > AFV_TRI_MAX_PAIRS || first_id < 0)
        return AFV_EINVAL;
    if (points) {
        if (!afv_points_is_live(points) || points->c != t->c) return AFV_EINVAL;
        if (points->float_dim != t->float_dim || points->desc_bytes != t->desc_bytes || points->words != t->words) return AFV_EUNSUPPORTED;
    }
    return guarded(t->c, [&] {
        return create_new_points_impl(t, cur, neighbours, nn, search, jobs, has_mp_cur, has_mp_nb, points, first_id, match12, status, route, x3d,
                                      new_id, n_new, n_done);
    });
}
