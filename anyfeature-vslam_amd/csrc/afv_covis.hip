// afv_covis.hip — host side of afv_table_covis_votes and afv_table_local_points (include/afv_covis.h; kernels: k_covis.hip): the counts behind
// KeyFrame::UpdateConnections (KeyFrame.cc:329-418) and Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (Tracking.cc:1040-1104), read
// from the mvpMapPoints planes of the table and the flags of the store.  Staging: the Blob of afv_runtime.h, one upload, one wait.
#include <algorithm>
#include <unordered_set>

#include "afv_runtime.h"
#include "k_covis.h"

namespace {

template <class T>
T *at(uint8_t *base, size_t off) { return reinterpret_cast<T *>(base + off); }

// table and store of one context, planes the kernels can take
int cv_check_pair(const afv_table *t, const afv_points *p) {
    if (!afv_points_is_live(p) || p->c != t->c) return AFV_EINVAL;
    if (t->cap > AFV_COVIS_MAX_CAP) return AFV_EUNSUPPORTED;
    return AFV_OK;
}

// distinct slots in range, each with a plane
int cv_check_slots(const afv_table *t, const int32_t *slots, int n) {
    if (n > 0 && (t->kf_pose.empty() || !t->d_mp)) return AFV_EINVAL;
    std::vector<uint8_t> seen((size_t)t->nsets, 0);
    for (int k = 0; k < n; ++k) {
        const int s = slots[k];
        if (s < 0 || s >= t->nsets || seen[(size_t)s] || !t->kf_has_mp[(size_t)s]) return AFV_EINVAL;
        seen[(size_t)s] = 1;
    }
    return AFV_OK;
}

int cv_check_ids(const int32_t *ids, int n, int cap) {
    for (int i = 0; i < n; ++i)
        if (ids[i] < -1 || ids[i] >= cap) return AFV_EINVAL;
    return AFV_OK;
}

// the store's first-occurrence words and positions, made with the first local-points call: words 0xFFFFFFFF at rest
int cv_ensure_words(afv_points *p) {
    if (p->d_covis) return AFV_OK;
    afv_ctx *c = p->c;
    const size_t bytes = (size_t)p->cap * 4;
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&p->d_covis), 2 * bytes));
    HIPCHK(c, afv_fill(c, p->d_covis, 0xff, 2 * bytes));
    return AFV_OK;
}

}  // namespace

extern "C" int afv_table_covis_votes(afv_table *t, afv_points *points, const int32_t *slots, const int32_t *key_id, const uint8_t *kf_bad, int nk,
                                     const afv_covis_query *queries, int nq, int32_t *votes, int32_t *order, int32_t *n_order, int32_t *best,
                                     int32_t *n_nonzero) {
    if (!t || !points || !slots || !key_id || !queries || !n_order || !best || !n_nonzero) return AFV_EINVAL;
    if (nk < 1 || nk > AFV_COVIS_MAX_KF || nq < 1 || nq > AFV_COVIS_MAX_QUERIES) return AFV_EINVAL;
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        int rc = cv_check_pair(t, points);
        if (rc) return rc;
        std::vector<afv_covis_query> Q;
        if (!afv_load_jobs(queries, nq, sizeof(afv_covis_query), Q)) return AFV_EINVAL;
        rc = cv_check_slots(t, slots, nk);
        if (rc) return rc;
        {
            std::unordered_set<int32_t> keys(key_id, key_id + nk);
            if ((int)keys.size() != nk) return AFV_EINVAL;
        }
        int max_n = 0;
        for (const afv_covis_query &q : Q) {
            if (q.skip_bad != 0 && q.skip_bad != 1) return AFV_EINVAL;
            if (q.skip_bad && !kf_bad) return AFV_EINVAL;
            if (q.kind == AFV_COVIS_QUERY_SLOT) {
                if (q.position < 0 || q.position >= nk) return AFV_EINVAL;
                max_n = std::max(max_n, t->h_n[(size_t)slots[q.position]]);
            } else if (q.kind == AFV_COVIS_QUERY_IDS) {
                if (q.n < 0 || q.n > AFV_COVIS_MAX_IDS || (q.n > 0 && !q.ids)) return AFV_EINVAL;
                rc = cv_check_ids(q.ids, q.n, points->cap);
                if (rc) return rc;
                max_n = std::max(max_n, q.n);
            } else {
                return AFV_EINVAL;
            }
        }
        HIPCHK(c, hipSetDevice(c->device));
        // 1. the layout: the keyframe list, the id lists, the records; then device-only scratch and the results
        Blob b(c);
        std::vector<int32_t> kf_n((size_t)nk);
        for (int k = 0; k < nk; ++k) kf_n[(size_t)k] = t->h_n[(size_t)slots[k]];
        const size_t slots_off = b.put(slots, (size_t)nk * 4), n_off = b.put(kf_n.data(), (size_t)nk * 4), key_off = b.put(key_id, (size_t)nk * 4);
        const size_t bad_off = kf_bad ? b.put(kf_bad, (size_t)nk) : 0;
        std::vector<size_t> src_off((size_t)nq, 0), dst_off((size_t)nq, 0);
        for (int q = 0; q < nq; ++q)
            if (Q[(size_t)q].kind == AFV_COVIS_QUERY_IDS && Q[(size_t)q].n > 0) src_off[(size_t)q] = b.put(Q[(size_t)q].ids, (size_t)Q[(size_t)q].n * 4);
        const size_t rec_off = b.reserve((size_t)nq * sizeof(DevCovisQuery));
        const size_t in_bytes = b.h.size();
        for (int q = 0; q < nq; ++q) {
            const afv_covis_query &j = Q[(size_t)q];
            const int n = j.kind == AFV_COVIS_QUERY_SLOT ? t->h_n[(size_t)slots[j.position]] : j.n;
            dst_off[(size_t)q] = b.reserve_scratch((size_t)std::max(n, 1) * 4);
        }
        const size_t row = (size_t)nq * nk * 4;
        const size_t votes_off = b.reserve_scratch(row), order_off = b.reserve_scratch(row);
        const size_t no_off = b.reserve_scratch((size_t)nq * 4), best_off = b.reserve_scratch((size_t)nq * 4), nz_off = b.reserve_scratch((size_t)nq * 4);
        rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        // 2. the records, against the device buffer as it stands now
        uint8_t *B = c->d_match, *H = b.h.data();
        for (int q = 0; q < nq; ++q) {
            const afv_covis_query &j = Q[(size_t)q];
            DevCovisQuery &D = at<DevCovisQuery>(H, rec_off)[q];
            D = DevCovisQuery{};
            if (j.kind == AFV_COVIS_QUERY_SLOT) {
                const size_t s = (size_t)slots[j.position];
                D.src = t->d_mp + s * t->cap;
                D.n = t->h_n[s];
                D.self = j.position;
            } else {
                D.src = at<const int>(B, src_off[(size_t)q]);
                D.n = j.n;
                D.self = -1;
            }
            D.dst = at<int>(B, dst_off[(size_t)q]);
            D.th = j.th;
            D.skip_bad = j.skip_bad;
        }
        DevCovisVotes A{};
        A.mp = t->d_mp; A.cap = t->cap; A.nk = nk; A.nq = nq;
        A.slots = at<const int>(B, slots_off); A.kf_n = at<const int>(B, n_off); A.key_id = at<const int>(B, key_off);
        A.kf_bad = kf_bad ? B + bad_off : nullptr;
        A.queries = at<const DevCovisQuery>(B, rec_off);
        A.votes = at<int>(B, votes_off); A.order = at<int>(B, order_off);
        A.n_order = at<int>(B, no_off); A.best = at<int>(B, best_off); A.n_nonzero = at<int>(B, nz_off);
        // 3. one upload, filter, votes, order; one wait
        HIPCHK(c, b.upload(in_bytes));
        afv_launch_covis_votes(&points->P, &A, max_n, c->stream);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            c->last_error = std::string("afv_table_covis_votes launch: ") + hipGetErrorString(e);
            return AFV_EHIP;
        }
        if (votes) HIPCHK(c, b.fetch(votes, votes_off, row, c->stream));
        if (order) HIPCHK(c, b.fetch(order, order_off, row, c->stream));
        HIPCHK(c, b.fetch(n_order, no_off, (size_t)nq * 4, c->stream));
        HIPCHK(c, b.fetch(best, best_off, (size_t)nq * 4, c->stream));
        HIPCHK(c, b.fetch(n_nonzero, nz_off, (size_t)nq * 4, c->stream));
        HIPCHK(c, b.wait());
        return AFV_OK;
    });
}

extern "C" int afv_table_local_points(afv_table *t, afv_points *points, const int32_t *local, int nl, const int32_t *frame_pts, int n_pts, int max_out,
                                      int32_t *ids_out, uint8_t *seen_out, int32_t *n_out) {
    if (!t || !points || !n_out || nl < 0 || nl > AFV_COVIS_MAX_LOCAL || max_out < 0) return AFV_EINVAL;
    if ((nl > 0 && !local) || (max_out > 0 && !ids_out)) return AFV_EINVAL;
    if (n_pts < 0 || n_pts > AFV_COVIS_MAX_IDS || (n_pts > 0 && !frame_pts)) return AFV_EINVAL;
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        int rc = cv_check_pair(t, points);
        if (rc) return rc;
        rc = cv_check_slots(t, local, nl);
        if (rc) return rc;
        rc = cv_check_ids(frame_pts, n_pts, points->cap);
        if (rc) return rc;
        if (nl == 0) {
            *n_out = 0;
            return AFV_OK;
        }
        HIPCHK(c, hipSetDevice(c->device));
        rc = cv_ensure_words(points);
        if (rc) return rc;
        std::vector<int32_t> local_n((size_t)nl);
        size_t cand = 0;
        int max_n = 0;
        for (int l = 0; l < nl; ++l) {
            local_n[(size_t)l] = t->h_n[(size_t)local[l]];
            cand += (size_t)local_n[(size_t)l];
            max_n = std::max(max_n, local_n[(size_t)l]);
        }
        const size_t room = std::min<size_t>((size_t)max_out, cand);  // no answer is longer than the candidates
        const bool want_seen = seen_out != nullptr;
        Blob b(c);
        const size_t local_off = b.put(local, (size_t)nl * 4), n_off = b.put(local_n.data(), (size_t)nl * 4);
        const size_t pts_off = n_pts > 0 ? b.put(frame_pts, (size_t)n_pts * 4) : 0;
        const size_t in_bytes = b.h.size();
        const size_t count_off = b.reserve_scratch((size_t)nl * 4), total_off = b.reserve_scratch(4);
        const size_t ids_off = b.reserve_scratch(std::max<size_t>(room, 1) * 4), seen_off = b.reserve_scratch(std::max<size_t>(room, 1));
        rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        uint8_t *B = c->d_match, *H = b.h.data();
        DevCovisLocal A{};
        A.P = points->P;
        A.mp = t->d_mp; A.cap = t->cap; A.nl = nl;
        A.local = at<const int>(B, local_off); A.local_n = at<const int>(B, n_off);
        A.frame_pts = n_pts > 0 ? at<const int>(B, pts_off) : nullptr;
        A.n_pts = n_pts;
        A.max_out = (int)room;  // a total beyond the caller's max_out is beyond room too: total <= cand
        A.word = points->d_covis; A.pos = reinterpret_cast<int *>(points->d_covis + points->cap);
        A.count = at<int>(B, count_off); A.total = at<int>(B, total_off);
        A.ids_out = at<int>(B, ids_off);
        A.seen = want_seen ? B + seen_off : nullptr;
        HIPCHK(c, b.upload(in_bytes));
        if (want_seen && room) HIPCHK(c, hipMemsetAsync(B + seen_off, 0, room, c->stream));
        afv_launch_covis_local(&A, max_n, c->stream);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            c->last_error = std::string("afv_table_local_points launch: ") + hipGetErrorString(e);
            return AFV_EHIP;
        }
        // the answer's length is known after the wait: everything it can be comes back in the one transfer, the caller gets `total` entries
        HIPCHK(c, hipMemcpyAsync(H + total_off, B + total_off, 4, hipMemcpyDeviceToHost, c->stream));
        if (room) HIPCHK(c, hipMemcpyAsync(H + ids_off, B + ids_off, room * 4, hipMemcpyDeviceToHost, c->stream));
        if (want_seen && room) HIPCHK(c, hipMemcpyAsync(H + seen_off, B + seen_off, room, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, b.wait());
        const int total = *at<const int>(H, total_off);
        if (total > max_out) {
            c->last_error = "afv_table_local_points: the local points exceed max_out";
            return AFV_ECAPACITY;
        }
        if (total > 0) {
            std::memcpy(ids_out, H + ids_off, (size_t)total * 4);
            if (want_seen) std::memcpy(seen_out, H + seen_off, (size_t)total);
        }
        *n_out = total;
        return AFV_OK;
    });
}
