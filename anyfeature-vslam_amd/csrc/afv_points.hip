// afv_points.hip — host side of the resident map-point store (include/afv_hip.h, "resident map points"; kernels: k_points.hip).
//
// Reference objects: MapPoint (XYZ, normalVector, minDistance / maxDistance, refSize / refDistance / refSigma, the descriptor of
// ComputeDistinctiveDescriptors; src/MapPoint.cc) and the geometry in front of every projection search - Frame::isInFrustum
// (src/Frame.cc:276-331) ahead of SearchByProjection(F, vpMapPoints) (Tracking.cc:988-1028), and the projection loops of
// SearchByProjection(cur, last) (FeatureMatcher.cc:1312-1351), the relocalisation search (:1425-1465) and Fuse (:811-858).  The points live
// in HBM, a frame gets a pose, a search sends point ids.
#include <mutex>
#include <unordered_set>

#include "afv_runtime.h"

// stores alive in the process: afv_points_destroy after afv_destroy is a no-op, as for frames (afv_frame.hip)
static std::mutex g_points_mutex;
static std::unordered_set<const afv_points *> g_live_points;

static void points_free(afv_points *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_points_mutex);
        g_live_points.erase(p);
    }
    if (p->c) (void)hipSetDevice(p->c->device);
    if (p->ev) (void)hipEventDestroy(p->ev);
    if (p->h_pin) (void)hipHostFree(p->h_pin);
    if (p->d_block) (void)hipFree(p->d_block);
    if (p->d_stage) (void)hipFree(p->d_stage);
    if (p->d_covis) (void)hipFree(p->d_covis);
    delete p;
}

bool afv_points_is_live(const afv_points *p) {
    std::lock_guard<std::mutex> lk(g_points_mutex);
    return p && g_live_points.count(p);
}

void afv_points_release_all(afv_ctx *c) {
    std::vector<afv_points *> mine;
    mine.swap(c->points);
    for (afv_points *p : mine) points_free(p);
}

extern "C" int afv_points_create(afv_ctx *c, int capacity, int desc_bytes_in, int float_dim, afv_points **out) {
    if (!c || !out) return AFV_EINVAL;
    *out = nullptr;
    if (capacity < 1 || capacity > AFV_POINTS_MAX_CAPACITY) return AFV_EINVAL;
    if (float_dim != 0 && (float_dim < 4 || float_dim > 1024 || (float_dim & 3))) return AFV_EINVAL;
    const int desc_bytes = float_dim ? 4 * float_dim : (desc_bytes_in == 0 ? AFV_DESC_BYTES : desc_bytes_in);
    if (!float_dim && (desc_bytes < 1 || desc_bytes > 64)) return AFV_EINVAL;
    const int words = float_dim ? float_dim : (desc_bytes <= 32 ? 8 : 16);
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        if (!c->d_points_count) {  // the accumulator and ticket of k_points_project: zero at rest from here on
            HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&c->d_points_count), 2 * sizeof(int)));
            HIPCHK(c, afv_fill(c, c->d_points_count, 0, 2 * sizeof(int)));
        }
        afv_points *p = new (std::nothrow) afv_points();
        if (!p) return AFV_ENOMEM;
        p->c = c;
        p->cap = capacity;
        p->desc_bytes = desc_bytes;
        p->words = words;
        p->float_dim = float_dim;
        size_t off = 0;
        auto take = [&](size_t bytes) {
            const size_t o = off;
            off = align_up(off + bytes, 256);
            return o;
        };
        size_t o_f[11];
        for (size_t &o : o_f) o = take((size_t)capacity * 4);
        const size_t o_flags = take((size_t)capacity), o_desc = take((size_t)capacity * words * 4);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p->d_block), off);
        if (e == hipSuccess) e = hipMemsetAsync(p->d_block, 0, off, c->stream);  // flags 0: nothing is set
        if (e != hipSuccess) {
            c->last_error = std::string("afv_points_create: ") + hipGetErrorString(e);
            points_free(p);
            return e == hipErrorOutOfMemory ? AFV_ENOMEM : AFV_EHIP;
        }
        uint8_t *B = p->d_block;
        DevPointPlanes &P = p->P;
        float **fp[11] = {&P.pos[0], &P.pos[1], &P.pos[2], &P.normal[0], &P.normal[1], &P.normal[2], &P.min_d, &P.max_d, &P.ref_size, &P.ref_dist, &P.ref_sigma};
        for (int i = 0; i < 11; ++i) *fp[i] = reinterpret_cast<float *>(B + o_f[i]);
        P.flags = B + o_flags;
        P.desc = B + o_desc;
        P.cap = capacity;
        P.words = words;
        try {
            c->points.push_back(p);
            std::lock_guard<std::mutex> lk(g_points_mutex);
            g_live_points.insert(p);
        } catch (...) {
            auto it = std::find(c->points.begin(), c->points.end(), p);
            if (it != c->points.end()) c->points.erase(it);
            points_free(p);
            return AFV_ENOMEM;
        }
        *out = p;
        return AFV_OK;
    });
}

extern "C" void afv_points_destroy(afv_points *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_points_mutex);
        if (!g_live_points.count(p)) return;  // released with its context
    }
    afv_ctx *c = p->c;
    auto it = std::find(c->points.begin(), c->points.end(), p);
    if (it == c->points.end()) return;
    c->points.erase(it);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    points_free(p);
}

// ---- staging of the setters: one pinned image, one upload, one launch per call ----
struct PointsStage {
    afv_points *p;
    afv_points *h;  // (the host side of the staging lives in the store)
    size_t bytes = 0;
    size_t take(size_t n) {
        const size_t o = bytes;
        bytes = align_up(bytes + n, 16);
        return o;
    }
    // after every take(): both buffers hold `bytes`; the previous upload has left the pinned image
    int open() {
        afv_ctx *c = p->c;
        h = p;
        if (h->ev_armed) HIPCHK(c, hipEventSynchronize(h->ev));
        h->ev_armed = false;
        if (bytes > h->pin_bytes) {
            if (h->h_pin) (void)hipHostFree(h->h_pin);
            h->h_pin = nullptr;
            h->pin_bytes = 0;
            const size_t want = align_up(bytes + bytes / 2, 1 << 16);
            HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&h->h_pin), want, hipHostMallocDefault));
            h->pin_bytes = want;
        }
        if (bytes > p->stage_bytes) {  // grow-only; hipFree waits for the work that still reads the old buffer
            if (p->d_stage) (void)hipFree(p->d_stage);
            p->d_stage = nullptr;
            p->stage_bytes = 0;
            const size_t want = align_up(bytes + bytes / 2, 1 << 16);
            HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&p->d_stage), want));
            p->stage_bytes = want;
        }
        if (!h->ev) HIPCHK(c, hipEventCreateWithFlags(&h->ev, hipEventDisableTiming));
        return AFV_OK;
    }
    size_t put(size_t off, const void *src, size_t n) {
        std::memcpy(h->h_pin + off, src, n);
        return off;
    }
    int upload(size_t n) {
        afv_ctx *c = p->c;
        HIPCHK(c, hipMemcpyAsync(p->d_stage, h->h_pin, n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(h->ev, c->stream));
        h->ev_armed = true;
        return AFV_OK;
    }
};

static bool ids_ok(const afv_points *p, const int32_t *ids, int n) {
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= p->cap) return false;
    return true;
}

static int points_set_fields(afv_points *p, const int32_t *ids, int n, const float *pos, const float *normal, const float *const f5[5],
                             const uint8_t *bad, const uint8_t *observed, int mark_set) {
    if (!p || n < 0 || (n > 0 && !ids)) return AFV_EINVAL;
    if (!ids_ok(p, ids, n)) return AFV_EINVAL;
    if (n == 0) return AFV_OK;
    afv_ctx *c = p->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        PointsStage S{p, nullptr};
        const size_t N = (size_t)n;
        const size_t o_ids = S.take(N * 4), o_pos = pos ? S.take(N * 12) : 0, o_nrm = normal ? S.take(N * 12) : 0;
        size_t o_f[5];
        for (int k = 0; k < 5; ++k) o_f[k] = f5[k] ? S.take(N * 4) : 0;
        const size_t o_bad = bad ? S.take(N) : 0, o_obs = observed ? S.take(N) : 0;
        int rc = S.open();
        if (rc) return rc;
        S.put(o_ids, ids, N * 4);
        if (pos) S.put(o_pos, pos, N * 12);
        if (normal) S.put(o_nrm, normal, N * 12);
        for (int k = 0; k < 5; ++k)
            if (f5[k]) S.put(o_f[k], f5[k], N * 4);
        if (bad) S.put(o_bad, bad, N);
        if (observed) S.put(o_obs, observed, N);
        rc = S.upload(S.bytes);
        if (rc) return rc;
        uint8_t *D = p->d_stage;
        DevPointsMove M{};
        M.P = p->P;
        M.ids = reinterpret_cast<const int *>(D + o_ids);
        M.n = n;
        M.pos = pos ? reinterpret_cast<float *>(D + o_pos) : nullptr;
        M.normal = normal ? reinterpret_cast<float *>(D + o_nrm) : nullptr;
        float **dst[5] = {&M.min_d, &M.max_d, &M.ref_size, &M.ref_dist, &M.ref_sigma};
        for (int k = 0; k < 5; ++k) *dst[k] = f5[k] ? reinterpret_cast<float *>(D + o_f[k]) : nullptr;
        M.bad = bad ? D + o_bad : nullptr;
        M.observed = observed ? D + o_obs : nullptr;
        M.mark_set = mark_set;
        afv_launch_points_move(&M, c->stream);
        HIPCHK(c, hipGetLastError());
        return AFV_OK;
    });
}

extern "C" int afv_points_set(afv_points *p, const int32_t *ids, int n, const float *pos, const float *normal, const float *min_d,
                              const float *max_d, const float *ref_size, const float *ref_dist, const float *ref_sigma) {
    const float *const f5[5] = {min_d, max_d, ref_size, ref_dist, ref_sigma};
    return points_set_fields(p, ids, n, pos, normal, f5, nullptr, nullptr, 1);
}

extern "C" int afv_points_set_flags(afv_points *p, const int32_t *ids, int n, const uint8_t *bad, const uint8_t *observed) {
    const float *const f5[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    return points_set_fields(p, ids, n, nullptr, nullptr, f5, bad, observed, 0);
}

extern "C" int afv_points_set_descriptors(afv_points *p, const int32_t *ids, int n, const uint8_t *rows) {
    if (!p || n < 0 || (n > 0 && (!ids || !rows))) return AFV_EINVAL;
    if (!ids_ok(p, ids, n)) return AFV_EINVAL;
    if (n == 0) return AFV_OK;
    afv_ctx *c = p->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        PointsStage S{p, nullptr};
        const size_t N = (size_t)n, row = (size_t)p->words * 4;
        const size_t o_ids = S.take(N * 4), o_rows = S.take(N * row);
        int rc = S.open();
        if (rc) return rc;
        S.put(o_ids, ids, N * 4);
        uint8_t *hb = S.h->h_pin + o_rows;
        if ((size_t)p->desc_bytes == row) {
            std::memcpy(hb, rows, N * row);
        } else {  // rows of desc_bytes -> zero-padded device rows, as afv_frame_set_features
            for (size_t i = 0; i < N; ++i) {
                std::memcpy(hb + i * row, rows + i * p->desc_bytes, (size_t)p->desc_bytes);
                std::memset(hb + i * row + p->desc_bytes, 0, row - (size_t)p->desc_bytes);
            }
        }
        rc = S.upload(S.bytes);
        if (rc) return rc;
        afv_launch_points_rows(&p->P, reinterpret_cast<const int *>(p->d_stage + o_ids), n, p->d_stage + o_rows, nullptr, 0, nullptr, nullptr, 0, c->stream);
        HIPCHK(c, hipGetLastError());
        return AFV_OK;
    });
}

extern "C" int afv_points_set_descriptors_from_table(afv_points *p, const int32_t *ids, int n, afv_table *t, const int32_t *slot, const int32_t *idx) {
    if (!p || !t || n < 0 || (n > 0 && (!ids || !slot || !idx))) return AFV_EINVAL;
    if (t->c != p->c) return AFV_EINVAL;
    if (t->float_dim != p->float_dim || t->desc_bytes != p->desc_bytes || t->words != p->words) return AFV_EUNSUPPORTED;  // rows of another kind / width
    if (!ids_ok(p, ids, n)) return AFV_EINVAL;
    for (int i = 0; i < n; ++i)
        if (slot[i] < 0 || slot[i] >= t->nsets || idx[i] < 0 || idx[i] >= t->h_n[(size_t)slot[i]]) return AFV_EINVAL;
    if (n == 0) return AFV_OK;
    afv_ctx *c = p->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        PointsStage S{p, nullptr};
        const size_t N = (size_t)n;
        const size_t o_ids = S.take(N * 4), o_slot = S.take(N * 4), o_idx = S.take(N * 4);
        int rc = S.open();
        if (rc) return rc;
        S.put(o_ids, ids, N * 4);
        S.put(o_slot, slot, N * 4);
        S.put(o_idx, idx, N * 4);
        rc = S.upload(S.bytes);
        if (rc) return rc;
        const uint8_t *D = p->d_stage;
        afv_launch_points_rows(&p->P, reinterpret_cast<const int *>(D + o_ids), n, nullptr, t->d_desc, t->cap, reinterpret_cast<const int *>(D + o_slot),
                               reinterpret_cast<const int *>(D + o_idx), 0, c->stream);
        HIPCHK(c, hipGetLastError());
        return AFV_OK;
    });
}

extern "C" int afv_points_get(afv_points *p, const int32_t *ids, int n, float *pos, float *normal, float *min_d, float *max_d, float *ref_size,
                              float *ref_dist, float *ref_sigma, uint8_t *flags, uint8_t *rows) {
    if (!p || n < 0 || (n > 0 && !ids)) return AFV_EINVAL;
    if (!ids_ok(p, ids, n)) return AFV_EINVAL;
    if (n == 0) return AFV_OK;
    afv_ctx *c = p->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        PointsStage S{p, nullptr};
        const size_t N = (size_t)n, row = (size_t)p->words * 4;
        const size_t o_ids = S.take(N * 4);
        const size_t in_bytes = S.bytes;
        const size_t o_pos = S.take(N * 12), o_nrm = S.take(N * 12);
        size_t o_f[5];
        for (size_t &o : o_f) o = S.take(N * 4);
        const size_t o_flags = S.take(N), o_rows = S.take(N * row);
        int rc = S.open();
        if (rc) return rc;
        S.put(o_ids, ids, N * 4);
        rc = S.upload(in_bytes);
        if (rc) return rc;
        uint8_t *D = p->d_stage;
        DevPointsMove M{};
        M.P = p->P;
        M.ids = reinterpret_cast<const int *>(D + o_ids);
        M.n = n;
        M.gather = 1;
        M.pos = reinterpret_cast<float *>(D + o_pos);
        M.normal = reinterpret_cast<float *>(D + o_nrm);
        float **dst[5] = {&M.min_d, &M.max_d, &M.ref_size, &M.ref_dist, &M.ref_sigma};
        for (int k = 0; k < 5; ++k) *dst[k] = reinterpret_cast<float *>(D + o_f[k]);
        M.flags = D + o_flags;
        afv_launch_points_move(&M, c->stream);
        afv_launch_points_rows(&p->P, M.ids, n, D + o_rows, nullptr, 0, nullptr, nullptr, 1, c->stream);
        HIPCHK(c, hipGetLastError());
        uint8_t *H = S.h->h_pin;
        HIPCHK(c, hipMemcpyAsync(H + in_bytes, D + in_bytes, S.bytes - in_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        S.h->ev_armed = false;
        if (pos) std::memcpy(pos, H + o_pos, N * 12);
        if (normal) std::memcpy(normal, H + o_nrm, N * 12);
        float *outs[5] = {min_d, max_d, ref_size, ref_dist, ref_sigma};
        for (int k = 0; k < 5; ++k)
            if (outs[k]) std::memcpy(outs[k], H + o_f[k], N * 4);
        if (flags) std::memcpy(flags, H + o_flags, N);
        if (rows)
            for (size_t i = 0; i < N; ++i) std::memcpy(rows + i * p->desc_bytes, H + o_rows + i * row, (size_t)p->desc_bytes);
        return AFV_OK;
    });
}

// ---- the pose of a resident frame ----
extern "C" int afv_frame_set_pose(afv_frame *f, const float *Rcw, const float *tcw, const float *Ow, float fx, float fy, float cx, float cy, float mbf) {
    if (!f || !Rcw || !tcw || !Ow) return AFV_EINVAL;
    std::memcpy(f->Rcw, Rcw, sizeof(f->Rcw));
    std::memcpy(f->tcw, tcw, sizeof(f->tcw));
    std::memcpy(f->Ow, Ow, sizeof(f->Ow));
    f->fx = fx; f->fy = fy; f->cx = cx; f->cy = cy; f->mbf = mbf;
    f->has_pose = true;
    return AFV_OK;
}

// ---- the searches through ids ----
// A call that fails after k_points_project went out may leave the context's accumulator and ticket armed (a launch that did not run to
// its end): they are put back to zero behind whatever is still on the stream, as the ticket of the one-launch search is
static int points_call_failed(afv_ctx *c, int rc) {
    if (rc != AFV_OK && c->d_points_count) (void)hipMemsetAsync(c->d_points_count, 0, 2 * sizeof(int), c->stream);
    return rc;
}
// the caller's record in the current layout, checked against the frame: everything the header promises to refuse before a launch
static int load_search(afv_frame *f, const afv_point_search *caller, afv_point_search &s) {
    if (!f || !caller) return AFV_EINVAL;
    const uint32_t ss = caller->struct_size;
    if (ss < offsetof(afv_point_search, check_orientation) + sizeof(int32_t) || ss > 4 * sizeof(afv_point_search) || (ss & 3)) return AFV_EINVAL;
    s = afv_point_search{};
    std::memcpy(&s, caller, std::min<size_t>(ss, sizeof(s)));
    if (s.flavour < AFV_PT_FRUSTUM || s.flavour > AFV_PT_FUSE) return AFV_EINVAL;
    if (!s.points || s.nq < 0 || s.nq > 65535 || (s.nq > 0 && !s.ids)) return AFV_EINVAL;
    {
        std::lock_guard<std::mutex> lk(g_points_mutex);
        if (!g_live_points.count(s.points)) return AFV_EINVAL;
    }
    if (s.points->c != f->c) return AFV_EINVAL;
    if (s.points->float_dim != f->float_dim || s.points->desc_bytes != f->desc_bytes) return AFV_EUNSUPPORTED;
    if (!f->has_pose || !f->has_features || !f->has_grid) return AFV_EINVAL;
    // the frame in the query role is read by LASTFRAME (sizes, angles) and by RELOC without host angles; elsewhere the field is ignored
    const bool reads_qframe = s.flavour == AFV_PT_LASTFRAME || (s.flavour == AFV_PT_RELOC && !s.qangle && s.qframe);
    if (s.flavour == AFV_PT_LASTFRAME && !s.qframe) return AFV_EINVAL;
    if (reads_qframe && (!afv_frame_is_live(s.qframe) || s.qframe->c != f->c || !s.qframe->has_features || s.nq > s.qframe->n)) return AFV_EINVAL;
    if (!reads_qframe) s.qframe = nullptr;
    for (int q = 0; q < s.nq; ++q)
        if (s.ids[q] < -1 || s.ids[q] >= s.points->cap) return AFV_EINVAL;
    return AFV_OK;
}

static void fill_points_job(const afv_frame *f, const afv_point_search &s, DevPointsJob &J) {
    J = DevPointsJob{};
    J.P = s.points->P;
    J.nq = s.nq;
    J.flavour = s.flavour;
    std::memcpy(J.R, f->Rcw, sizeof(J.R));
    std::memcpy(J.t, f->tcw, sizeof(J.t));
    std::memcpy(J.Ow, f->Ow, sizeof(J.Ow));
    J.fx = f->fx; J.fy = f->fy; J.cx = f->cx; J.cy = f->cy; J.mbf = f->mbf;
    J.min_x = f->p.min_x; J.max_x = f->p.max_x; J.min_y = f->p.min_y; J.max_y = f->p.max_y;
    J.rs_th = s.radius_scale * s.radius_th;  // FeatureMatcher.cc:91: radiusScale * radiusTh, the first product of the radius
    J.cos_limit = s.viewing_cos_limit;
    J.tol = f->c->p.scale_factor;            // Frame.cc:73
    J.last_size = s.flavour == AFV_PT_LASTFRAME ? s.qframe->d_size : nullptr;
}

static int search_points(afv_frame *f, const afv_point_search *caller, int kind, int use_inf_gate, int32_t *out, int32_t *nm, uint8_t *in_view,
                         int32_t *n_in_view) {
    afv_point_search s;
    const int rc0 = load_search(f, caller, s);
    if (rc0) return rc0;
    if (!out || !nm) return AFV_EINVAL;
    if ((kind == AFV_KIND_FUSE) != (s.flavour == AFV_PT_FUSE)) return AFV_EINVAL;
    afv_ctx *c = f->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        PointQueries pq;
        fill_points_job(f, s, pq.job);
        pq.ids = s.ids;
        pq.in_view = in_view;
        ProjJobSpec J = afv_frame_proj_spec(f, kind == AFV_KIND_FUSE && use_inf_gate);
        J.f.occupied = kind == AFV_KIND_FUSE ? nullptr : s.occupied;
        ProjQueries &Q = J.q;
        Q.nq = s.nq;
        Q.from = ProjQueries::POINT_IDS;
        Q.points = &pq;
        // the angles alone are not made from the ids: the last frame's / the keyframe's, from a resident frame in that role or (RELOC) a host array
        if (s.qframe && (s.flavour == AFV_PT_LASTFRAME || (s.flavour == AFV_PT_RELOC && !s.qangle))) {
            Q.angle = s.qframe->d_angle;
            Q.angle_on_device = true;
        } else if (s.flavour == AFV_PT_RELOC) {
            Q.angle = s.qangle;
        }
        J.th = s.th_high; J.ratio = s.nnratio;
        J.check_ori = (s.flavour == AFV_PT_FRUSTUM || kind == AFV_KIND_FUSE) ? 0 : s.check_orientation;
        J.mode = s.flavour == AFV_PT_FRUSTUM ? AFV_PROJ_LOCALMAP : AFV_PROJ_LASTFRAME;
        J.stereo = s.flavour != AFV_PT_RELOC;  // every flavour but RELOC has a stereo gate
        const int rc = afv_project_run(c, &J, 1, kind, out, nm);
        if (rc) return points_call_failed(c, rc);
        if (n_in_view) *n_in_view = pq.n_in_view;
        return AFV_OK;
    });
}

extern "C" int afv_frame_search_points(afv_frame *f, const afv_point_search *s, int32_t *assign, int32_t *nmatches, uint8_t *in_view, int32_t *n_in_view) {
    return search_points(f, s, AFV_KIND_PROJ, 0, assign, nmatches, in_view, n_in_view);
}

extern "C" int afv_frame_fuse_points(afv_frame *f, const afv_point_search *s, int use_inf_gate, int32_t *best, int32_t *nfound) {
    return search_points(f, s, AFV_KIND_FUSE, use_inf_gate, best, nfound, nullptr, nullptr);
}

extern "C" int afv_frame_project_points(afv_frame *f, const afv_point_search *caller, afv_point_projection *host_out) {
    afv_point_search s;
    const int rc0 = load_search(f, caller, s);
    if (rc0) return rc0;
    if (!host_out || host_out->struct_size < sizeof(afv_point_projection) || host_out->struct_size > 4 * sizeof(afv_point_projection)) return AFV_EINVAL;
    afv_ctx *c = f->c;
    return guarded(c, [&]() -> int {
        host_out->n_in_view = 0;
        if (s.nq == 0) return AFV_OK;
        HIPCHK(c, hipSetDevice(c->device));
        Blob b(c);
        const size_t nq4 = (size_t)s.nq * 4;
        const size_t o_ids = b.put(s.ids, nq4);
        const size_t in_bytes = b.h.size();
        const size_t o_count = b.reserve_scratch(16);
        size_t o_f[10];  // u v r qmin qmax ur er size sigma cos
        for (size_t &o : o_f) o = b.reserve_scratch(nq4);
        const size_t o_valid = b.reserve_scratch((size_t)s.nq), o_occ = b.reserve_scratch((size_t)s.nq);
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        uint8_t *B = c->d_match;
        HIPCHK(c, b.upload(in_bytes));
        DevPointsJob J;
        fill_points_job(f, s, J);
        J.ids = reinterpret_cast<const int *>(B + o_ids);
        float **dst[10] = {&J.qu, &J.qv, &J.qr, &J.qmin, &J.qmax, &J.q_ur, &J.q_er, &J.o_size, &J.o_sigma, &J.o_cos};
        for (int k = 0; k < 10; ++k) *dst[k] = reinterpret_cast<float *>(B + o_f[k]);
        J.qvalid = B + o_valid;
        J.qocc = B + o_occ;
        J.qd = nullptr;
        J.count = c->d_points_count;
        J.ticket = c->d_points_count + 1;
        J.count_out = reinterpret_cast<int *>(B + o_count);
        afv_launch_points_project(&J, c->stream);
        return points_call_failed(c, [&]() -> int {
            HIPCHK(c, hipGetLastError());
            float *outs[10] = {host_out->u, host_out->v, host_out->r, host_out->qmin, host_out->qmax, host_out->ur, host_out->er, host_out->size, host_out->sigma,
                               host_out->view_cos};
            for (int k = 0; k < 10; ++k)
                if (outs[k]) HIPCHK(c, b.fetch(outs[k], o_f[k], nq4, c->stream));
            if (host_out->in_view) HIPCHK(c, b.fetch(host_out->in_view, o_valid, (size_t)s.nq, c->stream));
            HIPCHK(c, b.fetch(&host_out->n_in_view, o_count, 4, c->stream));
            HIPCHK(c, b.wait());
            return AFV_OK;
        }());
    });
}
