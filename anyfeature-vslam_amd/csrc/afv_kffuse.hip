// afv_kffuse.hip — host side of afv_table_fuse_points (include/afv_hip.h, "fusing map points into keyframes of the table"): FeatureMatcher::Fuse
// (FeatureMatcher.cc:794-940, :942-1064) into up to 64 slots of the keyframe table per call, as LocalMapping::SearchInNeighbors
// (LocalMapping.cc:475-555) and LoopClosing::SearchAndFuse (LoopClosing.cc:601-628) run it.  Also what a slot holds for it: the table's
// camera, the pose and the mvpMapPoints plane of a slot, the grid of KeyFrame::GetFeaturesInArea.
// No kernel lives here: the geometry and the membership test are k_kffuse_project (k_points.hip, the text of k_points_project), the search is
// k_match_fuse (k_project.hip) over the job records every projection search uses, the grid is k_frame_grid (k_frame.hip), the occupant lookup
// k_kffuse_finish (k_points.hip).  Staging: the Blob of afv_runtime.h, one upload, one wait.
#include "afv_runtime.h"

namespace {

void kf_ensure_host(afv_table *t) {
    if (!t->kf_pose.empty()) return;
    t->kf_pose.assign((size_t)t->nsets, KfPose{});
    t->kf_has_pose.assign((size_t)t->nsets, 0);
    t->kf_has_mp.assign((size_t)t->nsets, 0);
    t->kf_grid_ok.assign((size_t)t->nsets, 0);
}

int kf_ensure_plane(afv_table *t) {
    if (t->d_mp) return AFV_OK;
    afv_ctx *c = t->c;
    const size_t bytes = (size_t)t->nsets * t->cap * sizeof(int32_t);
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&t->d_mp), bytes));
    HIPCHK(c, afv_fill(c, t->d_mp, 0xff, bytes));  // -1: no point
    return AFV_OK;
}

// the grid planes of every slot, for the camera as it stands (a camera with another cell count: allocated again)
int kf_ensure_grid(afv_table *t) {
    afv_ctx *c = t->c;
    const int cells = t->cam.grid_cols * t->cam.grid_rows;
    if (t->d_kf_cell_ptr && t->kf_cells != cells) {
        (void)hipFree(t->d_kf_cell_ptr);  // (hipFree waits for the work that still reads it)
        t->d_kf_cell_ptr = nullptr;
    }
    if (!t->d_kf_cell_ptr) {
        HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&t->d_kf_cell_ptr), (size_t)t->nsets * ((size_t)cells + 1) * sizeof(int)));
        t->kf_cells = cells;
        std::fill(t->kf_grid_ok.begin(), t->kf_grid_ok.end(), 0);
    }
    if (!t->d_kf_cell_ent) HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&t->d_kf_cell_ent), (size_t)t->nsets * t->cap * sizeof(int4)));
    return AFV_OK;
}

template <class T>
T *at(uint8_t *base, size_t off) { return reinterpret_cast<T *>(base + off); }

// one list of ids of a call: jobs that pass the same pointer and length share its upload and its descriptor gather
struct IdList {
    const int32_t *ids;
    int nq;
    size_t ids_off, rows_off;
};

}  // namespace

void afv_kffuse_slot_reset(afv_table *t, int slot) {
    if (t->kf_pose.empty()) return;
    t->kf_has_pose[(size_t)slot] = 0;
    t->kf_has_mp[(size_t)slot] = 0;
    t->kf_grid_ok[(size_t)slot] = 0;
}

void afv_kffuse_grid_stale(afv_table *t, int slot) {
    if (t->kf_pose.empty()) return;
    if (slot < 0) std::fill(t->kf_grid_ok.begin(), t->kf_grid_ok.end(), 0);
    else t->kf_grid_ok[(size_t)slot] = 0;
}

void afv_kffuse_free(afv_table *t) {
    void *ptrs[] = {t->d_mp, t->d_kf_cell_ptr, t->d_kf_cell_ent};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    t->d_mp = nullptr;
    t->d_kf_cell_ptr = nullptr;
    t->d_kf_cell_ent = nullptr;
}

// afv_table_clone: camera, poses and the plane travel like inf and scale; the grids are built again on demand
int afv_kffuse_clone(const afv_table *src, afv_table *dst) {
    afv_ctx *c = dst->c;
    dst->has_camera = src->has_camera;
    dst->cam = src->cam;
    if (src->kf_pose.empty()) {
        if (!dst->kf_pose.empty())
            for (int s = 0; s < dst->nsets; ++s) afv_kffuse_slot_reset(dst, s);
        return AFV_OK;
    }
    kf_ensure_host(dst);
    dst->kf_pose = src->kf_pose;
    dst->kf_has_pose = src->kf_has_pose;
    dst->kf_has_mp = src->kf_has_mp;
    std::fill(dst->kf_grid_ok.begin(), dst->kf_grid_ok.end(), 0);
    if (src->d_mp) {
        const int rc = kf_ensure_plane(dst);
        if (rc) return rc;
        HIPCHK(c, afv_copy_dd(c, dst->d_mp, src->d_mp, (size_t)dst->nsets * dst->cap * sizeof(int32_t)));
    } else {
        std::fill(dst->kf_has_mp.begin(), dst->kf_has_mp.end(), 0);
    }
    return AFV_OK;
}

// afv_table_broadcast: the root's camera, poses and plane flags in one image, then the plane
int afv_kffuse_broadcast(afv_comm *m, afv_table *t, int root) {
    afv_ctx *c = t->c;
    kf_ensure_host(t);
    const bool is_root = afv_comm_rank(m) == root;
    const size_t ns = (size_t)t->nsets;
    const size_t bytes = align_up(8 + sizeof(afv_table_camera) + 2 * ns, 16) + ns * sizeof(KfPose);
    std::vector<uint8_t> img(bytes, 0);
    const size_t o_cam = 8, o_flags = o_cam + sizeof(afv_table_camera), o_pose = align_up(o_flags + 2 * ns, 16);
    if (is_root) {
        img[0] = t->has_camera;
        img[1] = t->d_mp != nullptr;
        std::memcpy(img.data() + o_cam, &t->cam, sizeof(t->cam));
        std::memcpy(img.data() + o_flags, t->kf_has_pose.data(), ns);
        std::memcpy(img.data() + o_flags + ns, t->kf_has_mp.data(), ns);
        std::memcpy(img.data() + o_pose, t->kf_pose.data(), ns * sizeof(KfPose));
    }
    uint8_t *d_img = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&d_img), bytes));
    struct Free { void *p; ~Free() { (void)hipFree(p); } } free_img{d_img};
    if (is_root) HIPCHK(c, hipMemcpyAsync(d_img, img.data(), bytes, hipMemcpyHostToDevice, c->stream));
    int rc = afv_comm_broadcast(m, d_img, bytes, root, c->stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(img.data(), d_img, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (img[1]) {
        rc = kf_ensure_plane(t);
        if (rc) return rc;
        rc = afv_comm_broadcast(m, t->d_mp, ns * t->cap * sizeof(int32_t), root, c->stream);
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (is_root) return AFV_OK;
    t->has_camera = img[0] != 0;
    std::memcpy(&t->cam, img.data() + o_cam, sizeof(t->cam));
    std::memcpy(t->kf_has_pose.data(), img.data() + o_flags, ns);
    std::memcpy(t->kf_has_mp.data(), img.data() + o_flags + ns, ns);
    std::memcpy(t->kf_pose.data(), img.data() + o_pose, ns * sizeof(KfPose));
    if (!img[1]) std::fill(t->kf_has_mp.begin(), t->kf_has_mp.end(), 0);
    std::fill(t->kf_grid_ok.begin(), t->kf_grid_ok.end(), 0);
    return AFV_OK;
}

extern "C" int afv_table_set_camera(afv_table *t, const afv_table_camera *caller) {
    if (!t || !caller) return AFV_EINVAL;
    const uint32_t ss = caller->struct_size;
    if (ss < sizeof(afv_table_camera) || ss > 4 * sizeof(afv_table_camera) || (ss & 3)) return AFV_EINVAL;
    afv_table_camera cam;
    std::memcpy(&cam, caller, sizeof(cam));
    cam.struct_size = (uint32_t)sizeof(cam);
    if (cam.grid_cols < 1 || cam.grid_rows < 1 || (long)cam.grid_cols * cam.grid_rows > 8192) return AFV_EINVAL;
    const float vals[6] = {cam.min_x, cam.max_x, cam.min_y, cam.max_y, cam.grid_inv_w, cam.grid_inv_h};
    for (float v : vals)
        if (!std::isfinite(v)) return AFV_EINVAL;
    afv_ctx *c = t->c;
    if (afv_frame_grid_lds(cam.grid_cols, cam.grid_rows, t->cap) > (size_t)c->frame_lds_max) {
        c->last_error = "afv_table_set_camera: the grid of a slot does not fit the LDS of one workgroup (cells x features too large)";
        return AFV_EUNSUPPORTED;
    }
    return guarded(c, [&]() -> int {
        kf_ensure_host(t);
        t->cam = cam;
        t->has_camera = true;
        afv_kffuse_grid_stale(t, -1);
        return AFV_OK;
    });
}

extern "C" int afv_table_set_pose(afv_table *t, int slot, const float *Rcw, const float *tcw, const float *Ow, float fx, float fy, float cx, float cy,
                                  float mbf) {
    if (!t || slot < 0 || slot >= t->nsets || !Rcw || !tcw || !Ow) return AFV_EINVAL;
    return guarded(t->c, [&]() -> int {
        kf_ensure_host(t);
        KfPose &p = t->kf_pose[(size_t)slot];
        std::memcpy(p.R, Rcw, sizeof(p.R));
        std::memcpy(p.t, tcw, sizeof(p.t));
        std::memcpy(p.Ow, Ow, sizeof(p.Ow));
        p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy; p.mbf = mbf;
        t->kf_has_pose[(size_t)slot] = 1;
        return AFV_OK;
    });
}

extern "C" int afv_table_set_map_points(afv_table *t, int slot, const int32_t *ids) {
    if (!t || slot < 0 || slot >= t->nsets) return AFV_EINVAL;
    const int n = t->h_n[(size_t)slot];
    if (n > 0 && !ids) return AFV_EINVAL;
    for (int i = 0; i < n; ++i)
        if (ids[i] < -1) return AFV_EINVAL;
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        kf_ensure_host(t);
        const int rc = kf_ensure_plane(t);
        if (rc) return rc;
        if (n > 0) HIPCHK(c, hipMemcpy(t->d_mp + (size_t)slot * t->cap, ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
        t->kf_has_mp[(size_t)slot] = 1;
        return AFV_OK;
    });
}

extern "C" int afv_table_get_map_points(afv_table *t, int slot, int32_t *ids) {
    if (!t || slot < 0 || slot >= t->nsets) return AFV_EINVAL;
    if (t->kf_pose.empty() || !t->kf_has_mp[(size_t)slot] || !t->d_mp) return AFV_EINVAL;
    const int n = t->h_n[(size_t)slot];
    if (n > 0 && !ids) return AFV_EINVAL;
    afv_ctx *c = t->c;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n > 0) HIPCHK(c, hipMemcpy(ids, t->d_mp + (size_t)slot * t->cap, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return AFV_OK;
}

// everything the header promises to refuse before a launch
static int kf_check(const afv_table *t, const afv_points *p, const std::vector<afv_table_fuse_job> &J) {
    if (p->c != t->c) return AFV_EINVAL;
    if (p->float_dim != t->float_dim || p->desc_bytes != t->desc_bytes || p->words != t->words) return AFV_EUNSUPPORTED;
    if (!t->has_camera) return AFV_EINVAL;
    size_t total = 0;
    for (const afv_table_fuse_job &j : J) {
        const int s = j.slot;
        if (s < 0 || s >= t->nsets) return AFV_EINVAL;
        if (!t->has_geo[(size_t)s] || !t->has_scale[(size_t)s] || !t->d_geo || !t->d_scale) return AFV_EINVAL;
        if (j.use_inf_gate != 0 && j.use_inf_gate != 1) return AFV_EINVAL;
        if (j.use_inf_gate && (!t->has_inf[(size_t)s] || !t->d_inf)) return AFV_EINVAL;
        if (t->kf_pose.empty() || !t->kf_has_mp[(size_t)s] || !t->d_mp) return AFV_EINVAL;
        if (!t->kf_has_pose[(size_t)s]) return AFV_EINVAL;  // (a pose_override replaces R, t and Ow; the intrinsics are always the slot's)
        if (j.nq < 0 || j.nq > 65535 || (j.nq > 0 && !j.ids)) return AFV_EINVAL;
        total += (size_t)j.nq;
        if (total > AFV_KFFUSE_MAX_QUERIES) return AFV_EINVAL;
        for (int q = 0; q < j.nq; ++q)
            if (j.ids[q] < -1 || j.ids[q] >= p->cap) return AFV_EINVAL;
    }
    return AFV_OK;
}

extern "C" int afv_table_fuse_points(afv_table *t, afv_points *points, const afv_table_fuse_job *jobs, int nt, int32_t *best, int32_t *occupant,
                                     uint8_t *status, int32_t *nfused) {
    if (!t || !points || nt < 0 || nt > AFV_KFFUSE_MAX_TARGETS) return AFV_EINVAL;
    if (!afv_points_is_live(points)) return AFV_EINVAL;
    if (nt == 0) return AFV_OK;
    if (!jobs || !best || !occupant || !status || !nfused) return AFV_EINVAL;
    afv_ctx *c = t->c;
    return guarded(c, [&]() -> int {
        std::vector<afv_table_fuse_job> J;
        if (!afv_load_jobs(jobs, nt, sizeof(afv_table_fuse_job), J)) return AFV_EINVAL;
        int rc = kf_check(t, points, J);
        if (rc) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        rc = kf_ensure_grid(t);
        if (rc) return rc;
        const size_t plane = (size_t)t->nsets * t->cap, pitch = (size_t)t->words * 4;
        const int cells = t->cam.grid_cols * t->cam.grid_rows;
        // 1. the layout: id lists, the records, then device-only scratch and the results
        Blob b(c);
        std::vector<IdList> lists;
        std::vector<int> list_of((size_t)nt, -1), first_of_list;
        std::vector<int> stale;  // the targets whose grid has to be built, each once
        size_t total = 0;
        int max_nq = 0;
        for (int i = 0; i < nt; ++i) {
            const afv_table_fuse_job &j = J[(size_t)i];
            total += (size_t)j.nq;
            max_nq = std::max(max_nq, j.nq);
            if (!t->kf_grid_ok[(size_t)j.slot] && std::find(stale.begin(), stale.end(), j.slot) == stale.end()) stale.push_back(j.slot);
            if (j.nq == 0) continue;
            for (size_t l = 0; l < lists.size(); ++l)
                if (lists[l].ids == j.ids && lists[l].nq == j.nq) list_of[(size_t)i] = (int)l;
            if (list_of[(size_t)i] < 0) {
                list_of[(size_t)i] = (int)lists.size();
                first_of_list.push_back(i);
                lists.push_back(IdList{j.ids, j.nq, b.put(j.ids, (size_t)j.nq * 4), 0});
            }
        }
        if (total == 0) {
            std::fill(nfused, nfused + nt, 0);
            return AFV_OK;
        }
        const size_t kf_off = b.reserve((size_t)nt * sizeof(DevKfFuseJob));
        const size_t pj_off = b.reserve((size_t)nt * sizeof(DevProjJob));
        const size_t gj_off = b.reserve(std::max<size_t>(stale.size(), 1) * sizeof(DevGridJob));
        const size_t in_bytes = b.h.size();
        for (IdList &L : lists) L.rows_off = b.reserve_scratch((size_t)L.nq * pitch);
        std::vector<size_t> q_off((size_t)nt, 0), v_off((size_t)nt, 0);
        for (int i = 0; i < nt; ++i) {
            const size_t nq1 = (size_t)std::max(J[(size_t)i].nq, 1);
            q_off[(size_t)i] = b.reserve_scratch(6 * align_up(nq1 * 4, 16));
            v_off[(size_t)i] = b.reserve_scratch(nq1);
        }
        const size_t best_off = b.reserve_scratch(total * 4), occ_off = b.reserve_scratch(total * 4), st_off = b.reserve_scratch(total);
        rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        // 2. the records, against the device buffer as it stands now
        uint8_t *B = c->d_match, *H = b.h.data();
        size_t acc = 0;
        for (int i = 0; i < nt; ++i) {
            const afv_table_fuse_job &j = J[(size_t)i];
            const size_t s = (size_t)j.slot, row0 = s * t->cap;
            const size_t nq1 = (size_t)std::max(j.nq, 1), fstride = align_up(nq1 * 4, 16);
            const IdList *L = j.nq > 0 ? &lists[(size_t)list_of[(size_t)i]] : nullptr;
            DevKfFuseJob &K = at<DevKfFuseJob>(H, kf_off)[i];
            K = DevKfFuseJob{};
            const KfPose &P = t->kf_pose[s];
            if (j.pose_override) {  // the decomposed Scw of Fuse no. 2; the intrinsics stay the slot's
                std::memcpy(K.R, j.pose_override->R, sizeof(K.R));
                std::memcpy(K.t, j.pose_override->t, sizeof(K.t));
                std::memcpy(K.Ow, j.pose_override->Ow, sizeof(K.Ow));
            } else {
                std::memcpy(K.R, P.R, sizeof(K.R));
                std::memcpy(K.t, P.t, sizeof(K.t));
                std::memcpy(K.Ow, P.Ow, sizeof(K.Ow));
            }
            K.fx = P.fx; K.fy = P.fy; K.cx = P.cx; K.cy = P.cy; K.mbf = P.mbf;
            K.min_x = t->cam.min_x; K.max_x = t->cam.max_x; K.min_y = t->cam.min_y; K.max_y = t->cam.max_y;
            K.rs_th = j.radius_scale * j.radius_th;  // FeatureMatcher.cc:91: the first product of the radius, as fill_points_job makes it
            K.cos_limit = 0.0f;
            K.tol = c->p.scale_factor;               // Frame.cc:73
            K.ids = L ? at<const int>(B, L->ids_off) : nullptr;
            K.nq = j.nq;
            K.n = t->h_n[s];
            K.plane = t->d_mp + row0;
            float *qf = at<float>(B, q_off[(size_t)i]);
            K.qu = qf; K.qv = qf + fstride / 4; K.qr = qf + 2 * (fstride / 4); K.qmin = qf + 3 * (fstride / 4); K.qmax = qf + 4 * (fstride / 4);
            K.q_ur = qf + 5 * (fstride / 4);
            K.qvalid = B + v_off[(size_t)i];
            K.status = B + st_off + acc;
            K.qd = (L && first_of_list[(size_t)list_of[(size_t)i]] == i) ? at<uint4>(B, L->rows_off) : nullptr;
            K.best = at<const int>(B, best_off + acc * 4);
            K.occupant = at<int>(B, occ_off + acc * 4);
            DevProjJob &D = at<DevProjJob>(H, pj_off)[i];
            D = DevProjJob{};
            D.fdesc = reinterpret_cast<const uint32_t *>(t->d_desc + row0 * pitch);
            D.n = K.n; D.words = t->float_dim ? 0 : t->words; D.fdim = t->float_dim;
            D.x = t->d_geo + row0; D.y = t->d_geo + plane + row0; D.u_right = t->d_geo + 3 * plane + row0;
            D.size = t->d_scale + row0;
            D.inf = j.use_inf_gate ? t->d_inf + row0 : nullptr;  // the 5.99 / 7.8 gates of Fuse no. 1
            D.min_x = t->cam.min_x; D.min_y = t->cam.min_y; D.inv_w = t->cam.grid_inv_w; D.inv_h = t->cam.grid_inv_h;
            D.cols = t->cam.grid_cols; D.rows = t->cam.grid_rows;
            D.cell_ptr = t->d_kf_cell_ptr + s * ((size_t)cells + 1);
            D.cell_ent = t->d_kf_cell_ent + row0;
            D.nq = j.nq;
            D.qdesc = L ? at<const uint32_t>(B, L->rows_off) : nullptr;
            D.qvalid = K.qvalid;
            D.qu = K.qu; D.qv = K.qv; D.qr = K.qr; D.qmin = K.qmin; D.qmax = K.qmax; D.q_ur = K.q_ur;
            D.th = j.th_low; D.tol = K.tol; D.inv_tol = 1.0f / K.tol;
            D.assign = at<int>(B, best_off + acc * 4);
            acc += (size_t)j.nq;
        }
        for (size_t k = 0; k < stale.size(); ++k) {
            const size_t s = (size_t)stale[k], row0 = s * t->cap;
            DevGridJob &g = at<DevGridJob>(H, gj_off)[k];
            g = DevGridJob{};
            g.n = t->h_n[s]; g.cap = t->cap;
            g.x = t->d_geo + row0; g.y = t->d_geo + plane + row0; g.size = t->d_scale + row0;
            g.min_x = t->cam.min_x; g.min_y = t->cam.min_y; g.inv_w = t->cam.grid_inv_w; g.inv_h = t->cam.grid_inv_h;
            g.cols = t->cam.grid_cols; g.rows = t->cam.grid_rows;
            g.cell_ptr = t->d_kf_cell_ptr + s * ((size_t)cells + 1);
            g.cell_ent = t->d_kf_cell_ent + row0;
        }
        // 3. one upload, the grids of the stale targets, geometry and membership, the search, the occupants; one wait
        HIPCHK(c, b.upload(in_bytes));
        if (!stale.empty()) afv_launch_frame_grid(at<const DevGridJob>(B, gj_off), (int)stale.size(), afv_frame_grid_lds(t->cam.grid_cols, t->cam.grid_rows, t->cap), c->stream);
        const DevKfFuseJob *kj = at<const DevKfFuseJob>(B, kf_off);
        afv_launch_kffuse_project(&points->P, kj, nt, max_nq, c->stream);
        afv_launch_match_fuse(at<const DevProjJob>(B, pj_off), nt, max_nq, nullptr, c->stream);
        afv_launch_kffuse_finish(&points->P, kj, nt, max_nq, c->stream);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            c->last_error = std::string("afv_table_fuse_points launch: ") + hipGetErrorString(e);
            return AFV_EHIP;
        }
        HIPCHK(c, b.fetch(best, best_off, total * 4, c->stream));
        HIPCHK(c, b.fetch(occupant, occ_off, total * 4, c->stream));
        HIPCHK(c, b.fetch(status, st_off, total, c->stream));
        HIPCHK(c, b.wait());
        for (int s : stale) t->kf_grid_ok[(size_t)s] = 1;
        size_t at_q = 0;
        for (int i = 0; i < nt; ++i) {
            int n = 0;
            for (int q = 0; q < J[(size_t)i].nq; ++q) n += status[at_q + q] >= 4;
            nfused[i] = n;
            at_q += (size_t)J[(size_t)i].nq;
        }
        return AFV_OK;
    });
}
