// afv_project.hip — host side of the projection-guided searches: SearchByProjection in its flavours, Fuse, SearchBySim3
// and SearchForInitialization.  No kernel lives here (k_project.hip, k_frame.hip, k_points.hip).
// One runner, afv_project_run, stages, launches and collects for every route: the host-array entry points below (afv_match_projection /
// _fuse / _initialization / _sim3), the searches against a resident frame (afv_frame.hip) and the searches through map-point ids
// (afv_points.hip).  A route describes each job once as a ProjJobSpec (afv_runtime.h) and decides there where every array lives; the runner
// reads that description and never asks a second time.  The grid of Frame::AssignFeaturesToGrid is built ON THE DEVICE on every route
// (k_frame_grid): a host-array side uploads x / y / size and runs the same kernel a resident frame ran when it was extracted.
#include "afv_runtime.h"

namespace {

// how a call runs: the ordered engine (wg_lds != 0: the workgroup fixed point with that much dynamic LDS), where results and inputs live
struct Route {
    size_t wg_lds = 0;
    bool zero_copy = false, zero_copy_in = false, ticket = false;
};
// what staging leaves behind for the launches and the collection
struct Staged {
    std::vector<DevProjJob> rec;                     // the search jobs, as they were copied into the image at jobs_off
    size_t jobs_off = 0, gjobs_off = 0, nm_off = 0;  // the records the kernels read: search jobs, grid jobs (staged feature sides), counts
    size_t in_bytes = 0;                            // what the upload covers: inputs and records
    size_t out_off = 0, total_out = 0;
    size_t in_view_off = 0, count_off = 0;          // POINT_IDS: qvalid and the in-view count k_points_project leaves
    const int *ref_slot = nullptr, *ref_idx = nullptr;  // TABLE_ROWS: the staged (slot, idx) the gather reads
    int max_nq = 0;
    size_t grid_lds = 0;
};

// 1. what is refused before anything touches the device
int check_specs(const ProjJobSpec *specs, int njobs, int kind) {
    for (int i = 0; i < njobs; ++i) {
        const ProjSide &f = specs[i].f;
        const ProjQueries &q = specs[i].q;
        if ((f.on_device || q.from != ProjQueries::HOST_ROWS || q.valid_on_device || q.angle_on_device) && njobs != 1) return AFV_EINVAL;
        if (f.n < 0 || f.n > AFV_MAX_SIDE || q.nq < 0 || q.nq > 65535) return AFV_EINVAL;
        if (f.fdim != 0) {  // float descriptors (L2^2): rows of fdim floats
            if (f.fdim < 4 || f.fdim > 1024 || (f.fdim & 3)) return AFV_EINVAL;
        } else if (f.desc_bytes < 1 || f.desc_bytes > 64) {
            return AFV_EINVAL;
        }
        if (f.grid_cols < 1 || f.grid_rows < 1 || (long)f.grid_cols * f.grid_rows > 8192) return AFV_EINVAL;
        if (f.n > 0 && (!f.desc || !f.x || !f.y || !f.size)) return AFV_EINVAL;
        // the arrays the query side's source must bring
        if (q.nq > 0 && q.from == ProjQueries::POINT_IDS && (!q.points || !q.points->ids)) return AFV_EINVAL;
        if (q.nq > 0 && q.from != ProjQueries::POINT_IDS &&
            (!(q.from == ProjQueries::TABLE_ROWS ? static_cast<const void *>(q.ref_table) : q.desc) || !q.u || !q.v || !q.r || !q.min_size || !q.max_size))
            return AFV_EINVAL;
        const bool no_angles = (f.n > 0 && !f.angle) || (q.nq > 0 && !q.angle);
        if (kind == AFV_KIND_INIT && specs[i].check_ori && no_angles) return AFV_EINVAL;
        if (kind == AFV_KIND_PROJ && specs[i].mode != AFV_PROJ_LOCALMAP && specs[i].mode != AFV_PROJ_LASTFRAME) return AFV_EINVAL;
        if (kind == AFV_KIND_PROJ && specs[i].mode == AFV_PROJ_LASTFRAME && specs[i].check_ori && no_angles) return AFV_EINVAL;
        // stereo frames: the queries' right-image coordinate (and, for the projection searches, their gate) come with mvuRight
        if (specs[i].stereo && kind != AFV_KIND_INIT && q.nq > 0 && q.from != ProjQueries::POINT_IDS && (!q.ur || (kind == AFV_KIND_PROJ && !q.er_max)))
            return AFV_EINVAL;
    }
    return AFV_OK;
}
// ... and once the device is set: the row width both sides share, and rows by reference (checked here, gathered on the device)
int check_rows(const afv_ctx *c, const ProjJobSpec *specs, int njobs) {
    for (int i = 0; i < njobs; ++i) {
        const ProjSide &f = specs[i].f;
        const ProjQueries &q = specs[i].q;
        if (f.words != (f.fdim ? f.fdim : (f.desc_bytes <= 32 ? 8 : 16))) return AFV_EINVAL;  // dwords of one row
        if (q.from != ProjQueries::TABLE_ROWS) continue;
        const afv_table *qt = q.ref_table;
        if (qt->c != c || !q.ref_slot || !q.ref_idx || f.fdim != qt->float_dim || f.desc_bytes != qt->desc_bytes) return AFV_EINVAL;
        for (int k = 0; k < q.nq; ++k) {
            const int sl = q.ref_slot[k];
            if (sl < 0 || sl >= qt->nsets || q.ref_idx[k] < 0 || q.ref_idx[k] >= qt->h_n[sl]) return AFV_EINVAL;
        }
    }
    return AFV_OK;
}

// 2. the route: plain values in, no HIP call.  wg_lds_need: what the fixed point of the largest job takes (afv_project_wg_lds);
// one_resident_job: ONE job against a feature side that is already on the device; occupancy_mask: that job brings one and the kind reads it
Route choose_route(int kind, bool any_float, int max_nq, size_t wg_lds_need, int proj_engine, int proj_wg_lds_max, int proj_fuse, bool stage_pinned,
                   bool one_resident_job, bool occupancy_mask) {
    const bool fuse = kind == AFV_KIND_FUSE;
    Route r;
    // ordered phase: the workgroup fixed point when the largest job's tables fit the LDS it may use
    // (float descriptors: the projection searches' fixed point carries float distances; SearchForInitialization's packs them in 16 bits and
    // float jobs take its ordered walk)
    if (!fuse && !(any_float && kind == AFV_KIND_INIT) && proj_engine != 0 && proj_wg_lds_max > 0 && (kind != AFV_KIND_INIT || max_nq <= 32767))
        r.wg_lds = wg_lds_need > (size_t)proj_wg_lds_max ? 0 : wg_lds_need;
    // results straight into the pinned arena (device-visible host memory) when the kernels write them once and never read them back
    r.zero_copy = stage_pinned && (fuse || r.wg_lds != 0);
    // ... and, for ONE job against a resident frame, the inputs straight out of it: the job record is the kernel argument, the queries
    // (a few KB per array, read once by the ranking kernel) come over the link without a copy-engine hop ahead of the launch
    // (not with an occupancy mask: that one is gathered per candidate, which belongs in device memory)
    // (nor with float rows: a query row is 4 * dim bytes and is read once per CANDIDATE - that belongs in device memory too)
    r.zero_copy_in = r.zero_copy && one_resident_job && !any_float && !occupancy_mask;
    // one launch for ranking + ordered phase: the projection searches (a few candidates per query).  SearchForInitialization keeps two: its
    // ranking walks 100-pixel windows (hundreds of cells per query) and is better off on 250 four-wave workgroups than on 63 sixteen-wave
    // ones (measured: 59.6 us against 72.5 host to host)
    r.ticket = r.zero_copy_in && r.wg_lds && proj_fuse && kind == AFV_KIND_PROJ && !any_float;  // (the one-launch kernel is binary-only)
    return r;
}

template <class T>
T *at(uint8_t *base, size_t off) { return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(base) + off); }  // (integers: a base may still be null, see afv_project_run)
size_t put_rows(Blob &b, const void *rows, int n, const ProjSide &f) {  // descriptor rows of the feature side's kind, host -> device pitch
    return f.fdim ? b.put(rows, (size_t)n * f.fdim * 4) : put_desc(b, static_cast<const uint8_t *>(rows), n, f.desc_bytes, f.words);
}

// 3 + 4. the staging blob - every job's inputs, then the records, then device-only scratch - and, array by array as it is placed, the records:
// an array staged from the host is at its offset from IN (the device blob B, or the pinned image H itself on the zero-copy route), what a
// kernel of this call makes (the grid, gathered rows, the queries of k_points_project) at its offset from B, results at theirs from RES,
// and an array that is already on the device is the pointer in the spec.  H and B are the arena and the buffer as the caller found them
void stage(afv_ctx *c, Blob &b, const ProjJobSpec *specs, int njobs, int kind, const Route &route, uint8_t *H, uint8_t *B, Staged &S) {
    const bool fuse = kind == AFV_KIND_FUSE, per_query = kind != AFV_KIND_PROJ;
    const bool staged_side = !specs[0].f.on_device;  // (a side on the device comes alone)
    uint8_t *IN = route.zero_copy_in ? H : B, *RES = route.zero_copy ? H : B;
    S = Staged{};
    S.rec = std::vector<DevProjJob>((size_t)njobs);
    for (int i = 0; i < njobs; ++i) {
        const ProjSide &f = specs[i].f;
        const ProjQueries &q = specs[i].q;
        DevProjJob &d = S.rec[i];
        const bool stereo = specs[i].stereo && kind != AFV_KIND_INIT, gate = stereo && kind == AFV_KIND_PROJ;
        const bool ids = q.from == ProjQueries::POINT_IDS;
        const size_t n4 = (size_t)f.n * 4, nq4 = (size_t)q.nq * 4;
        d.n = f.n; d.words = f.fdim ? 0 : f.words; d.fdim = f.fdim;
        if (staged_side) {
            d.fdesc = at<uint32_t>(B, put_rows(b, f.desc, f.n, f));
            d.x = at<float>(B, b.put(f.x, n4)); d.y = at<float>(B, b.put(f.y, n4)); d.size = at<float>(B, b.put(f.size, n4));
            if (f.angle) d.angle = at<float>(B, b.put(f.angle, n4));
            if (fuse && f.inf) d.inf = at<float>(B, b.put(f.inf, n4));
            if (stereo) d.u_right = at<float>(B, b.put(f.u_right, n4));
            S.grid_lds = std::max(S.grid_lds, afv_frame_grid_lds(f.grid_cols, f.grid_rows, std::max(f.n, 1)));
        } else {
            d.fdesc = static_cast<const uint32_t *>(f.desc);
            d.x = f.x; d.y = f.y; d.size = f.size; d.angle = f.angle;
            d.inf = fuse ? f.inf : nullptr;
            d.u_right = stereo ? f.u_right : nullptr;
            d.cell_ptr = f.cell_ptr; d.cell_ent = f.cell_ent;
        }
        if (f.occupied && kind != AFV_KIND_INIT) d.occupied = at<uint8_t>(IN, b.put(f.occupied, (size_t)f.n));
        d.min_x = f.min_x; d.min_y = f.min_y; d.inv_w = f.inv_w; d.inv_h = f.inv_h; d.cols = f.grid_cols; d.rows = f.grid_rows;
        d.nq = q.nq;
        if (ids) {
            q.points->job.ids = at<int>(IN, b.put(q.points->ids, nq4));
        } else {
            if (stereo) d.q_ur = at<float>(IN, b.put(q.ur, nq4));
            if (gate) d.q_er = at<float>(IN, b.put(q.er_max, nq4));
        }
        if (q.from == ProjQueries::TABLE_ROWS) {
            S.ref_slot = at<int>(IN, b.put(q.ref_slot, nq4));
            S.ref_idx = at<int>(IN, b.put(q.ref_idx, nq4));
        } else if (q.from == ProjQueries::HOST_ROWS) {
            d.qdesc = at<uint32_t>(IN, put_rows(b, q.desc, q.nq, f));
        } else if (q.from == ProjQueries::DEVICE_ROWS) {
            d.qdesc = static_cast<const uint32_t *>(q.desc);
        }
        d.qvalid = (q.valid && !q.valid_on_device) ? at<uint8_t>(IN, b.put(q.valid, (size_t)q.nq)) : q.valid;
        if (!ids) {
            d.qu = at<float>(IN, b.put(q.u, nq4)); d.qv = at<float>(IN, b.put(q.v, nq4)); d.qr = at<float>(IN, b.put(q.r, nq4));
            d.qmin = at<float>(IN, b.put(q.min_size, nq4)); d.qmax = at<float>(IN, b.put(q.max_size, nq4));
        }
        d.qangle = (q.angle && !q.angle_on_device) ? at<float>(IN, b.put(q.angle, nq4)) : q.angle;
        if (q.occupies) d.qocc = at<uint8_t>(IN, b.put(q.occupies, (size_t)q.nq));
        d.th = specs[i].th; d.ratio = specs[i].ratio; d.tol = specs[i].tol; d.inv_tol = specs[i].inv_tol;
        d.check_ori = specs[i].check_ori != 0; d.mode = specs[i].mode;
        d.pass_cap = afv_debug_pass_cap;
        d.stereo_gate = gate ? 1 : 0;
        S.total_out += (size_t)(per_query ? q.nq : f.n);
        S.max_nq = std::max(S.max_nq, q.nq);
    }
    // records the kernels read: the search jobs and, for staged feature sides, the grid jobs (uploaded with the inputs)
    S.jobs_off = b.reserve((size_t)njobs * sizeof(DevProjJob));
    if (staged_side) S.gjobs_off = b.reserve((size_t)njobs * sizeof(DevGridJob));
    S.nm_off = b.reserve((size_t)njobs * 4);
    S.in_bytes = b.h.size();
    for (int i = 0; i < njobs; ++i) {  // device-only scratch
        const ProjSide &f = specs[i].f;
        const ProjQueries &q = specs[i].q;
        DevProjJob &d = S.rec[i];
        const size_t nq1 = (size_t)std::max(q.nq, 1), nq4 = nq1 * 4;
        d.keys = at<unsigned long long>(B, b.reserve_scratch(nq1 * 64));  // 64-byte record / 8 keys per query
        d.ncand = at<int>(B, b.reserve_scratch(nq4));
        d.orilist = at<int>(B, b.reserve_scratch(nq1 * 8));
        if (q.from == ProjQueries::TABLE_ROWS) d.qdesc = at<uint32_t>(B, b.reserve_scratch(nq4 * q.ref_table->words));  // what k_frame_gather writes
        if (q.from == ProjQueries::POINT_IDS) {  // what k_points_project writes: the whole query side
            DevPointsJob &pj = q.points->job;
            pj.nq = q.nq;
            d.qu = pj.qu = at<float>(B, b.reserve_scratch(nq4)); d.qv = pj.qv = at<float>(B, b.reserve_scratch(nq4));
            d.qr = pj.qr = at<float>(B, b.reserve_scratch(nq4)); d.qmin = pj.qmin = at<float>(B, b.reserve_scratch(nq4));
            d.qmax = pj.qmax = at<float>(B, b.reserve_scratch(nq4));
            pj.q_ur = at<float>(B, b.reserve_scratch(nq4)); pj.q_er = at<float>(B, b.reserve_scratch(nq4));
            if (specs[i].stereo && kind != AFV_KIND_INIT) d.q_ur = pj.q_ur;
            if (d.stereo_gate) d.q_er = pj.q_er;
            S.in_view_off = b.reserve_scratch(nq1);
            d.qvalid = pj.qvalid = at<uint8_t>(B, S.in_view_off);
            d.qocc = pj.qocc = at<uint8_t>(B, b.reserve_scratch(nq1));
            pj.qd = at<uint4>(B, b.reserve_scratch(nq4 * f.words));
            d.qdesc = reinterpret_cast<const uint32_t *>(pj.qd);
            S.count_off = b.reserve_scratch(16);
            pj.count = c->d_points_count;
            pj.ticket = c->d_points_count + 1;
            pj.count_out = at<int>(B, S.count_off);
            pj.o_size = pj.o_sigma = pj.o_cos = nullptr;
        }
        if (staged_side) {  // the grid k_frame_grid builds behind the upload, and its job
            d.cell_ptr = at<int>(B, b.reserve_scratch(((size_t)f.grid_cols * f.grid_rows + 1) * 4));
            d.cell_ent = at<int4>(B, b.reserve_scratch((size_t)std::max(f.n, 1) * 16));
            DevGridJob &g = at<DevGridJob>(b.h.data(), S.gjobs_off)[i];
            g = DevGridJob{};
            g.n = f.n; g.cap = std::max(f.n, 1);
            g.x = const_cast<float *>(d.x); g.y = const_cast<float *>(d.y); g.size = const_cast<float *>(d.size);
            g.min_x = f.min_x; g.min_y = f.min_y; g.inv_w = f.inv_w; g.inv_h = f.inv_h; g.cols = f.grid_cols; g.rows = f.grid_rows;
            g.cell_ptr = const_cast<int *>(d.cell_ptr); g.cell_ent = const_cast<int4 *>(d.cell_ent);
        }
    }
    S.out_off = b.reserve_scratch(std::max<size_t>(S.total_out, 1) * 4);
    size_t acc = 0;
    for (int i = 0; i < njobs; ++i) {
        S.rec[i].assign = at<int>(RES, S.out_off + acc * 4);
        S.rec[i].nmatches = at<int>(RES, S.nm_off + (size_t)i * 4);
        acc += (size_t)(per_query ? specs[i].q.nq : specs[i].f.n);
    }
    std::memcpy(b.h.data() + S.jobs_off, S.rec.data(), (size_t)njobs * sizeof(DevProjJob));
}

// 5. upload, the kernels that make inputs (grid, gather, k_points_project), the search
int launch(afv_ctx *c, Blob &b, const ProjJobSpec *specs, int njobs, int kind, const Staged &S, const Route &route) {
    uint8_t *B = c->d_match, *H = b.h.data();
    const ProjQueries &q0 = specs[0].q;  // (a query side with a device source comes alone)
    if (!route.zero_copy_in) HIPCHK(c, b.upload(S.in_bytes));
    if (!specs[0].f.on_device) {
        if (S.grid_lds > (size_t)c->frame_lds_max) {
            c->last_error = "projection search: the grid of the feature side does not fit the LDS of one workgroup (cells x features too large)";
            return AFV_EUNSUPPORTED;
        }
        afv_launch_frame_grid(at<const DevGridJob>(B, S.gjobs_off), njobs, S.grid_lds, c->stream);
    }
    if (q0.from == ProjQueries::TABLE_ROWS) {
        const afv_table *qt = q0.ref_table;
        afv_launch_frame_gather(qt->d_desc, qt->d_n, qt->nsets, qt->cap, S.ref_slot, S.ref_idx, q0.nq, const_cast<uint32_t *>(S.rec[0].qdesc), nullptr,
                                qt->words, c->stream);
    }
    if (q0.from == ProjQueries::POINT_IDS && q0.nq > 0) {  // geometry and descriptor gather: the one launch a search through ids adds
        afv_launch_points_project(&q0.points->job, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    const DevProjJob *dj = at<const DevProjJob>(B, S.jobs_off);
    const DevProjJob *one = route.zero_copy_in ? at<const DevProjJob>(H, S.jobs_off) : nullptr;
    int *ticket = route.ticket ? c->d_proj_ticket : nullptr;
    if (kind == AFV_KIND_FUSE) afv_launch_match_fuse(dj, njobs, S.max_nq, one, c->stream);
    else if (kind == AFV_KIND_INIT) afv_launch_match_init(dj, njobs, S.max_nq, route.wg_lds, one, ticket, c->stream);
    else afv_launch_match_projection(dj, njobs, S.max_nq, route.wg_lds, one, ticket, c->stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        if (ticket) (void)hipMemsetAsync(ticket, 0, sizeof(int), c->stream);  // a launch that did not go out must not leave the ticket armed
        c->last_error = std::string("projection search launch: ") + hipGetErrorString(e);
        return AFV_EHIP;
    }
    return AFV_OK;
}

// 6. results to the caller
int collect(afv_ctx *c, Blob &b, const ProjJobSpec *specs, int njobs, int kind, const Staged &S, const Route &route, int32_t *assign, int32_t *nmatches) {
    const bool fuse = kind == AFV_KIND_FUSE;
    const ProjQueries &q0 = specs[0].q;
    if (!route.zero_copy) {
        HIPCHK(c, b.fetch(assign, S.out_off, S.total_out * 4, c->stream));
        if (!fuse) HIPCHK(c, b.fetch(nmatches, S.nm_off, (size_t)njobs * 4, c->stream));
    }
    if (q0.from == ProjQueries::POINT_IDS) {
        PointQueries *pq = q0.points;
        pq->n_in_view = 0;
        if (q0.nq > 0) {
            if (pq->in_view) HIPCHK(c, b.fetch(pq->in_view, S.in_view_off, (size_t)q0.nq, c->stream));
            HIPCHK(c, b.fetch(&pq->n_in_view, S.count_off, 4, c->stream));
        }
    }
    HIPCHK(c, b.wait());
    if (route.zero_copy) {
        std::memcpy(assign, b.h.data() + S.out_off, S.total_out * 4);
        if (!fuse) std::memcpy(nmatches, b.h.data() + S.nm_off, (size_t)njobs * 4);
    }
    if (fuse) {  // independent queries: the count is just the number of hits
        size_t at_q = 0;
        for (int i = 0; i < njobs; ++i) {
            int found = 0;
            for (int k = 0; k < specs[i].q.nq; ++k) found += assign[at_q + k] >= 0;
            nmatches[i] = found;
            at_q += (size_t)specs[i].q.nq;
        }
        return AFV_OK;
    }
    for (int i = 0; i < njobs; ++i)
        if (nmatches[i] == AFV_PASS_GUARD) {  // the fixed point did not settle within its pass guard (never observed)
            c->last_error = "projection search: the fixed point hit its pass guard; afv_set_projection_resolve(ctx, 0) selects the ordered walk";
            return AFV_EHIP;
        }
    return AFV_OK;
}

}  // namespace

int afv_project_run(afv_ctx *c, const ProjJobSpec *specs, int njobs, int kind, int32_t *assign, int32_t *nmatches) {
    if (!c || !specs || njobs < 1 || !assign || !nmatches) return AFV_EINVAL;
    int rc = check_specs(specs, njobs, kind);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = check_rows(c, specs, njobs);
    if (rc) return rc;
    bool any_float = false;
    int max_nq = 0;
    for (int i = 0; i < njobs; ++i) {
        any_float = any_float || specs[i].f.fdim != 0;
        max_nq = std::max(max_nq, specs[i].q.nq);
    }
    size_t wg_lds_need = 0;
    for (int i = 0; i < njobs; ++i)
        wg_lds_need = std::max(wg_lds_need, afv_project_wg_lds(kind == AFV_KIND_INIT, specs[i].f.n, specs[i].q.nq, any_float ? 1 : 0));
    Blob b(c);
    Staged S;
    Route route;
    // The records hold addresses inside the pinned arena and the device buffer, both grow-only: staging writes them against the two as they
    // stand, and a call that outgrows either (a context's first, a larger one than any before) grows it and stages once more
    for (;;) {
        uint8_t *const H = c->h_stage, *const B = c->d_match;
        route = choose_route(kind, any_float, max_nq, wg_lds_need, c->proj_engine, c->proj_wg_lds_max, c->proj_fuse, c->stage_pinned,
                             specs[0].f.on_device && njobs == 1, specs[0].f.occupied && kind != AFV_KIND_INIT);
        b.h.n = 0;
        stage(c, b, specs, njobs, kind, route, H, B, S);
        if (c->h_stage == H && b.h.size() <= c->match_bytes) break;
        rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
    }
    rc = launch(c, b, specs, njobs, kind, S, route);
    if (rc) return rc;
    return collect(c, b, specs, njobs, kind, S, route, assign, nmatches);
}

// ---- the host-array entry points ----
// one afv_proj_job as a spec: both sides are host arrays
static ProjJobSpec spec_of(const afv_proj_job &j) {
    ProjJobSpec J;
    ProjSide &f = J.f;
    f.n = j.n; f.desc_bytes = j.desc_bytes; f.fdim = j.float_dim;
    f.words = j.float_dim ? j.float_dim : (j.desc_bytes <= 32 ? 8 : 16);
    f.desc = j.desc;
    f.x = j.x; f.y = j.y; f.size = j.size; f.angle = j.angle; f.inf = j.inf; f.u_right = j.u_right;
    f.min_x = j.min_x; f.min_y = j.min_y; f.inv_w = j.grid_inv_w; f.inv_h = j.grid_inv_h;
    f.grid_cols = j.grid_cols; f.grid_rows = j.grid_rows;
    afv_proj_host_fields(j, J);
    J.tol = j.size_tol; J.inv_tol = j.inv_size_tol;
    J.stereo = j.u_right != nullptr;
    return J;
}
// job arrays arrive with the layout the caller was compiled against (struct_size): bring them to the current one
static int proj_jobs_entry(afv_ctx *c, const afv_proj_job *jobs, int njobs, int32_t *out, int32_t *nm, int kind) {
    return guarded(c, [&]() -> int {
        std::vector<afv_proj_job> J;
        if (!afv_load_jobs(jobs, njobs, offsetof(afv_proj_job, u_right), J)) return AFV_EINVAL;
        std::vector<ProjJobSpec> S;
        S.reserve(J.size());
        for (const afv_proj_job &j : J) S.push_back(spec_of(j));
        return afv_project_run(c, S.data(), njobs, kind, out, nm);
    });
}
extern "C" int afv_match_projection(afv_ctx *c, const afv_proj_job *jobs, int njobs, int32_t *assign, int32_t *nmatches) {
    return proj_jobs_entry(c, jobs, njobs, assign, nmatches, AFV_KIND_PROJ);
}
extern "C" int afv_match_fuse(afv_ctx *c, const afv_proj_job *jobs, int njobs, int32_t *best, int32_t *nfound) {
    return proj_jobs_entry(c, jobs, njobs, best, nfound, AFV_KIND_FUSE);
}
extern "C" int afv_match_initialization(afv_ctx *c, const afv_proj_job *jobs, int njobs, int32_t *match12, int32_t *nmatches) {
    return proj_jobs_entry(c, jobs, njobs, match12, nmatches, AFV_KIND_INIT);
}
static int afv_match_sim3_impl(afv_ctx *c, const afv_proj_job *j12, const afv_proj_job *j21, int32_t *match12, int32_t *nfound) {
    if (!c || !j12 || !j21 || !match12 || !nfound) return AFV_EINVAL;
    std::vector<afv_proj_job> A, Bv;
    if (!afv_load_jobs(j12, 1, offsetof(afv_proj_job, u_right), A) || !afv_load_jobs(j21, 1, offsetof(afv_proj_job, u_right), Bv)) return AFV_EINVAL;
    if (A[0].nq != Bv[0].n || Bv[0].nq != A[0].n) return AFV_EINVAL;
    ProjJobSpec S[2] = {spec_of(A[0]), spec_of(Bv[0])};
    for (ProjJobSpec &J : S) {
        J.f.inf = nullptr;  // no reprojection gate in SearchBySim3
        J.stereo = false;   // ... and no stereo branch (FeatureMatcher.cc:1066-1287)
    }
    std::vector<int32_t> best((size_t)S[0].q.nq + (size_t)S[1].q.nq + 1);
    int32_t nf[2];
    const int rc = afv_project_run(c, S, 2, AFV_KIND_FUSE, best.data(), nf);
    if (rc) return rc;
    const int32_t *m1 = best.data(), *m2 = best.data() + S[0].q.nq;
    int found = 0;
    for (int i1 = 0; i1 < S[0].q.nq; ++i1) {  // FeatureMatcher.cc:1268-1284
        const int idx2 = m1[i1];
        const bool agree = idx2 >= 0 && m2[idx2] == i1;
        match12[i1] = agree ? idx2 : -1;
        found += agree;
    }
    *nfound = found;
    return AFV_OK;
}
extern "C" int afv_match_sim3(afv_ctx *c, const afv_proj_job *j12, const afv_proj_job *j21, int32_t *match12, int32_t *nfound) {
    return guarded(c, [&] { return afv_match_sim3_impl(c, j12, j21, match12, nfound); });
}
extern "C" int afv_set_projection_resolve(afv_ctx *c, int engine) {
    if (!c || engine < 0 || engine > 3) return AFV_EINVAL;
    c->proj_fuse = engine != 3;          // 3 = the fixed point as two launches (ranking, then ordered phase): the A / B of the one-launch form
    c->proj_engine = engine == 3 ? 1 : engine;
    return AFV_OK;
}
