// k_points.hip — the resident map-point store (include/afv_hip.h, "resident map points"; host side: afv_points.hip).
//
//   k_points_project  Frame::isInFrustum (Frame.cc:276-331) and the projections in front of SearchByProjection(cur, last)
//                     (FeatureMatcher.cc:1312-1351), the relocalisation search (:1425-1465) and Fuse (:811-858): a thread per query, the
//                     pose as kernel argument; writes the query arrays the projection searches read and gathers the descriptor rows
//   k_points_move     the setters / afv_points_get: n ids between packed host-order arrays and the planes
//   k_points_rows     descriptor rows of n ids: packed rows or rows of a keyframe table into the store, or out of it
//
// The arithmetic is the restatement's (tests/_points_ref.py), statement for statement: float, one rounding per operator (the build's
// -ffp-contract=off; hipcc's correctly rounded divide and square root), three-term sums as a0 + (a1 + a2).
#include "afv_device.h"
#include "afv_runtime.h"

#define PT_T 256

__device__ __forceinline__ float pt_sum3(float a0, float a1, float a2) { return a0 + (a1 + a2); }
__device__ __forceinline__ bool pt_finite(float v) { return __builtin_isfinite(v); }

// what the rule set `fv` makes of point `id` (set and not bad) seen by camera J: in view or not, and the query the searches read.
// CAM: DevPointsJob, or the record of a target keyframe (DevKfFuseJob) - the same field names, ONE text for every route
struct PtQuery {
    float u, v, ur, r, er, size, sigma, vcos, mn, mx;
};
template <class CAM>
__device__ __forceinline__ bool pt_project_one(const DevPointPlanes &P, const CAM &J, int fv, int id, float last_size, PtQuery &o) {
    bool ok = true;
    float u = 0.0f, v = 0.0f, ur = 0.0f, r = 0.0f, er = 0.0f, size = 0.0f, sigma = 0.0f, vcos = 0.0f, mn = 0.0f, mx = 0.0f;
    {
        const float X = P.pos[0][id], Y = P.pos[1][id], Z = P.pos[2][id];
        const float pcx = pt_sum3(J.R[0] * X, J.R[1] * Y, J.R[2] * Z) + J.t[0];
        const float pcy = pt_sum3(J.R[3] * X, J.R[4] * Y, J.R[5] * Z) + J.t[1];
        const float pcz = pt_sum3(J.R[6] * X, J.R[7] * Y, J.R[8] * Z) + J.t[2];
        if ((fv == AFV_PT_FRUSTUM || fv == AFV_PT_FUSE) && pcz < 0.0f) ok = false;  // Frame.cc:290, FeatureMatcher.cc:825
        const float invz = 1.0f / pcz;
        if (fv == AFV_PT_LASTFRAME && invz < 0.0f) ok = false;                        // :1329 (RELOC: no depth test)
        if (fv == AFV_PT_FUSE) {
            const float x = pcx * invz, y = pcy * invz;  // :829-833
            u = J.fx * x + J.cx;
            v = J.fy * y + J.cy;
            if (!(u >= J.min_x && u < J.max_x && v >= J.min_y && v < J.max_y)) ok = false;  // KeyFrame::IsInImage
        } else {
            u = (J.fx * pcx) * invz + J.cx;  // Frame.cc:295-296
            v = (J.fy * pcy) * invz + J.cy;
            if (u < J.min_x || u > J.max_x) ok = false;
            if (v < J.min_y || v > J.max_y) ok = false;
        }
        ur = u - J.mbf * invz;
        if (fv == AFV_PT_LASTFRAME) {
            size = last_size;  // :1341
        } else {
            const float p0 = X - J.Ow[0], p1 = Y - J.Ow[1], p2 = Z - J.Ow[2];
            const float dist = sqrtf(pt_sum3(p0 * p0, p1 * p1, p2 * p2));
            const float lo = 0.8f * P.min_d[id], hi = 1.2f * P.max_d[id];  // MapPoint.cc:420-430
            if (dist < lo || dist > hi) ok = false;
            if (fv != AFV_PT_RELOC) {
                const float dot = pt_sum3(p0 * P.normal[0][id], p1 * P.normal[1][id], p2 * P.normal[2][id]);
                if (fv == AFV_PT_FRUSTUM) {
                    vcos = dot / dist;
                    if (vcos < J.cos_limit) ok = false;
                } else if (dot < 0.5f * dist) {  // :853 in double, :351 / :1010 in float: 0.5 * dist is exact in both
                    ok = false;
                }
            }
            const float rd = P.ref_dist[id];
            size = (P.ref_size[id] * rd) / dist;    // MapPoint::PredictSize
            sigma = (P.ref_sigma[id] * rd) / dist;  // MapPoint::PredictSigma
        }
        if (fv == AFV_PT_FRUSTUM) {
            const float by_cos = (double)vcos > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos compares against a double literal
            r = (J.rs_th * by_cos) * size;                              // FeatureMatcher.cc:91
            er = r * sigma;                                             // :117
        } else {
            r = J.rs_th * size;
            er = r;  // :1371
        }
        mn = size / J.tol;
        mx = size * J.tol;
        if (!(pt_finite(u) && pt_finite(v) && pt_finite(r) && pt_finite(mn) && pt_finite(mx))) ok = false;  // D1
    }
    o.u = u; o.v = v; o.ur = ur; o.r = r; o.er = er; o.size = size; o.sigma = sigma; o.vcos = vcos; o.mn = mn; o.mx = mx;
    return ok;
}

__global__ __launch_bounds__(PT_T) void k_points_project(const DevPointsJob J) {
    __shared__ int s_id[PT_T];  // the point of an in-view query of this workgroup, -1 otherwise: what the gather below reads
    const int tid = threadIdx.x, q = blockIdx.x * PT_T + tid;
    const DevPointPlanes &P = J.P;
    bool ok = false;
    int id = -1;
    unsigned fl = 0;
    float u = 0.0f, v = 0.0f, ur = 0.0f, r = 0.0f, er = 0.0f, size = 0.0f, sigma = 0.0f, vcos = 0.0f, mn = 0.0f, mx = 0.0f;
    if (q < J.nq) {
        id = J.ids[q];
        if (id >= 0 && id < P.cap) fl = P.flags[id];
        else id = -1;
    }
    if ((fl & AFV_PTF_SET) && !(fl & AFV_PTF_BAD)) {
        PtQuery o;
        ok = pt_project_one(P, J, J.flavour, id, J.flavour == AFV_PT_LASTFRAME ? J.last_size[q] : 0.0f, o);
        u = o.u; v = o.v; ur = o.ur; r = o.r; er = o.er; size = o.size; sigma = o.sigma; vcos = o.vcos; mn = o.mn; mx = o.mx;
    }
    if (!ok) u = v = ur = r = er = size = sigma = vcos = mn = mx = 0.0f;
    if (q < J.nq) {
        J.qu[q] = u; J.qv[q] = v; J.qr[q] = r; J.qmin[q] = mn; J.qmax[q] = mx; J.q_ur[q] = ur; J.q_er[q] = er;
        J.qvalid[q] = ok ? 1 : 0;
        J.qocc[q] = (fl & AFV_PTF_OBSERVED) ? 1 : 0;
        if (J.o_size) J.o_size[q] = size;
        if (J.o_sigma) J.o_sigma[q] = sigma;
        if (J.o_cos) J.o_cos[q] = vcos;
    }
    const unsigned long long m = __ballot(ok);
    if ((tid & 63) == 0 && m) atomicAdd(J.count, __popcll(m));
    s_id[tid] = ok ? id : -1;
    __syncthreads();
    // the accumulator and the ticket are zero at rest (like the ticket of the one-launch search): the workgroup that draws the last
    // ticket takes the sum, hands it to the call and leaves both words zero for the next launch - no fill in front of the kernel.
    // Deliberately one fence per workgroup: the other wavefronts' adds to J.count are ordered before the barrier, the barrier before
    // thread 0's device-scope fence, and that fence before its ticket (cumulativity), so the last workgroup's exchange sees every add
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(J.ticket, 1) == (int)gridDim.x - 1) {
            __threadfence();
            *J.count_out = atomicExch(J.count, 0);
            atomicExch(J.ticket, 0);
        }
    }
    if (!J.qd) return;  // (uniform)
    // the rows of this workgroup's queries, a thread per 16 bytes; a query that is not in view gets a zero row
    const int quads = P.words >> 2;
    for (int t = tid; t < PT_T * quads; t += PT_T) {
        const int ql = t / quads, h = t - ql * quads, qq = blockIdx.x * PT_T + ql;
        if (qq >= J.nq) break;
        const int i = s_id[ql];
        uint4 val = make_uint4(0, 0, 0, 0);
        if (i >= 0) val = reinterpret_cast<const uint4 *>(P.desc + (size_t)i * P.words * 4)[h];
        J.qd[(size_t)qq * quads + h] = val;
    }
}

__global__ __launch_bounds__(PT_T) void k_points_move(const DevPointsMove M) {
    const int i = blockIdx.x * PT_T + threadIdx.x;
    if (i >= M.n) return;
    const int id = M.ids[i];
    const DevPointPlanes &P = M.P;
    if (id < 0 || id >= P.cap) return;  // (the host refused such a call)
    float *const packed[5] = {M.min_d, M.max_d, M.ref_size, M.ref_dist, M.ref_sigma};
    float *const plane[5] = {P.min_d, P.max_d, P.ref_size, P.ref_dist, P.ref_sigma};
    if (M.gather) {
        for (int k = 0; k < 3; ++k) {
            if (M.pos) M.pos[3 * i + k] = P.pos[k][id];
            if (M.normal) M.normal[3 * i + k] = P.normal[k][id];
        }
        for (int k = 0; k < 5; ++k)
            if (packed[k]) packed[k][i] = plane[k][id];
        if (M.flags) M.flags[i] = P.flags[id];
        return;
    }
    for (int k = 0; k < 3; ++k) {
        if (M.pos) P.pos[k][id] = M.pos[3 * i + k];
        if (M.normal) P.normal[k][id] = M.normal[3 * i + k];
    }
    for (int k = 0; k < 5; ++k)
        if (packed[k]) plane[k][id] = packed[k][i];
    if (M.mark_set || M.bad || M.observed) {
        unsigned f = P.flags[id];
        if (M.mark_set) f |= AFV_PTF_SET;
        if (M.bad) f = M.bad[i] ? (f | AFV_PTF_BAD) : (f & ~AFV_PTF_BAD);
        if (M.observed) f = M.observed[i] ? (f | AFV_PTF_OBSERVED) : (f & ~AFV_PTF_OBSERVED);
        P.flags[id] = (uint8_t)f;
    }
}

__global__ __launch_bounds__(PT_T) void k_points_rows(const DevPointPlanes P, const int *__restrict__ ids, int n, uint4 *packed,
                                                      const uint8_t *__restrict__ table, int table_cap, const int *__restrict__ slot,
                                                      const int *__restrict__ idx, int gather) {
    const int quads = P.words >> 2;
    const int t = blockIdx.x * PT_T + threadIdx.x;
    if (t >= n * quads) return;
    const int i = t / quads, h = t - i * quads, id = ids[i];
    if (id < 0 || id >= P.cap) return;
    uint4 *row = reinterpret_cast<uint4 *>(P.desc + (size_t)id * P.words * 4);
    if (gather) packed[t] = row[h];
    else if (table) row[h] = reinterpret_cast<const uint4 *>(table + ((size_t)slot[i] * table_cap + idx[i]) * P.words * 4)[h];  // (host-checked references)
    else row[h] = packed[t];
}

// ---------------- afv_table_fuse_points: Fuse into keyframes of the table ----------------
//   k_kffuse_project  a workgroup per (target, 256 queries): the AFV_PT_FUSE geometry with the target's camera (pt_project_one), the
//                     membership test IsInKeyFrame against the slot's plane of point ids held in the LDS, the status 0 / 1 / 2 and the
//                     rows of the id list (by the first job that names the list)
//   k_kffuse_finish   behind k_match_fuse: what sits on the winning feature - occupant and the status 3 .. 6
__global__ __launch_bounds__(PT_T) void k_kffuse_project(const DevPointPlanes P, const DevKfFuseJob *__restrict__ jobs) {
    __shared__ __attribute__((aligned(16))) int s_plane[4096];  // the slot's mvpMapPoints (a table's cap is at most 4096)
    __shared__ int s_id[PT_T];
    const DevKfFuseJob &J = jobs[blockIdx.y];
    const int tid = threadIdx.x, q = blockIdx.x * PT_T + tid;
    const int nq = J.nq, n = min(J.n, 4096);
    if ((int)blockIdx.x * PT_T >= nq) return;  // (uniform)
    const int n4 = (n + 3) & ~3;
    for (int i = tid; i < n4; i += PT_T) s_plane[i] = i < n ? J.plane[i] : -1;
    int id = -1;
    unsigned fl = 0;
    if (q < nq) {
        id = J.ids[q];
        if (id >= 0 && id < P.cap) fl = P.flags[id];
        else id = -1;
    }
    const bool valid = (fl & AFV_PTF_SET) && !(fl & AFV_PTF_BAD);
    bool ok = false;
    PtQuery o{};
    if (valid) ok = pt_project_one(P, J, AFV_PT_FUSE, id, 0.0f, o);
    __syncthreads();
    bool member = false;
    if (valid) {  // every lane walks the whole plane: the reads are broadcasts, four ids each
        const int4 *pl = reinterpret_cast<const int4 *>(s_plane);
        for (int i = 0; i < (n4 >> 2); ++i) {
            const int4 e = pl[i];
            member = member || e.x == id || e.y == id || e.z == id || e.w == id;
        }
    }
    const bool search = valid && !member && ok;
    if (!search) o = PtQuery{};
    if (q < nq) {
        J.qu[q] = o.u; J.qv[q] = o.v; J.qr[q] = o.r; J.qmin[q] = o.mn; J.qmax[q] = o.mx; J.q_ur[q] = o.ur;
        J.qvalid[q] = search ? 1 : 0;
        J.status[q] = !valid ? 0 : member ? 1 : !ok ? 2 : AFV_KF_PENDING;
    }
    if (!J.qd) return;  // (uniform)
    s_id[tid] = valid ? id : -1;
    __syncthreads();
    const int quads = P.words >> 2;
    for (int t = tid; t < PT_T * quads; t += PT_T) {
        const int ql = t / quads, h = t - ql * quads, qq = blockIdx.x * PT_T + ql;
        if (qq >= nq) break;
        const int i = s_id[ql];
        uint4 val = make_uint4(0, 0, 0, 0);
        if (i >= 0) val = reinterpret_cast<const uint4 *>(P.desc + (size_t)i * P.words * 4)[h];
        J.qd[(size_t)qq * quads + h] = val;
    }
}

__global__ __launch_bounds__(PT_T) void k_kffuse_finish(const DevPointPlanes P, const DevKfFuseJob *__restrict__ jobs) {
    const DevKfFuseJob &J = jobs[blockIdx.y];
    const int q = blockIdx.x * PT_T + threadIdx.x;
    if (q >= J.nq) return;
    const int b = J.best[q];
    int occ = -1;
    unsigned st = J.status[q];
    if (st == AFV_KF_PENDING) {
        if (b < 0 || b >= J.n) {
            st = 3;
        } else {
            occ = J.plane[b];
            if (occ < 0) {
                st = 4;
            } else {
                unsigned fl = AFV_PTF_SET;  // an occupant out of range counts as good: the store is not read for it
                if (occ < P.cap) fl = P.flags[occ];
                st = ((fl & AFV_PTF_SET) && (fl & AFV_PTF_BAD)) ? 5 : 6;
            }
        }
        J.status[q] = (uint8_t)st;
    }
    J.occupant[q] = occ;
}

extern "C" void afv_launch_kffuse_project(const DevPointPlanes *P, const DevKfFuseJob *jobs, int njobs, int max_nq, hipStream_t stream) {
    if (njobs <= 0 || max_nq <= 0) return;
    hipLaunchKernelGGL(k_kffuse_project, dim3((max_nq + PT_T - 1) / PT_T, njobs), dim3(PT_T), 0, stream, *P, jobs);
}
extern "C" void afv_launch_kffuse_finish(const DevPointPlanes *P, const DevKfFuseJob *jobs, int njobs, int max_nq, hipStream_t stream) {
    if (njobs <= 0 || max_nq <= 0) return;
    hipLaunchKernelGGL(k_kffuse_finish, dim3((max_nq + PT_T - 1) / PT_T, njobs), dim3(PT_T), 0, stream, *P, jobs);
}

extern "C" void afv_launch_points_project(const DevPointsJob *job, hipStream_t stream) {
    if (job->nq <= 0) return;
    hipLaunchKernelGGL(k_points_project, dim3((job->nq + PT_T - 1) / PT_T), dim3(PT_T), 0, stream, *job);
}

extern "C" void afv_launch_points_move(const DevPointsMove *job, hipStream_t stream) {
    if (job->n <= 0) return;
    hipLaunchKernelGGL(k_points_move, dim3((job->n + PT_T - 1) / PT_T), dim3(PT_T), 0, stream, *job);
}

extern "C" void afv_launch_points_rows(const DevPointPlanes *P, const int *ids, int n, uint8_t *packed, const uint8_t *table, int table_cap,
                                       const int *slot, const int *idx, int gather, hipStream_t stream) {
    if (n <= 0) return;
    const long total = (long)n * (P->words / 4);
    hipLaunchKernelGGL(k_points_rows, dim3((unsigned)((total + PT_T - 1) / PT_T)), dim3(PT_T), 0, stream, *P, ids, n, reinterpret_cast<uint4 *>(packed), table,
                       table_cap, slot, idx, gather);
}
