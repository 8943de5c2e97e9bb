// k_refresh.hip — MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:279-349) and MapPoint::UpdateNormalAndDepth (:372-418) for a
// batch of resident map points (include/afv_hip.h, "Refresh of resident map points"; host side: afv_refresh.hip).  The observations
// arrive as the edge lists of afv_table_bundle_adjust, grouped by point (pt_ptr); every row and plane is read where it is resident.
//
//   k_refresh_desc     a wavefront per point, four per workgroup (the shape of k_distinctive).  A ballot rank compacts the observations of
//                      keyframes that are not bad, in list order, into c_row / c_obs (the table row and the observation of the c-th good
//                      one).  Lane = row i in chunks of 64; the m-th smallest of row i by afv_bisect_mth (k_median.h: the text
//                      k_distinctive runs).  A point's rows are scattered over slots, so what is staged once is not the rows but their
//                      DISTANCES: with N <= 64 rows (the common case: a point has 2 - 30 observations) lane i computes d(i, j) once into
//                      s_d[j][i] - every lane reads row j at one address, its own row sits in registers (binary) - and the <= 10 / <= 31
//                      steps read the LDS alone, conflict-free.  Beyond 64 rows the distances are recomputed in every step, the rows
//                      re-read through c_row.  The winning row is copied into the store by the wavefront, a dword per lane.
//   k_refresh_normals  a wavefront per point: a lane per observation computes its unit vector (tri_dist of k_tri_match.h, then the
//                      division), through the LDS every lane takes the sum serially in list order; lane 0 writes the planes.
// Both skip a point that is unset or bad in the store.  The normal part reads ref_kf (mpRefKF), not the row the descriptor part chose.
// Deviations R1 - R3: include/afv_hip.h.  Plain vector stores only; no atomics, no spinning, no cooperative launch.
//
// The arithmetic is the restatement's (tests/_refresh_ref.py): float, one rounding per operator (the build's -ffp-contract=off).
#include "afv_device.h"
#include "afv_runtime.h"
#include "k_tri_row.h"
#include "k_tri_match.h"
#include "k_median.h"

#define RF_CACHE 64

// the bytes of dword w that belong to a row of `bytes` bytes: pad bytes are not part of the descriptor
__device__ __forceinline__ uint32_t rf_word_mask(int w, int bytes) {
    const int left = bytes - 4 * w;
    return left >= 4 ? 0xffffffffu : left <= 0 ? 0u : (1u << (8 * left)) - 1u;
}

__device__ __forceinline__ int rf_point_status(unsigned fl, int n) {
    if (!(fl & AFV_PTF_SET) || (fl & AFV_PTF_BAD)) return AFV_REFRESH_SKIPPED;
    return n == 0 ? AFV_REFRESH_NO_OBSERVATIONS : AFV_REFRESH_DONE;
}

// W: dwords of a binary row (8 or 16); 0: float rows of A.float_dim floats
template <int W>
__global__ __launch_bounds__(256) void k_refresh_desc(const DevRefresh A) {
    __shared__ unsigned s_d[4][RF_CACHE][64];  // [wavefront][j][lane = row i]
    const int wv = (int)threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = (int)blockIdx.x * 4 + wv;
    if (p >= A.np) return;  // wave-uniform
    const int id = A.point_ids[p];
    const int b = A.pt_ptr[p], n = A.pt_ptr[p + 1] - b;
    const int st = rf_point_status(A.P.flags[id], n);
    int N = 0;  // the observations of good keyframes (:297-306), in list order
    if (st == AFV_REFRESH_DONE) {
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int e = b + c0 + lane;
            bool good = false;
            int row = 0;
            if (c0 + lane < n) {
                const int k = A.obs_kf[e];
                good = A.kf_bad[k] == 0;
                row = A.slots[k] * A.cap + A.obs_idx[e];
            }
            const unsigned long long mask = __ballot(good);
            if (good) {
                const int c = b + N + __popcll(mask & ((1ull << lane) - 1ull));
                A.c_row[c] = row;
                A.c_obs[c] = e;
            }
            N += __popcll(mask);
        }
    }
    if (A.desc_writes_status && lane == 0) A.status[p] = st;
    if (N == 0) {
        if (lane == 0) {  // R3
            A.best_obs[p] = -1;
            A.best_median[p] = 0;
        }
        return;
    }
    WAVE_LDS_SYNC();  // c_row / c_obs of one lane are read by the others
    const int *crow = A.c_row + b;
    const int m = (N - 1) >> 1;         // vDists[0.5 * (N - 1)]
    const bool cached = N <= RF_CACHE;  // wave-uniform
    const int words = A.P.words;
    unsigned best_med = 0xffffffffu, best_row = 0xffffffffu;
    for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        const size_t ri = (size_t)crow[min(i, N - 1)];
        unsigned lo;
        if constexpr (W > 0) {
            const uint32_t *rows = reinterpret_cast<const uint32_t *>(A.desc);
            uint32_t q[W], mk[W];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                mk[w] = rf_word_mask(w, A.desc_bytes);
                q[w] = rows[ri * W + w];
            }
            auto dist = [&](int j) {
                const uint32_t *r = rows + (size_t)crow[j] * W;
                int d = 0;
#pragma unroll
                for (int w = 0; w < W; ++w) d += __popc((q[w] ^ r[w]) & mk[w]);
                return (unsigned)d;
            };
            if (cached)
                for (int j = 0; j < N; ++j) s_d[wv][j][lane] = dist(j);
            lo = afv_bisect_mth(0u, (unsigned)(8 * A.desc_bytes), m, [&](unsigned mid) {
                int cnt = 0;
                if (cached)
                    for (int j = 0; j < N; ++j) cnt += s_d[wv][j][lane] <= mid;
                else
                    for (int j = 0; j < N; ++j) cnt += dist(j) <= mid;
                return cnt;
            });
        } else {
            const float *rows = reinterpret_cast<const float *>(A.desc);
            const int dim = A.float_dim;
            const float *q = rows + ri * dim;
            auto dist = [&](int j) { return __float_as_uint(l2sqr(q, rows + (size_t)crow[j] * dim, dim)); };
            if (cached)
                for (int j = 0; j < N; ++j) s_d[wv][j][lane] = dist(j);
            lo = afv_bisect_mth(0u, 0x7f800000u, m, [&](unsigned mid) {
                int cnt = 0;
                if (cached)
                    for (int j = 0; j < N; ++j) cnt += s_d[wv][j][lane] <= mid;
                else
                    for (int j = 0; j < N; ++j) cnt += dist(j) <= mid;
                return cnt;
            });
        }
        if (i < N && lo < best_med) {  // strict: the first row keeps a tie (rows ascend with i0 inside a lane)
            best_med = lo;
            best_row = (unsigned)i;
        }
    }
    const AfvBestRow g = afv_wave_best_row(best_med, best_row);
    // mDescriptor = descriptors[BestIdx].clone() (:344): the whole padded row, as afv_points_set_descriptors_from_table copies it
    const uint32_t *src = reinterpret_cast<const uint32_t *>(A.desc) + (size_t)crow[g.row] * words;
    uint32_t *dst = reinterpret_cast<uint32_t *>(A.P.desc) + (size_t)id * words;
    for (int w = lane; w < words; w += 64) dst[w] = src[w];
    if (lane == 0) {
        A.best_obs[p] = A.c_obs[b + (int)g.row];
        A.best_median[p] = (int)g.median;
    }
}

__global__ __launch_bounds__(256) void k_refresh_normals(const DevRefresh A) {
    __shared__ float s_u[4][3][64];  // [wavefront][component][observation of the chunk]
    const int wv = (int)threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = (int)blockIdx.x * 4 + wv;
    if (p >= A.np) return;  // wave-uniform
    const int id = A.point_ids[p];
    const int b = A.pt_ptr[p], n = A.pt_ptr[p + 1] - b;
    int st = rf_point_status(A.P.flags[id], n);
    if (st != AFV_REFRESH_DONE) {  // :375-376, :383-384
        if (lane == 0) A.status[p] = st;
        return;
    }
    const float X = A.P.pos[0][id], Y = A.P.pos[1][id], Z = A.P.pos[2][id];
    const int ref = A.ref_kf[p];
    float acc[3] = {0.0f, 0.0f, 0.0f};
    bool bad = false;
    unsigned e_ref = 0xffffffffu;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int cnt = min(64, n - c0);
        if (lane < cnt) {
            const int e = b + c0 + lane, k = A.obs_kf[e];
            float nv[3];
            const float d = tri_dist(X, Y, Z, A.centres + 3 * (size_t)k, nv);
            if (!__builtin_isfinite(d) || d == 0) bad = true;  // R2
#pragma unroll
            for (int q = 0; q < 3; ++q) s_u[wv][q][lane] = nv[q] / d;
            if (k == ref) e_ref = (unsigned)e;
        }
        WAVE_LDS_ONLY_SYNC();
        for (int j = 0; j < cnt; ++j) {  // normal = normal + normal_i / normal_i.norm() (:397), in list order
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = acc[q] + s_u[wv][q][j];
        }
        WAVE_LDS_ONLY_SYNC();
    }
    bad = __any(bad);
    e_ref = afv_wave_min_u32(e_ref);
    if (ref < 0 || e_ref == 0xffffffffu) st = AFV_REFRESH_NO_REF;  // R1
    else if (bad) st = AFV_REFRESH_BAD_DISTANCE;
    if (lane != 0) return;
    A.status[p] = st;
    if (st != AFV_REFRESH_DONE) return;
    float nv[3];
    const float dist = tri_dist(X, Y, Z, A.centres + 3 * (size_t)ref, nv);
    const size_t f = (size_t)A.slots[ref] * A.cap + A.obs_idx[e_ref];
    const float size = A.size[f], max_d = dist * size;
    const DevPointPlanes &P = A.P;
#pragma unroll
    for (int q = 0; q < 3; ++q) P.normal[q][id] = acc[q] / (float)n;  // :416
    P.ref_dist[id] = dist;
    P.ref_size[id] = size;
    P.ref_sigma[id] = sqrtf(A.sigma2[f]);
    P.max_d[id] = max_d;
    P.min_d[id] = max_d / A.max_size[ref];
}

extern "C" void afv_launch_refresh_desc(const DevRefresh *A, hipStream_t stream) {
    if (A->np <= 0) return;
    const dim3 grid((A->np + 3) / 4);
    if (A->float_dim > 0) hipLaunchKernelGGL(k_refresh_desc<0>, grid, dim3(256), 0, stream, *A);
    else if (A->P.words == 8) hipLaunchKernelGGL(k_refresh_desc<8>, grid, dim3(256), 0, stream, *A);
    else hipLaunchKernelGGL(k_refresh_desc<16>, grid, dim3(256), 0, stream, *A);
}

extern "C" void afv_launch_refresh_normals(const DevRefresh *A, hipStream_t stream) {
    if (A->np <= 0) return;
    hipLaunchKernelGGL(k_refresh_normals, dim3((A->np + 3) / 4), dim3(256), 0, stream, *A);
}
