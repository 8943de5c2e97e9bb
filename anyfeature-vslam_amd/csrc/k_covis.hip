// k_covis.hip — the kernels of afv_table_covis_votes and afv_table_local_points (include/afv_covis.h; host side: afv_covis.hip).
//
// Reference: KeyFrame::UpdateConnections (KeyFrame.cc:329-418), Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (Tracking.cc:1040-1104)
// and the skip of SearchLocalPoints (Tracking.cc:1003-1005).  The reference answers "which keyframes observe this point" from
// MapPoint::GetObservations(); here the answer is read from the mvpMapPoints planes of the table: keyframe k observes id p when p stands in
// plane(k).  All arithmetic is integer: any order of the sums gives the same answer.
#include "afv_runtime.h"
#include "k_covis.h"

namespace {

constexpr int CV_T = 256;          // lanes per workgroup of every kernel here
constexpr int CV_HASH = 8192;      // words of the id set of one plane: at most AFV_COVIS_MAX_CAP = 4096 distinct ids, half full
constexpr unsigned CV_EMPTY = 0xffffffffu;

__device__ __forceinline__ bool cv_good(const DevPointPlanes &P, int id) {  // V1
    if (id < 0 || id >= P.cap) return false;
    const unsigned fl = P.flags[id];
    return (fl & AFV_PTF_SET) && !(fl & AFV_PTF_BAD);
}
__device__ __forceinline__ unsigned cv_hash(unsigned id) { return (id * 2654435761u) >> 19; }  // 13 bits

// every query as a list of good ids, -1 where the entry is skipped: the plane of a slot or the caller's list, filtered once
__global__ __launch_bounds__(CV_T) void k_covis_filter(const DevPointPlanes P, const DevCovisQuery *__restrict__ queries) {
    const DevCovisQuery &Q = queries[blockIdx.y];
    for (int i = blockIdx.x * CV_T + threadIdx.x; i < Q.n; i += gridDim.x * CV_T) {
        const int id = Q.src[i];
        Q.dst[i] = cv_good(P, id) ? id : -1;
    }
}

// one workgroup per listed keyframe: the set of the distinct ids of its plane in the LDS, then every query streamed over it
__global__ __launch_bounds__(CV_T) void k_covis_votes(const DevCovisVotes A) {
    __shared__ unsigned s_set[CV_HASH];
    __shared__ int s_votes[AFV_COVIS_MAX_QUERIES];
    const int k = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < CV_HASH; i += CV_T) s_set[i] = CV_EMPTY;
    if (tid < AFV_COVIS_MAX_QUERIES) s_votes[tid] = 0;
    __syncthreads();
    const int *plane = A.mp + (size_t)A.slots[k] * A.cap;
    const int n = A.kf_n[k];
    for (int i = tid; i < n; i += CV_T) {
        const int id = plane[i];
        if (id < 0) continue;
        unsigned h = cv_hash((unsigned)id);
        for (;;) {  // at most 4096 distinct ids in 8192 words: an empty word is always met
            const unsigned old = atomicCAS(&s_set[h], CV_EMPTY, (unsigned)id);
            if (old == CV_EMPTY || old == (unsigned)id) break;  // a duplicate of the plane stands in the set once
            h = (h + 1) & (CV_HASH - 1);
        }
    }
    __syncthreads();
    for (int q = 0; q < A.nq; ++q) {
        const DevCovisQuery &Q = A.queries[q];
        if (Q.self == k) continue;  // obs.first == keyId (uniform over the workgroup); s_votes[q] stays 0
        int hits = 0;
        for (int i = tid; i < Q.n; i += CV_T) {
            const int id = Q.dst[i];
            if (id < 0) continue;
            unsigned h = cv_hash((unsigned)id);
            for (;;) {
                const unsigned e = s_set[h];
                if (e == (unsigned)id) { ++hits; break; }  // a duplicate of the query counts every time
                if (e == CV_EMPTY) break;
                h = (h + 1) & (CV_HASH - 1);
            }
        }
        if (hits) atomicAdd(&s_votes[q], hits);
    }
    __syncthreads();
    if (tid < A.nq) A.votes[(size_t)tid * A.nk + k] = s_votes[tid];
}

// one workgroup per query: the connection rule over a row of votes
__global__ __launch_bounds__(CV_T) void k_covis_order(const DevCovisVotes A) {
    __shared__ int s_v[AFV_COVIS_MAX_KF], s_key[AFV_COVIS_MAX_KF], s_order[AFV_COVIS_MAX_KF];
    __shared__ uint8_t s_in[AFV_COVIS_MAX_KF];  // bit 0: stands for best, bit 1: member of order
    __shared__ uint16_t s_list[AFV_COVIS_MAX_KF];  // the members, in no particular order: the rank below is a count, not a position here
    __shared__ unsigned long long s_best;
    __shared__ int s_cnt[2];
    const int q = blockIdx.x, tid = threadIdx.x, nk = A.nk;
    const DevCovisQuery &Q = A.queries[q];
    const int th = Q.th;
    if (tid == 0) { s_best = 0ull; s_cnt[0] = 0; s_cnt[1] = 0; }
    __syncthreads();
    int nz = 0;
    unsigned long long mine = 0ull;
    for (int p = tid; p < nk; p += CV_T) {
        const int v = A.votes[(size_t)q * nk + p], key = A.key_id[p];
        const bool stands = v > 0 && !(Q.skip_bad && A.kf_bad[p]);  // Tracking.cc:1087
        const bool member = stands && v >= th;
        s_v[p] = v; s_key[p] = key; s_order[p] = -1;
        s_in[p] = (uint8_t)((stands ? 1 : 0) | (member ? 2 : 0));
        nz += v > 0;
        if (member) s_list[atomicAdd(&s_cnt[1], 1)] = (uint16_t)p;
        if (stands) {  // the highest vote, ties to the lowest keyId: `>` while the map is walked in ascending keyId
            const unsigned long long rec = ((unsigned long long)(unsigned)v << 32) | (unsigned)~((unsigned)key ^ 0x80000000u);
            mine = rec > mine ? rec : mine;
        }
    }
    if (nz) atomicAdd(&s_cnt[0], nz);
    if (mine) atomicMax(&s_best, mine);
    __syncthreads();
    const unsigned long long top = s_best;
    const int n_members = s_cnt[1];
    int best = -1;
    for (int p = tid; p < nk; p += CV_T) {
        if (!(s_in[p] & 1)) continue;
        const unsigned long long rec = ((unsigned long long)(unsigned)s_v[p] << 32) | (unsigned)~((unsigned)s_key[p] ^ 0x80000000u);
        if (rec == top) best = p;  // the keyIds are distinct: one position
    }
    if (best >= 0) {
        A.best[q] = best;
        if (n_members == 0) s_order[0] = best;  // the vPairs.empty() branch
    }
    // rank by counting: votes descending, ties by keyId descending (KeyframeComparison, then push_front)
    for (int p = tid; p < nk; p += CV_T) {
        if (!(s_in[p] & 2)) continue;
        const int v = s_v[p], key = s_key[p];
        int rank = 0;
        for (int m = 0; m < n_members; ++m) {
            const int o = s_list[m], vo = s_v[o];
            rank += vo > v || (vo == v && s_key[o] > key);
        }
        s_order[rank] = p;
    }
    __syncthreads();
    if (tid == 0) {
        if (top == 0ull) A.best[q] = -1;
        A.n_nonzero[q] = s_cnt[0];
        A.n_order[q] = n_members ? n_members : (top ? 1 : 0);
    }
    for (int p = tid; p < nk; p += CV_T) A.order[(size_t)q * nk + p] = s_order[p];
}

// ---- local points: candidate (l, i) carries the key l * cap + i; the lowest key of an id is its first occurrence ----
__global__ __launch_bounds__(CV_T) void k_covis_local_min(const DevCovisLocal A) {
    const int l = blockIdx.y, n = A.local_n[l];
    const int *plane = A.mp + (size_t)A.local[l] * A.cap;
    for (int i = blockIdx.x * CV_T + threadIdx.x; i < n; i += gridDim.x * CV_T) {
        const int id = plane[i];
        if (cv_good(A.P, id)) atomicMin(&A.word[id], (unsigned)(l * A.cap + i));
    }
}

// survivors per listed keyframe (one workgroup each)
__global__ __launch_bounds__(CV_T) void k_covis_local_count(const DevCovisLocal A) {
    __shared__ int s_n;
    const int l = blockIdx.x, n = A.local_n[l], tid = threadIdx.x;
    const int *plane = A.mp + (size_t)A.local[l] * A.cap;
    if (tid == 0) s_n = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += CV_T) {
        const int id = plane[i];
        mine += cv_good(A.P, id) && A.word[id] == (unsigned)(l * A.cap + i);
    }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (tid == 0) A.count[l] = s_n;
}

// the ordered compaction: workgroup l starts behind the survivors of 0 .. l - 1 and walks its plane in ascending feature index
__global__ __launch_bounds__(CV_T) void k_covis_local_compact(const DevCovisLocal A) {
    __shared__ int s_scan[CV_T];
    __shared__ int s_base, s_total;
    const int l = blockIdx.x, n = A.local_n[l], tid = threadIdx.x;
    const int *plane = A.mp + (size_t)A.local[l] * A.cap;
    if (tid == 0) { s_base = 0; s_total = 0; }
    __syncthreads();
    int before = 0, all = 0;
    for (int j = tid; j < A.nl; j += CV_T) {
        const int c = A.count[j];
        all += c;
        if (j < l) before += c;
    }
    if (before) atomicAdd(&s_base, before);
    if (all) atomicAdd(&s_total, all);
    __syncthreads();
    const int total = s_total;
    if (l == 0 && tid == 0) *A.total = total;
    if (total > A.max_out) return;  // AFV_ECAPACITY: nothing is written (uniform)
    int base = s_base;
    for (int i0 = 0; i0 < n; i0 += CV_T) {
        const int i = i0 + tid;
        int id = -1;
        bool keep = false;
        if (i < n) {
            id = plane[i];
            keep = cv_good(A.P, id) && A.word[id] == (unsigned)(l * A.cap + i);
        }
        s_scan[tid] = keep ? 1 : 0;
        __syncthreads();
        for (int d = 1; d < CV_T; d <<= 1) {  // inclusive scan of the chunk
            const int add = tid >= d ? s_scan[tid - d] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        if (keep) {
            const int j = base + s_scan[tid] - 1;
            A.ids_out[j] = id;
            A.pos[id] = j;
        }
        base += s_scan[CV_T - 1];
        __syncthreads();
    }
}

// seen[j] = 1 where local point j is a good id of the frame's list (idLastFrameSeen == currentFrame.mnId)
__global__ __launch_bounds__(CV_T) void k_covis_local_seen(const DevCovisLocal A) {
    if (*A.total > A.max_out) return;
    for (int i = blockIdx.x * CV_T + threadIdx.x; i < A.n_pts; i += gridDim.x * CV_T) {
        const int id = A.frame_pts[i];
        if (cv_good(A.P, id) && A.word[id] != CV_EMPTY) A.seen[A.pos[id]] = 1;
    }
}

// the words this call touched go back to rest
__global__ __launch_bounds__(CV_T) void k_covis_local_restore(const DevCovisLocal A) {
    const int l = blockIdx.y, n = A.local_n[l];
    const int *plane = A.mp + (size_t)A.local[l] * A.cap;
    for (int i = blockIdx.x * CV_T + threadIdx.x; i < n; i += gridDim.x * CV_T) {
        const int id = plane[i];
        if (cv_good(A.P, id)) A.word[id] = CV_EMPTY;
    }
}

}  // namespace

extern "C" void afv_launch_covis_votes(const DevPointPlanes *P, const DevCovisVotes *A, int max_n, hipStream_t stream) {
    if (max_n > 0) {
        const int bx = std::min((max_n + CV_T - 1) / CV_T, 64);
        hipLaunchKernelGGL(k_covis_filter, dim3(bx, A->nq), dim3(CV_T), 0, stream, *P, A->queries);
    }
    hipLaunchKernelGGL(k_covis_votes, dim3(A->nk), dim3(CV_T), 0, stream, *A);
    hipLaunchKernelGGL(k_covis_order, dim3(A->nq), dim3(CV_T), 0, stream, *A);
}

extern "C" void afv_launch_covis_local(const DevCovisLocal *A, int max_n, hipStream_t stream) {
    const int bx = std::max(1, std::min((max_n + CV_T - 1) / CV_T, 16));
    hipLaunchKernelGGL(k_covis_local_min, dim3(bx, A->nl), dim3(CV_T), 0, stream, *A);
    hipLaunchKernelGGL(k_covis_local_count, dim3(A->nl), dim3(CV_T), 0, stream, *A);
    hipLaunchKernelGGL(k_covis_local_compact, dim3(A->nl), dim3(CV_T), 0, stream, *A);
    if (A->seen && A->n_pts > 0) hipLaunchKernelGGL(k_covis_local_seen, dim3(std::min((A->n_pts + CV_T - 1) / CV_T, 64)), dim3(CV_T), 0, stream, *A);
    hipLaunchKernelGGL(k_covis_local_restore, dim3(bx, A->nl), dim3(CV_T), 0, stream, *A);
}
