// k_voctrain.hip — vocabulary training: DBoW2 TemplatedVocabulary::create for binary descriptors (HKmeansStep, initiateClustersKMpp,
// FORB::meanValue / distance, restated from upstream DBoW2 - the reference's DBoW2 is an empty submodule, parity unpinned; the trainer the
// reference ships is src/createVocabulary.cpp:257-308).  tests/_voctrain_ref.py is the normative restatement; integer arithmetic only.
//
// All open nodes of a tree level train at once.  The rows sit in ONE array in which every node owns a contiguous segment that keeps the
// rows' original order; a node is cut into tiles of at most VT_TILE rows, a workgroup per tile.  Per level:
//   seeding      k_vt_seed_first (trivial nodes: a centre per row; else the first centre), then per draw k_vt_seed_update (min-distance
//                update, int64 sum per tile) and k_vt_seed_pick (a workgroup per node: sum of the tile sums, cut from the node's key,
//                first tile, then first row, whose running sum reaches the cut)
//   rounds       k_vt_assoc: the node's <= k centres in LDS, every row read once: Hamming argmin (first minimum), "changed" against the
//                previous association, per-(cluster, bit) counts by wave ballots (one popcount covers 64 rows of a bit) into an LDS table.
//                A one-tile node finishes in the same workgroup (majority -> new centres); a multi-tile node flushes its table with integer
//                atomics and k_vt_mean finishes it.  Converged nodes drop out (their tiles return at once); the host reads two ints a round
//   partition    k_vt_part_hist / k_vt_part_scan / k_vt_part_scatter: stable segmented partition of the rows by cluster - the next level's
//                segments, ascending original order inside a group
// and at the end k_vt_doc_count: distinct (image, word) pairs through a hash set (the result is an integer: any order gives it).
#include "afv_voctrain.h"

__device__ __forceinline__ unsigned long long vt_sm(unsigned long long x) {  // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <int W>
__device__ __forceinline__ void vt_load_row(const uint32_t *rows, long long pos, uint32_t (&r)[W]) {
    const uint4 *p = reinterpret_cast<const uint4 *>(rows + (size_t)pos * W);
#pragma unroll
    for (int w = 0; w < W / 4; ++w) {
        const uint4 t = p[w];
        r[4 * w] = t.x, r[4 * w + 1] = t.y, r[4 * w + 2] = t.z, r[4 * w + 3] = t.w;
    }
}

// sum over the workgroup (VT_THREADS threads), in every thread; s_red: 8 long long of LDS
__device__ __forceinline__ long long vt_block_sum(long long v, long long *s_red) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();  // s_red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = 0;
    for (int w = 0; w < VT_THREADS / 64; ++w) t += s_red[w];
    return t;
}

// ---------------- row preparation ----------------
__global__ __launch_bounds__(VT_THREADS) void k_vt_pad(const uint8_t *__restrict__ src, size_t pitch, int desc_bytes, long long n, int words,
                                                       uint32_t *__restrict__ dst) {
    const long long e = (long long)blockIdx.x * VT_THREADS + threadIdx.x;
    if (e >= n * words) return;
    const long long row = e / words;
    const int w = (int)(e - row * words);
    const uint8_t *p = src + (size_t)row * pitch;
    uint32_t v = 0;
    for (int b = 0; b < 4; ++b)
        if (4 * w + b < desc_bytes) v |= (uint32_t)p[4 * w + b] << (8 * b);
    dst[e] = v;
}

// ---------------- seeding ----------------
__global__ __launch_bounds__(64) void k_vt_seed_first(VtArgs a) {
    const int b = blockIdx.x, W = a.words, k = a.k;
    const VtNode nd = a.nodes[b];
    uint32_t *cen = a.centres + (size_t)b * k * W;
    if (nd.len <= k) {  // the trivial case of HKmeansStep: a cluster per feature, in order
        for (int e = threadIdx.x; e < nd.len * W; e += 64) cen[e] = a.rows[(size_t)nd.start * W + e];
        for (int c = threadIdx.x; c < nd.len; c += 64) {
            a.assign[nd.start + c] = (uint8_t)c;
            a.sizes[b * k + c] = 1;
        }
        if (threadIdx.x == 0) a.ncent[b] = nd.len, a.done[b] = 1, a.seeded[b] = 1;
        return;
    }
    if (a.seeded[b]) return;  // the host put init_centres there
    const long long idx = (long long)(vt_sm(nd.key) % (unsigned long long)nd.len);
    for (int e = threadIdx.x; e < W; e += 64) cen[e] = a.rows[(size_t)(nd.start + idx) * W + e];
    if (threadIdx.x == 0) a.ncent[b] = 1;
}

template <int W>
__global__ __launch_bounds__(VT_THREADS) void k_vt_seed_update(VtArgs a) {
    __shared__ uint32_t s_c[W];
    __shared__ long long s_red[8];
    const VtTile t = a.tiles[blockIdx.x];
    if (a.seeded[t.node]) return;  // (uniform; k_vt_seed_pick does not read the tile sums of such a node)
    const uint32_t *last = a.centres + ((size_t)t.node * a.k + (a.ncent[t.node] - 1)) * W;
    if (threadIdx.x < W) s_c[threadIdx.x] = last[threadIdx.x];
    __syncthreads();
    long long sum = 0;
    for (int i = threadIdx.x; i < t.len; i += VT_THREADS) {
        const int pos = t.start + i;
        int md = a.draw == 1 ? 0x7fffffff : a.mindist[pos];
        if (md > 0) {
            uint32_t r[W];
            vt_load_row<W>(a.rows, pos, r);
            int d = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) d += __popc(r[w] ^ s_c[w]);
            if (d < md) md = d;
            a.mindist[pos] = md;
        }
        sum += md;
    }
    sum = vt_block_sum(sum, s_red);
    if (threadIdx.x == 0) a.tile_sum[blockIdx.x] = sum;
}

// first index i < count with base + val(0) + ... + val(i) >= cut, or -1; `base` becomes the sum BEFORE that index (or base + all)
template <class F>
__device__ __forceinline__ int vt_first_geq(F val, int count, long long &base, long long cut, long long *s_scan, long long *s_before, int *s_idx) {
    const int tid = threadIdx.x;
    for (int c0 = 0; c0 < count; c0 += VT_THREADS) {
        const int i = c0 + tid;
        const long long v = i < count ? (long long)val(i) : 0;
        __syncthreads();
        s_scan[tid] = v;
        if (tid == 0) *s_idx = 0x7fffffff;
        __syncthreads();
        for (int off = 1; off < VT_THREADS; off <<= 1) {
            const long long u = tid >= off ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += u;
            __syncthreads();
        }
        const long long incl = s_scan[tid];
        if (i < count && base + incl >= cut) atomicMin(s_idx, i);
        __syncthreads();
        const int found = *s_idx;
        if (found != 0x7fffffff) {
            if (i == found) *s_before = base + incl - v;
            __syncthreads();
            base = *s_before;
            return found;
        }
        base += s_scan[VT_THREADS - 1];
    }
    return -1;
}

__global__ __launch_bounds__(VT_THREADS) void k_vt_seed_pick(VtArgs a) {
    __shared__ long long s_scan[VT_THREADS], s_red[8], s_before;
    __shared__ int s_idx;
    const int b = blockIdx.x, W = a.words;
    if (a.seeded[b]) return;
    const VtNode nd = a.nodes[b];
    const int nc = a.ncent[b];
    const long long *ts = a.tile_sum + nd.tile0;
    long long part = 0;
    for (int i = threadIdx.x; i < nd.ntiles; i += VT_THREADS) part += ts[i];
    const long long total = vt_block_sum(part, s_red);
    if (total == 0) {  // every row equals a centre: seeding stops with fewer than k centres
        if (threadIdx.x == 0) a.seeded[b] = 1;
        return;
    }
    const long long cut = 1 + (long long)(vt_sm(nd.key + (unsigned long long)a.draw * VT_DRAW_STEP) % (unsigned long long)total);
    long long base = 0;
    const int ti = vt_first_geq([&](int i) { return ts[i]; }, nd.ntiles, base, cut, s_scan, &s_before, &s_idx);
    if (ti < 0) return;  // (cannot happen: total >= cut)
    const VtTile t = a.tiles[nd.tile0 + ti];
    const int32_t *md = a.mindist + t.start;
    const int ri = vt_first_geq([&](int i) { return md[i]; }, t.len, base, cut, s_scan, &s_before, &s_idx);
    if (ri < 0) return;
    uint32_t *cen = a.centres + ((size_t)b * a.k + nc) * W;
    if (threadIdx.x < W) cen[threadIdx.x] = a.rows[(size_t)(t.start + ri) * W + threadIdx.x];
    if (threadIdx.x == 0) {
        a.ncent[b] = nc + 1;
        if (nc + 1 == a.k) a.seeded[b] = 1;
    }
}

// ---------------- association rounds ----------------
// new centres of a node from its per-(cluster, bit) counts (FORB::meanValue: bit set iff count >= N / 2 + N % 2; one member: the member
// itself, which the same rule gives; an EMPTY cluster keeps its centre - the deviation from upstream, include/afv_hip.h).  cnt[bit * k + c].
template <class T>
__device__ __forceinline__ void vt_majority(const T *cnt, const int *size, int nc, int k, int W, uint32_t *cen) {
    for (int e = threadIdx.x; e < nc * W; e += VT_THREADS) {
        const int c = e / W, w = e - c * W;
        const int N = size[c];
        if (N == 0) continue;
        const unsigned th = (unsigned)(N / 2 + N % 2);
        uint32_t bits = 0;
        for (int i = 0; i < 32; ++i)
            if ((unsigned)cnt[(w * 32 + i) * k + c] >= th) bits |= 1u << i;
        cen[e] = bits;
    }
}

// what a node does with the outcome of a round (thread 0 of the workgroup that finishes the node); returns whether new centres are due
__device__ __forceinline__ bool vt_round_outcome(const VtArgs &a, int b, bool changed) {
    const bool capped = changed && a.max_iters > 0 && a.round >= a.max_iters;
    if (threadIdx.x == 0) {
        if (!changed || capped) a.done[b] = 1;
        else atomicAdd(&a.status[0], 1);
        if (capped) a.status[1] = 1;
    }
    return changed && !capped;
}

template <int W>
__global__ __launch_bounds__(VT_THREADS) void k_vt_assoc(VtArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    constexpr int BITS = W * 32;
    const int k = a.k, tid = threadIdx.x, lane = tid & 63;
    const VtTile t = a.tiles[blockIdx.x];
    const int b = t.node;
    if (a.done[b]) return;  // converged (or trivial) nodes drop out
    const int nc = a.ncent[b];
    uint32_t *s_cnt = s_dyn;             // [BITS][k]
    uint32_t *s_c = s_cnt + BITS * k;    // [k][W]
    int *s_size = reinterpret_cast<int *>(s_c + k * W);  // [k]
    uint32_t *cen = a.centres + (size_t)b * k * W;
    for (int e = tid; e < BITS * k; e += VT_THREADS) s_cnt[e] = 0;
    for (int e = tid; e < nc * W; e += VT_THREADS) s_c[e] = cen[e];
    if (tid < k) s_size[tid] = 0;
    __syncthreads();
    int my_changed = 0;
    for (int base = 0; base < t.len; base += VT_THREADS) {
        const bool active = base + tid < t.len;
        if (__ballot(active) == 0) continue;  // (wave-uniform; no barrier inside this loop)
        const int pos = t.start + base + tid;
        uint32_t r[W];
        int asg = 0xff;
        if (active) {
            vt_load_row<W>(a.rows, pos, r);
            int best = 0x7fffffff;
            for (int c = 0; c < nc; ++c) {
                int d = 0;
#pragma unroll
                for (int w = 0; w < W; ++w) d += __popc(r[w] ^ s_c[c * W + w]);
                if (d < best) best = d, asg = c;  // strictly smaller wins: the first minimum stays
            }
            if (a.assign[pos] != (uint8_t)asg) my_changed = 1;
            a.assign[pos] = (uint8_t)asg;
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) r[w] = 0;
        }
        // lane c keeps the mask of this wave's rows in cluster c; a ballot per bit, one popcount counts 64 rows
        unsigned long long mymask = 0;
        for (int c = 0; c < nc; ++c) {
            const unsigned long long bm = __ballot(asg == c);
            if (lane == c) mymask = bm;
        }
        if (lane < nc && mymask) atomicAdd(&s_size[lane], __popcll(mymask));
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t x = r[w];
            for (int i = 0; i < 32; ++i) {
                const unsigned long long m = __ballot((x >> i) & 1u);
                if (lane < nc) {
                    const int v = __popcll(m & mymask);
                    if (v) atomicAdd(&s_cnt[(w * 32 + i) * k + lane], (uint32_t)v);
                }
            }
        }
    }
    const int any_changed = __syncthreads_or(my_changed);
    const VtNode nd = a.nodes[b];
    if (nd.slot < 0) {  // the node is this tile: finish it here
        const bool changed = a.round == 1 || any_changed;
        if (tid < k) a.sizes[b * k + tid] = tid < nc ? s_size[tid] : 0;
        if (vt_round_outcome(a, b, changed)) vt_majority(s_cnt, s_size, nc, k, W, cen);
        return;
    }
    uint32_t *g = a.gcnt + (size_t)nd.slot * BITS * k;
    for (int e = tid; e < BITS * k; e += VT_THREADS) {
        const uint32_t v = s_cnt[e];
        if (v) atomicAdd(&g[e], v);
    }
    if (tid < nc && s_size[tid]) atomicAdd(&a.gsize[nd.slot * k + tid], s_size[tid]);
    if (tid == 0 && any_changed) atomicOr(&a.changed[b], 1);
}

// multi-tile nodes: a workgroup per node finishes the round from the flushed counts and clears them for the next one
__global__ __launch_bounds__(VT_THREADS) void k_vt_mean(VtArgs a) {
    __shared__ int s_size[32];
    const int b = a.multi[blockIdx.x], k = a.k, W = a.words, tid = threadIdx.x;
    if (a.done[b]) return;
    const VtNode nd = a.nodes[b];
    const int nc = a.ncent[b], bits = W * 32;
    uint32_t *g = a.gcnt + (size_t)nd.slot * bits * k;
    int *gs = a.gsize + nd.slot * k;
    if (tid < k) {
        s_size[tid] = tid < nc ? gs[tid] : 0;
        a.sizes[b * k + tid] = s_size[tid];
    }
    const bool changed = a.round == 1 || a.changed[b];
    __syncthreads();
    if (vt_round_outcome(a, b, changed)) vt_majority(g, s_size, nc, k, W, a.centres + (size_t)b * k * W);
    __syncthreads();
    for (int e = tid; e < bits * k; e += VT_THREADS) g[e] = 0;
    if (tid < k) gs[tid] = 0;
    if (tid == 0) a.changed[b] = 0;
}

// ---------------- stable segmented partition by cluster ----------------
__global__ __launch_bounds__(VT_THREADS) void k_vt_part_hist(VtArgs a) {
    __shared__ int s_h[32];
    const VtTile t = a.tiles[blockIdx.x];
    if (threadIdx.x < 32) s_h[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < t.len; i += VT_THREADS) atomicAdd(&s_h[a.assign[t.start + i] & 31], 1);
    __syncthreads();
    if (threadIdx.x < a.k) a.tile_hist[blockIdx.x * a.k + threadIdx.x] = s_h[threadIdx.x];
}

__global__ __launch_bounds__(64) void k_vt_part_scan(VtArgs a) {
    const int b = blockIdx.x, c = threadIdx.x, k = a.k;
    if (c >= k) return;
    const VtNode nd = a.nodes[b];
    int off = nd.start;
    for (int cc = 0; cc < c; ++cc) off += a.sizes[b * k + cc];
    for (int t = nd.tile0; t < nd.tile0 + nd.ntiles; ++t) {
        a.tile_off[t * k + c] = off;
        off += a.tile_hist[t * k + c];
    }
}

template <int W>
__global__ __launch_bounds__(VT_THREADS) void k_vt_part_scatter(VtArgs a) {
    __shared__ int s_run[32], s_wc[VT_THREADS / 64][32];
    const int k = a.k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const VtTile t = a.tiles[blockIdx.x];
    if (tid < 32) s_run[tid] = tid < k ? a.tile_off[blockIdx.x * k + tid] : 0;
    for (int base = 0; base < t.len; base += VT_THREADS) {
        const bool active = base + tid < t.len;
        const int pos = t.start + base + tid;
        const int asg = active ? (int)a.assign[pos] : 0xff;
        int rank = 0;
        for (int c = 0; c < k; ++c) {
            const unsigned long long m = __ballot(asg == c);
            if (asg == c) rank = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == c) s_wc[wave][c] = __popcll(m);
        }
        __syncthreads();  // (also orders s_run's initialisation / last update before its use)
        if (active && asg < k) {
            int dst = s_run[asg] + rank;
            for (int w = 0; w < wave; ++w) dst += s_wc[w][asg];
            const uint4 *src = reinterpret_cast<const uint4 *>(a.rows + (size_t)pos * W);
            uint4 *out = reinterpret_cast<uint4 *>(a.rows_out + (size_t)dst * W);
#pragma unroll
            for (int w = 0; w < W / 4; ++w) out[w] = src[w];
        }
        __syncthreads();
        if (tid < k) {
            int s = 0;
            for (int w = 0; w < VT_THREADS / 64; ++w) s += s_wc[w][tid];
            s_run[tid] += s;
        }
        __syncthreads();
    }
}

// ---------------- document counts ----------------
// Ni[word] = images with at least one feature whose descent ends in the word: every (image, leaf) pair enters a hash set once (open
// addressing, the table holds at least twice the rows); whoever claims the empty slot counts the pair
__global__ __launch_bounds__(VT_THREADS) void k_vt_doc_count(const int *__restrict__ leaf, long long n, const int *__restrict__ image_ptr, int nimages,
                                                             unsigned long long *table, unsigned long long mask, int *ni) {
    const long long i = (long long)blockIdx.x * VT_THREADS + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nimages;  // the last image whose first row is <= i (empty images share a start with their successor: skipped)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)image_ptr[mid] <= i) lo = mid;
        else hi = mid;
    }
    const int lf = leaf[i];
    const unsigned long long key = ((unsigned long long)(unsigned)lo << 32) | (unsigned)lf;
    unsigned long long h = vt_sm(key) & mask;
    for (unsigned long long probe = 0; probe <= mask; ++probe) {
        const unsigned long long old = atomicCAS(&table[h], ~0ull, key);
        if (old == ~0ull) {
            atomicAdd(&ni[lf], 1);
            return;
        }
        if (old == key) return;
        h = (h + 1) & mask;
    }
}

// ---------------- launchers ----------------
extern "C" size_t afv_voctrain_assoc_lds(int k, int words) { return ((size_t)words * 32 * k + (size_t)k * words + (size_t)k) * 4; }

// once per call: k = 32 with 512-bit rows asks for 66 KB of dynamic LDS, more than the 64 KB a kernel gets by default
extern "C" int afv_voctrain_prepare(void) {
    bool ok = hipFuncSetAttribute(reinterpret_cast<const void *>(k_vt_assoc<8>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024) == hipSuccess;
    ok = hipFuncSetAttribute(reinterpret_cast<const void *>(k_vt_assoc<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024) == hipSuccess && ok;
    if (!ok) (void)hipGetLastError();
    return ok ? 1 : 0;
}

extern "C" void afv_launch_vt_pad(const uint8_t *src, size_t pitch, int desc_bytes, long long n, int words, uint32_t *dst, hipStream_t stream) {
    const long long total = n * words;
    hipLaunchKernelGGL(k_vt_pad, dim3((unsigned)((total + VT_THREADS - 1) / VT_THREADS)), dim3(VT_THREADS), 0, stream, src, pitch, desc_bytes, n, words, dst);
}

extern "C" void afv_launch_vt_seed_first(const VtArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(k_vt_seed_first, dim3(a->nnodes), dim3(64), 0, stream, *a);
}

extern "C" void afv_launch_vt_seed_draw(const VtArgs *a, hipStream_t stream) {
    if (a->words == 8) hipLaunchKernelGGL(k_vt_seed_update<8>, dim3(a->ntiles), dim3(VT_THREADS), 0, stream, *a);
    else hipLaunchKernelGGL(k_vt_seed_update<16>, dim3(a->ntiles), dim3(VT_THREADS), 0, stream, *a);
    hipLaunchKernelGGL(k_vt_seed_pick, dim3(a->nnodes), dim3(VT_THREADS), 0, stream, *a);
}

extern "C" void afv_launch_vt_round(const VtArgs *a, hipStream_t stream) {
    const size_t lds = afv_voctrain_assoc_lds(a->k, a->words);
    if (a->words == 8) hipLaunchKernelGGL(k_vt_assoc<8>, dim3(a->ntiles), dim3(VT_THREADS), lds, stream, *a);
    else hipLaunchKernelGGL(k_vt_assoc<16>, dim3(a->ntiles), dim3(VT_THREADS), lds, stream, *a);
    if (a->nmulti > 0) hipLaunchKernelGGL(k_vt_mean, dim3(a->nmulti), dim3(VT_THREADS), 0, stream, *a);
}

extern "C" void afv_launch_vt_partition(const VtArgs *a, hipStream_t stream) {
    hipLaunchKernelGGL(k_vt_part_hist, dim3(a->ntiles), dim3(VT_THREADS), 0, stream, *a);
    hipLaunchKernelGGL(k_vt_part_scan, dim3(a->nnodes), dim3(64), 0, stream, *a);
    if (a->words == 8) hipLaunchKernelGGL(k_vt_part_scatter<8>, dim3(a->ntiles), dim3(VT_THREADS), 0, stream, *a);
    else hipLaunchKernelGGL(k_vt_part_scatter<16>, dim3(a->ntiles), dim3(VT_THREADS), 0, stream, *a);
}

extern "C" void afv_launch_vt_doc_count(const int *leaf, long long n, const int *image_ptr, int nimages, unsigned long long *table,
                                        unsigned long long table_mask, int *ni, hipStream_t stream) {
    hipLaunchKernelGGL(k_vt_doc_count, dim3((unsigned)((n + VT_THREADS - 1) / VT_THREADS)), dim3(VT_THREADS), 0, stream, leaf, n, image_ptr, nimages, table,
                       table_mask, ni);
}
