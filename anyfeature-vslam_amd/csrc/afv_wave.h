// afv_wave.h — device building blocks shared by the matcher-shaped kernels: wavefront hand-offs and DPP reductions, the rotation
// histogram rules of FeatureMatcher.cc, and the workgroup scaffolding of the three fixed-point engines (k_match_resolve_wg in
// k_match.hip, proj_resolve_wg and init_resolve_wg in k_project.hip).  Included by .hip files only.
//
// Every block here is parity critical: the outcome must equal the reference's sequential loop bit for bit, so there is ONE copy of each.
// Small results leave by value (a struct of ints), never through reference out-parameters: with `int &` parameters the three bin indices
// of afv_three_maxima stayed in private memory after inlining (scratch in seven kernels of k_project.hip, up to 28 more vector
// registers); by value every kernel descriptor equals the hand-inlined form.
#pragma once

#include <stdint.h>

// ---------------- LDS hand-offs inside ONE wavefront ----------------
// LDS hand-off between lanes of ONE wavefront: DS operations of a wave execute in order, only the compiler has to be
// kept from moving reads above writes
#define WAVE_LDS_SYNC()                                        \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
        __builtin_amdgcn_wave_barrier();                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); \
    } while (0)

// The same hand-off when nothing but LDS traffic of THIS wavefront has to be ordered: a workgroup-scope release also drains the
// vector-memory counter, i.e. it waits for every global store / load the wavefront still has in flight (about 2 us per round of the
// ordered resolve walk, measured) — wavefront scope keeps the compiler from reordering and costs nothing at run time.  Legal only
// where what the lanes hand over is in LDS alone (WAVE_LDS_SYNC when a global store of one lane is read by another behind it).
#define WAVE_LDS_ONLY_SYNC()                                   \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)

// ---------------- DPP control words ----------------
#define DPP_QUAD_XOR1 0xB1       // quad_perm:[1,0,3,2]
#define DPP_QUAD_XOR2 0x4E       // quad_perm:[2,3,0,1]
#define DPP_ROW_HALF_MIRROR 0x141
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_ROW_BCAST15 0x142    // lane 15 of each row into the next row: row mask 0xa = rows 1, 3
#define DPP_ROW_BCAST31 0x143    // lane 31 into rows 2, 3: row mask 0xc
// one step (OP) of a 64-lane reduction per control word, in the order every reduction below takes them: row shifts inside the rows of 16
// lanes, then row_bcast15 / row_bcast31 carry the row results.  Lane 63 ends up with the result over all lanes.
#define AFV_DPP_REDUCE64(OP)      \
    OP(DPP_ROW_SHR(1), 0xf)       \
    OP(DPP_ROW_SHR(2), 0xf)       \
    OP(DPP_ROW_SHR(4), 0xf)       \
    OP(DPP_ROW_SHR(8), 0xf)       \
    OP(DPP_ROW_BCAST15, 0xa)      \
    OP(DPP_ROW_BCAST31, 0xc)

// inclusive prefix sum over the 64 lanes of a wavefront on DPP (no LDS crossbar: a __shfl_up step is a ds_bpermute, ~100+ cycles of
// latency each; the latency-bound kernels — quadtree, retainBest — run dozens of these scans back to back): 4 Hillis-Steele steps
// inside each row of 16 lanes, then the row totals are carried over with row_bcast15 (rows 1, 3) and row_bcast31 (rows 2, 3)
static inline __device__ int afv_wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(1), 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(2), 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(4), 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR(8), 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_BCAST15, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_BCAST31, 0xc, 0xf, false);
    return v;
}
// sum over the 64 lanes (every lane receives it): the scan, then the last lane's total through a scalar register
__device__ __forceinline__ int afv_wave_sum(int v) { return __builtin_amdgcn_readlane(afv_wave_incl_scan(v), 63); }

// wave-wide minimum on DPP (row shifts inside the rows of 16 lanes, then row_bcast15 / row_bcast31 carry the row results: no LDS
// crossbar - a __shfl_xor butterfly is six dependent ds_bpermute pairs per call); every lane receives the result
__device__ __forceinline__ unsigned long long afv_wave_min_u64(unsigned long long v) {
#define AFV_MIN64_STEP(ctrl, rmask)                                                                                       \
    {                                                                                                                     \
        const unsigned lo_ = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)v, ctrl, rmask, 0xf, false);        \
        const unsigned hi_ = (unsigned)__builtin_amdgcn_update_dpp(-1, (int)(unsigned)(v >> 32), ctrl, rmask, 0xf, false); \
        const unsigned long long t_ = ((unsigned long long)hi_ << 32) | lo_;                                              \
        v = t_ < v ? t_ : v;                                                                                              \
    }
    AFV_DPP_REDUCE64(AFV_MIN64_STEP)
#undef AFV_MIN64_STEP
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned afv_wave_min_u32(unsigned v) {
#define AFV_MIN32_STEP(ctrl, rmask) v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, ctrl, rmask, 0xf, false));
    AFV_DPP_REDUCE64(AFV_MIN32_STEP)
#undef AFV_MIN32_STEP
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// a double of lane `src` (wave-uniform, usually a compile-time constant) for every lane, through scalar registers: two v_readlane, no
// LDS crossbar.  What one lane computed is handed to all of them this way (k_sim3opt.hip: the perturbed estimates of a linearisation).
__device__ __forceinline__ double afv_wave_read_f64(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// ---------------- the rotation histogram of FeatureMatcher.cc ----------------
// the bin of a match (FeatureMatcher.cc:1587-1599), rotFactor = 1/30 (:1579-1585)
__device__ __forceinline__ int afv_rotation_bin(float a1, float a2) {
    const float rot_factor = 1.0f / 30.0f;
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * rot_factor);
    if (bin == 30) bin = 0;
    return bin;
}

// computeThreeMaxima with the 0.1 cut (FeatureMatcher.cc:1631-1668) over the 30 bins of hist: the three dominant bins, -1 for one that is cut.
// Ties keep the earlier bin (strict >).  A match survives iff its bin is one of the three.
struct AfvMaxima3 {
    int i1, i2, i3;
};
__device__ __forceinline__ AfvMaxima3 afv_three_maxima(const int *hist) {
    int i1 = -1, i2 = -1, i3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < 30; ++i) {
        const int sz = hist[i];
        if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; i3 = i2; i2 = i1; i1 = i; }
        else if (sz > max2) { max3 = max2; max2 = sz; i3 = i2; i2 = i; }
        else if (sz > max3) { max3 = sz; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
    return AfvMaxima3{i1, i2, i3};
}

// Hamming distance over W dwords
template <int W>
__device__ __forceinline__ int afv_hamming(const uint32_t *a, const uint32_t *b) {
    int d = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) d += __popc(a[i] ^ b[i]);
    return d;
}

// ---------------- workgroup scaffolding of the fixed-point engines ----------------
// All three engines run on AFV_FP_T threads, a thread per live row / query.  The LDS scratch words belong to the caller (the functions
// below hold no __shared__ of their own): s_cntw[AFV_FP_NW], s_first, s_wlist[AFV_FP_WLIST], s_vote[3] and the flag bytes of the live rows
// (1 = asked for a rescan in the last pass, 2 = pinned by a rescan).
#define AFV_FP_T 1024                 // threads: one per live row
#define AFV_FP_NW (AFV_FP_T / 64)
#define AFV_FP_INF 0x7fffffff
#define AFV_FP_WLIST 128              // waiting rows looked at per convergence
#define AFV_FP_GUARD (-0x7fffffff)    // the match count reported when the pass guard trips (never observed; the host turns it into AFV_EHIP)

// "did any thread change something in this pass": ONE barrier.  Three rotating flags (the pass that writes flag p % 3 clears the one the
// pass after next will use): __syncthreads_or goes through the device library's workgroup reduction (an LDS round plus two barriers).
__device__ __forceinline__ bool afv_wg_any_changed(bool changed, int pass, int *s_vote) {
    if (__ballot(changed) && (threadIdx.x & 63) == 0) s_vote[pass % 3] = 1;
    __syncthreads();
    const bool any = s_vote[pass % 3] != 0;
    if (threadIdx.x == 0) s_vote[(pass + 2) % 3] = 0;
    return any;
}

// Ordered compaction: the threads with `pred` get consecutive slots from `base` on IN THREAD ORDER (ballot, the 16 wavefronts' counts
// meet in s_cntw behind one barrier, every thread adds up the counts before its wavefront and the set lanes below its own).  total = the
// threads with pred.  The caller puts a barrier before s_cntw is written again.
struct AfvSlot {
    int slot, total;
};
__device__ __forceinline__ AfvSlot afv_wg_ordered_slot(bool pred, int base, int *s_cntw) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(pred);
    if (lane == 0) s_cntw[wv] = __popcll(m);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int w = 0; w < AFV_FP_NW; ++w) {
        const int cw = s_cntw[w];
        off += w < wv ? cw : 0;
        tot += cw;
    }
    const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
    return AfvSlot{slot, tot};
}

// After convergence: the live rows that asked for a rescan, in order, into s_wlist.  Live row t < 1024 is held by thread t, so the first
// 1024 live rows are looked at per cycle (nwait of them wait, the first AFV_FP_WLIST are listed); only when none of them waits are the rows
// behind them searched, and then ONE is listed: the first (rare, slow, exact).  nw = entries of s_wlist to rescan.
// The barrier ahead of the search keeps thread 0 from overwriting s_first while other wavefronts still read nwait from it.
struct AfvWaiting {
    int nwait, nw;
};
__device__ __forceinline__ AfvWaiting afv_wg_collect_waiting(const uint8_t *s_flag, int nlive, int *s_cntw, int *s_first, unsigned short *s_wlist) {
    const int tid = threadIdx.x;
    {
        const bool waits = tid < nlive && (s_flag[tid] & 3) == 1;
        const AfvSlot S = afv_wg_ordered_slot(waits, 0, s_cntw);
        if (waits && S.slot < AFV_FP_WLIST) s_wlist[S.slot] = (unsigned short)tid;
        if (tid == 0) *s_first = S.total;
        __syncthreads();
    }
    const int nwait = *s_first;
    int nw = min(nwait, AFV_FP_WLIST);
    if (nw == 0 && nlive > AFV_FP_T) {
        __syncthreads();
        if (tid == 0) *s_first = AFV_FP_INF;
        __syncthreads();
        int mine = AFV_FP_INF;
        for (int li = AFV_FP_T + tid; li < nlive; li += AFV_FP_T)
            if ((s_flag[li] & 3) == 1) mine = min(mine, li);
        if (mine != AFV_FP_INF) atomicMin(s_first, mine);
        __syncthreads();
        if (*s_first != AFV_FP_INF) {
            if (tid == 0) s_wlist[0] = (unsigned short)*s_first;
            nw = 1;
        }
        __syncthreads();
    }
    return AfvWaiting{nwait, nw};
}

// The rescans of one step left their answers in s_part[0 .. N) (-1 = takes nothing), entry w for waiting row g0 + w.  They are adopted in
// order up to and including the first that took something: a rescan that ends in "no match" changes nothing for anybody behind it, one
// that takes a feature invalidates the answers behind it.  Every thread computes the same verdict.
struct AfvAdopt {
    int nadopt;
    bool took;
};
template <int N>
__device__ __forceinline__ AfvAdopt afv_wg_adopt_verdict(const int *s_part, int g0, int nw) {
    int nadopt = 0;
    bool took = false;
#pragma unroll
    for (int w = 0; w < N; ++w) {
        if (g0 + w < nw && !took) {
            ++nadopt;
            took = s_part[w] >= 0;
        }
    }
    return AfvAdopt{nadopt, took};
}

// the tail's count: every thread's cnt added into *s_nm (zeroed behind a barrier by the caller), one LDS atomic per wavefront
__device__ __forceinline__ void afv_wg_add_count(int cnt, int *s_nm) {
    cnt = afv_wave_incl_scan(cnt);
    if ((threadIdx.x & 63) == 63 && cnt) atomicAdd(s_nm, cnt);
}
