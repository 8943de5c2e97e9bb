// k_bowvec.hip — the BowVector and DBoW2's L1 score on the device: the arithmetic under KeyFrameDatabase::DetectLoopCandidates /
// DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:76-309), Vocabulary::score (src/Vocabulary.cpp:132-153) and the minScore loop
// of LoopClosing.cc:137-157.  DBoW2 is an empty submodule in the reference; BowVector::addWeight / normalize(L1) and L1Scoring::score
// follow upstream DBoW2 — parity unpinned, like the descent of k_bow.hip.
//
// Both results are defined to the bit by the ORDER of their double additions, so the sums are sequential by contract:
//   * a BowVector value is weight[w] added once per feature of the word (all addends equal: only the count matters, not which features),
//     the norm is the sum of fabs(value) in ascending word order;
//   * a score is the sum of fabs(v - w) - fabs(v) - fabs(w) over the shared words in ascending word order.
// The parallel part is everything around the sums: sorting the words of a frame, finding the shared words of a pair.
#include "afv_device.h"
#include "afv_runtime.h"  // the launchers below are declared there
#include "afv_jobs.h"

#define BV_NONE 0x7fffffff
#define BV_THREADS 1024

// One workgroup per BowVector: the word ids of the features that count (weight > 0) are sorted in LDS, the head of every run of equal
// ids becomes an entry, its value the repeated addition over the run.
__global__ __launch_bounds__(BV_THREADS) void k_bowvec_build(const int *__restrict__ leaf, int n, const double *__restrict__ weight,
                                                             const int32_t *__restrict__ word_id, const double *__restrict__ word_weight,
                                                             int32_t *out_word, double *out_value, int *__restrict__ out_n) {
    __shared__ int s_key[AFV_BOW_MAX_ENTRIES];
    __shared__ int s_scan[BV_THREADS];
    __shared__ double s_chunk[BV_THREADS];
    __shared__ double s_norm;
    const int tid = threadIdx.x;
    int P = 64;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += BV_THREADS) {
        int key = BV_NONE;
        if (i < n) {
            const int lf = leaf[i];
            const int id = word_id[lf];
            if (weight[lf] > 0 && id >= 0) key = id;  // DBoW2 transform: if(w > 0) addWeight
        }
        s_key[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += BV_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const int a = s_key[i], b = s_key[o];
                    if ((a > b) == ((i & k) == 0)) {
                        s_key[i] = b;
                        s_key[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    // entry position = number of run heads in front: every thread owns a contiguous stretch of the sorted keys
    const int per = (P + BV_THREADS - 1) / BV_THREADS, i0 = min(tid * per, P), i1 = min(i0 + per, P);
    int heads = 0;
    for (int i = i0; i < i1; ++i) heads += s_key[i] != BV_NONE && (i == 0 || s_key[i] != s_key[i - 1]);
    s_scan[tid] = heads;
    __syncthreads();
    for (int d = 1; d < BV_THREADS; d <<= 1) {
        const int add = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const int m = s_scan[BV_THREADS - 1];
    int pos = s_scan[tid] - heads;
    for (int i = i0; i < i1; ++i) {
        const int key = s_key[i];
        if (key == BV_NONE || (i > 0 && key == s_key[i - 1])) continue;
        int cnt = 1;
        while (i + cnt < P && s_key[i + cnt] == key) ++cnt;
        // BowVector::addWeight once per feature: repeated addition (count * weight differs from the 4th addition on)
        const double w = word_weight[key];
        double v = w;
        for (int c = 1; c < cnt; ++c) v += w;
        out_word[pos] = key;
        out_value[pos] = v;
        ++pos;
    }
    __syncthreads();  // the values are read back below by other threads of this workgroup
    // BowVector::normalize(L1): norm = sum of fabs(value), sequential in ascending word order (one lane; the others stage the values)
    if (tid == 0) s_norm = 0.0;
    for (int c0 = 0; c0 < m; c0 += BV_THREADS) {
        __syncthreads();
        if (c0 + tid < m) s_chunk[tid] = out_value[c0 + tid];
        __syncthreads();
        if (tid == 0) {
            double s = s_norm;
            const int e = min(BV_THREADS, m - c0);
            for (int j = 0; j < e; ++j) s += fabs(s_chunk[j]);
            s_norm = s;
        }
    }
    __syncthreads();
    const double norm = s_norm;
    if (norm > 0.0)
        for (int i = tid; i < m; i += BV_THREADS) out_value[i] = out_value[i] / norm;
    if (tid == 0) *out_n = m;
}

extern "C" void afv_launch_bowvec_build(const int *leaf, int n, const double *weight, const int32_t *word_id, const double *word_weight,
                                        int32_t *out_word, double *out_value, int *out_n, hipStream_t stream) {
    hipLaunchKernelGGL(k_bowvec_build, dim3(1), dim3(BV_THREADS), 0, stream, leaf, n, weight, word_id, word_weight, out_word, out_value, out_n);
}

// ---------------- L1 scores of queries against the slots of the keyframe table ----------------
// Grid (slot groups, queries): the workgroup's four wavefronts share ONE query whose word ids sit in LDS; a wavefront takes a slot at a
// time.  Lanes take the slot's words 64 at a time and binary-search the query list (<= 13 steps).  Shared words: their number by ballot +
// popcount, the smallest by the first set lane (the slot's words ascend).  The terms are added in lane order = ascending word order, each
// read from its lane into a scalar and added on every lane alike: the running sum is wave-uniform and no lane waits for LDS.
#define SB_THREADS 256
__global__ __launch_bounds__(SB_THREADS) void k_score_bow(const DevBowQuery *__restrict__ Q, const int32_t *__restrict__ bow_word,
                                                          const double *__restrict__ bow_value, const int32_t *__restrict__ bow_n,
                                                          const uint8_t *__restrict__ slot_state, int nsets, int cap, int slots_per_wg,
                                                          int32_t *__restrict__ common, double *__restrict__ score,
                                                          int32_t *__restrict__ first_common) {
    __shared__ int s_qw[AFV_BOW_MAX_ENTRIES];
    const DevBowQuery q = Q[blockIdx.y];
    const int qn = min(max(q.n, 0), AFV_BOW_MAX_ENTRIES);
    for (int i = threadIdx.x; i < qn; i += SB_THREADS) s_qw[i] = q.word[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s_begin = blockIdx.x * slots_per_wg, s_end = min(s_begin + slots_per_wg, nsets);
    for (int slot = s_begin + wave; slot < s_end; slot += SB_THREADS / 64) {
        const size_t o = (size_t)blockIdx.y * nsets + slot;
        if (!slot_state[slot]) {  // empty, masked out or without BowVector
            if (lane == 0) {
                common[o] = -1;
                score[o] = 0.0;
                if (first_common) first_common[o] = -1;
            }
            continue;
        }
        const int ns = min(max(bow_n[slot], 0), cap);
        const int32_t *sw = bow_word + (size_t)slot * cap;
        const double *sv = bow_value + (size_t)slot * cap;
        int cnt = 0, fc = -1;
        double s = 0.0;
        for (int base = 0; base < ns; base += 64) {
            const int i = base + lane;
            bool found = false;
            int w = 0;
            double term = 0.0;
            if (i < ns) {
                w = sw[i];
                int lo = 0, hi = qn;  // first query word >= w
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_qw[mid] < w) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < qn && s_qw[lo] == w) {
                    found = true;
                    const double v = q.value[lo], x = sv[i];
                    term = fabs(v - x) - fabs(v) - fabs(x);  // L1Scoring::score, left to right
                }
            }
            unsigned long long mask = __ballot(found);
            if (!mask) continue;
            if (fc < 0) fc = __builtin_amdgcn_readlane(w, (int)__ffsll((long long)mask) - 1);
            cnt += __popcll(mask);
            const int t_lo = __double2loint(term), t_hi = __double2hiint(term);
            while (mask) {
                const int l = (int)__ffsll((long long)mask) - 1;
                mask &= mask - 1;
                s += __hiloint2double(__builtin_amdgcn_readlane(t_hi, l), __builtin_amdgcn_readlane(t_lo, l));
            }
        }
        if (lane == 0) {
            common[o] = cnt;
            score[o] = cnt ? -s / 2.0 : 0.0;
            if (first_common) first_common[o] = fc;
        }
    }
}

extern "C" void afv_launch_score_bow(const DevBowQuery *q, int nq, const int32_t *bow_word, const double *bow_value, const int32_t *bow_n,
                                     const uint8_t *slot_state, int nsets, int cap, int32_t *common, double *score, int32_t *first_common,
                                     hipStream_t stream) {
    if (nq < 1 || nsets < 1) return;
    // one slot per wavefront while that still fills the chip; larger batches amortise the query's trip into LDS over more slots
    long per = ((long)nq * nsets) / 4096;
    per = std::min<long>(std::max<long>(per, 4), 64) & ~3L;
    const int slots_per_wg = (int)per;
    dim3 grid((nsets + slots_per_wg - 1) / slots_per_wg, nq);
    hipLaunchKernelGGL(k_score_bow, grid, dim3(SB_THREADS), 0, stream, q, bow_word, bow_value, bow_n, slot_state, nsets, cap, slots_per_wg, common,
                       score, first_common);
}
