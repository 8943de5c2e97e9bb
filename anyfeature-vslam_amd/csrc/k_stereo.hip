// k_stereo.hip — Frame::ComputeStereoMatches (src/Frame.cc:465-645) and Frame::ComputeStereoFromRGBD (:648-669) on resident frames.
//
// The semantics are those of tests/_stereo_ref.py (the reference's routine with deviations A, B, C: include/afv_hip.h), bit for bit.
// A job is small (about 1000 x 1000 predicates, at most 1000 windows) and latency-bound, so a stereo match is two launches and no host round trip
// (the RGB-D gather is a launch of its own call):
//   1. k_stereo_match — one WAVE per left keypoint.  The workgroup stages the right side as (minr, maxr, x, octave) in LDS, 128 keypoints
//      at a time; the lanes stride over iR and test the row band, the octave and the u range directly - the predicate "minr <= row <= maxr"
//      IS the row table of :485-498, so none is built.  A descriptor distance is evaluated only where the predicates pass; the wave reduces
//      on the key (distance bits << 32 | iR): the ordered walk's strict `<` keeps the lowest iR among equals.  The same wave goes on to the
//      SAD: lanes own pixels of the 11 x 11 window and accumulate the 11 offsets in integers, a butterfly adds them up, every lane then
//      runs the float tail (parabola, disparity gates) in plain C++ (the library is built with contraction off) and lane 0 stores.
//   2. k_stereo_median — one workgroup: k-th smallest SAD by a two-pass radix select over LDS histograms (the SADs are < 2^16), then the
//      per-element test (float)SAD >= 1.5f * 1.4f * median.
//   3. k_stereo_rgbd — the depth gather, one thread per feature.
#include "afv_device.h"
#include "afv_wave.h"
#include "afv_runtime.h"  // the launchers below are declared there: a signature that drifts is a compile error

#define ST_THREADS 256
#define ST_WAVES (ST_THREADS / AFV_WAVE)
#define ST_CHUNK 128  // right keypoints staged at a time (2 KB of LDS)
#define ST_W 5  // Frame.cc:567 w
#define ST_L 5  // :574 L
#define ST_NO_KEY 0xffffffffffffffffull
#define ST_COORD_MAX 1048576.0f

// FeatureMatcher::DescriptorDistance as the matchers evaluate it (k_project.hip): popcount over the zero-padded dwords of a binary row ...
__device__ __forceinline__ int stereo_hamming(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int words) {
    int d = 0;
    for (int i = 0; i < words; i += 4) {
        const uint4 x = *reinterpret_cast<const uint4 *>(a + i), y = *reinterpret_cast<const uint4 *>(b + i);
        d += __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
    }
    return d;
}
// ... and L2^2 of float rows in the accumulation order of proj_l2sqr (k_project.hip) / k_match_l2.hip: float differences, squares and
// 4-way partial sums in double, one rounding to float at the end
__device__ __forceinline__ float stereo_l2sqr(const float *__restrict__ a, const float *__restrict__ b, int dim) {
    double s = 0;
    for (int i = 0; i < dim; i += 4) {
        const float4 x = *reinterpret_cast<const float4 *>(a + i), y = *reinterpret_cast<const float4 *>(b + i);
        const double v0 = (double)(x.x - y.x), v1 = (double)(x.y - y.y), v2 = (double)(x.z - y.z), v3 = (double)(x.w - y.w);
        s += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
    }
    return (float)s;
}

__device__ __forceinline__ unsigned long long stereo_wave_min(unsigned long long v) {
#pragma unroll
    for (int m = 1; m < AFV_WAVE; m <<= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int stereo_wave_sum(int v) {
#pragma unroll
    for (int m = 1; m < AFV_WAVE; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// an end of a right keypoint's row band as an int: clamped to +-2^30 before the conversion, a NaN end becomes -2^30 (fmaxf returns the
// other operand), which empties the band (minr <= row needs row >= 0; row <= maxr fails)
__device__ __forceinline__ int stereo_band_end(float v) { return (int)fminf(fmaxf(v, -1073741824.0f), 1073741824.0f); }
// a scaled window coordinate the int gates may see: finite and within +-2^20 (no level is wider than 8192, so nothing is lost)
__device__ __forceinline__ bool stereo_coord_ok(float v) { return v >= -ST_COORD_MAX && v <= ST_COORD_MAX; }

__global__ __launch_bounds__(ST_THREADS) void k_stereo_match(const DevStereoJob J) {
    __shared__ int4 s_r[ST_CHUNK];  // (minr, maxr, x bits, octave) of the staged right keypoints
    const int tid = threadIdx.x, lane = tid & (AFV_WAVE - 1), wv = tid / AFV_WAVE;
    const int iL = blockIdx.x * ST_WAVES + wv;
    const bool have = iL < J.n_l;

    float uL = 0.f, vL = 0.f, sizeL = 1.f;
    int levelL = 0, row = -1;
    if (have) {
        const afv_keypoint kp = J.kps_l[iL];
        uL = kp.x;
        vL = kp.y;
        levelL = kp.octave;
        sizeL = J.size_l[iL];
        // :516 vRowIndices[vL]: truncation.  Only a y inside (-1, nRows) is converted (it truncates to a row of the table; NaN fails both tests)
        if (vL > -1.0f && vL < (float)J.n_rows) row = (int)vL;
    }
    const float min_u = uL - J.max_d;  // :521
    const float max_u = uL - 0.0f;     // :522 (minD = 0)
    // deviation B (the left keypoint's own row), :524 maxU < 0
    const bool search = have && row >= 0 && row < J.n_rows && !(max_u < 0.0f);

    unsigned long long best_key = ST_NO_KEY;
    bool in_row = false;
    for (int base = 0; base < J.n_r; base += ST_CHUNK) {  // (block-uniform trip count: every wave meets every barrier)
        const int cnt = min(ST_CHUNK, J.n_r - base);
        __syncthreads();
        for (int j = tid; j < cnt; j += ST_THREADS) {
            const afv_keypoint kr = J.kps_r[base + j];
            const float r = 2.0f * J.size_r[base + j];  // deviation A: the right keypoint's own size
            const float top = kr.y + r, bot = kr.y - r;
            s_r[j] = make_int4(stereo_band_end(floorf(bot)), stereo_band_end(ceilf(top)), __float_as_int(kr.x), kr.octave);  // :493-494
        }
        __syncthreads();
        if (search) {
            for (int j = lane; j < cnt; j += AFV_WAVE) {
                const int4 e = s_r[j];
                if (row < e.x || row > e.y) continue;  // :496-497: iR is in row `row` of the table
                in_row = true;
                if (e.w < levelL - 1 || e.w > levelL + 1) continue;  // :538
                const float uR = __int_as_float(e.z);
                if (!(uR >= min_u && uR <= max_u)) continue;  // :543
                const int iR = base + j;
                float d;
                if (J.fdim) d = stereo_l2sqr(reinterpret_cast<const float *>(J.desc_l) + (size_t)iL * J.fdim, reinterpret_cast<const float *>(J.desc_r) + (size_t)iR * J.fdim, J.fdim);
                else d = (float)stereo_hamming(J.desc_l + (size_t)iL * J.words, J.desc_r + (size_t)iR * J.words, J.words);
                if (d < J.th_high) {  // :548 against the starting value; among these the smallest (distance, iR) is what the walk keeps
                    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)iR;
                    best_key = key < best_key ? key : best_key;
                }
            }
        }
    }
    if (!have) return;  // (no barrier below)

    float out_ur = -1.0f, out_depth = -1.0f;
    int out_sad = -1, out_r = -1;
    do {
        if (!search) break;
        if (!__any(in_row)) break;  // :518 vCandidates.empty()
        best_key = stereo_wave_min(best_key);
        const bool found = best_key != ST_NO_KEY;
        const float best = found ? __uint_as_float((unsigned)(best_key >> 32)) : J.th_high;  // :527
        const int idx_r = found ? (int)(unsigned)(best_key & 0xffffffffu) : 0;               // :528 bestIdxR = 0
        if (!(best < J.th_orb)) break;  // :557
        out_r = idx_r;
        const float uR0 = J.kps_r[idx_r].x;            // :560
        const float s = 1.0f / sizeL;                  // :561
        const float fu = roundf(uL * s), fv = roundf(vL * s), fu0 = roundf(uR0 * s);  // :562-564
        // a zero / denormal / NaN size or a huge coordinate: the scaled coordinate is not one of any level; checked as floats, so that the
        // int gates below cannot overflow
        if (!(stereo_coord_ok(fu) && stereo_coord_ok(fv) && stereo_coord_ok(fu0))) break;
        const int su = (int)fu, sv = (int)fv, su0 = (int)fu0;
        if (levelL < 0 || levelL >= J.nlevels) break;  // deviation C: no such level
        const int w = J.lw[levelL], h = J.lh[levelL];
        if (su0 < 0 || su0 + ST_L + ST_W + 1 >= w) break;  // :578-581 iniu < 0 || endu >= cols
        if (sv - ST_W < 0 || sv + ST_W >= h || su - ST_W < 0 || su + ST_W >= w || su0 - ST_L - ST_W < 0) break;  // deviation C
        const uint8_t *__restrict__ imL = J.pyr_l[levelL], *__restrict__ imR = J.pyr_r[levelL];
        const int lc = imL[(size_t)sv * w + su];
        int rc[2 * ST_L + 1], acc[2 * ST_L + 1];
#pragma unroll
        for (int k = 0; k <= 2 * ST_L; ++k) {
            rc[k] = imR[(size_t)sv * w + su0 + k - ST_L];
            acc[k] = 0;
        }
        for (int p = lane; p < (2 * ST_W + 1) * (2 * ST_W + 1); p += AFV_WAVE) {
            const int py = p / (2 * ST_W + 1), dy = py - ST_W, dx = p - py * (2 * ST_W + 1) - ST_W;
            const size_t ro = (size_t)(sv + dy) * w;
            const int a = (int)imL[ro + su + dx] - lc;
            const uint8_t *rrow = imR + ro + su0 + dx - ST_L;
#pragma unroll
            for (int k = 0; k <= 2 * ST_L; ++k) {
                const int b = (int)rrow[k] - rc[k];
                acc[k] += abs(a - b);
            }
        }
        int best_sad = 0x7fffffff, best_inc = 0;  // :572-573
        float d1 = 0.f, d2 = 0.f, d3 = 0.f;
        int prev = 0, at = 0;
#pragma unroll
        for (int k = 0; k <= 2 * ST_L; ++k) {
            const int d = stereo_wave_sum(acc[k]);
            if (at == 1) {  // the offset right after the current best
                d3 = (float)d;
                at = 2;
            }
            if (d < best_sad) {  // :590 strict: the first of equal offsets stays
                best_sad = d;
                best_inc = k - ST_L;
                d1 = (float)prev;
                d2 = (float)d;
                at = 1;
            }
            prev = d;
        }
        if (best_inc == -ST_L || best_inc == ST_L) break;  // :599
        const float num = d1 - d3, s13 = d1 + d3, two_d2 = 2.0f * d2, den = s13 - two_d2, den2 = 2.0f * den;
        const float delta = num / den2;  // :607
        if (delta < -1.0f || delta > 1.0f) break;  // :609
        const float t0 = (float)su0 + (float)best_inc, t1 = t0 + delta;
        float best_u = sizeL * t1;       // :613
        float disparity = uL - best_u;   // :615
        if (!(disparity >= 0.0f && disparity < J.max_d)) break;  // :617
        if (disparity <= 0.0f) {         // :619-623
            disparity = 0.01f;
            best_u = (float)((double)uL - 0.01);
        }
        out_depth = J.mbf / disparity;   // :624
        out_ur = best_u;                 // :625
        out_sad = best_sad;
    } while (false);
    if (lane == 0) {
        J.u_right[iL] = out_ur;
        J.depth[iL] = out_depth;
        J.sad[iL] = out_sad;
        J.best_r[iL] = out_r;
    }
}

// the k-th smallest (k counted from 0) of the histogram in s_hist[256], on wave 0: the bin and k's rank inside it
__device__ __forceinline__ void stereo_pick_bin(const int *s_hist, int k, int lane, int *s_bin, int *s_rank) {
    const int h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
    const int c = h0 + h1 + h2 + h3;
    const int incl = afv_wave_incl_scan(c), excl = incl - c;
    if (k >= excl && k < incl) {  // exactly one lane
        int r = k - excl, b = 0;
        if (r >= h0) { r -= h0; b = 1;
            if (r >= h1) { r -= h1; b = 2;
                if (r >= h2) { r -= h2; b = 3; } } }
        *s_bin = 4 * lane + b;
        *s_rank = r;
    }
}

#define SM_THREADS 1024
__global__ __launch_bounds__(SM_THREADS) void k_stereo_median(float *__restrict__ u_right, float *__restrict__ depth, const int *__restrict__ sad, int n,
                                                              int *__restrict__ n_stereo) {
    __shared__ int s_hist[256];
    __shared__ int s_bin, s_rank, s_total, s_kept;
    const int tid = threadIdx.x;
    if (tid < 256) s_hist[tid] = 0;
    if (tid == 0) {
        s_total = 0;
        s_kept = 0;
        s_bin = 0;
        s_rank = 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += SM_THREADS) {  // pass 1: the high byte (a SAD is <= 61 710)
        const int s = sad[i];
        if (s >= 0) {
            atomicAdd(&s_hist[(s >> 8) & 255], 1);
            atomicAdd(&s_total, 1);
        }
    }
    __syncthreads();
    const int total = s_total;
    if (total == 0) {  // no accepted pair: nothing to do (the reference indexes an empty vector, :632)
        if (tid == 0) *n_stereo = 0;
        return;
    }
    if (tid < AFV_WAVE) stereo_pick_bin(s_hist, total / 2, tid, &s_bin, &s_rank);  // :632 vDistIdx[size / 2]
    __syncthreads();
    const int hi = s_bin, rank = s_rank;
    __syncthreads();
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += SM_THREADS) {  // pass 2: the low byte among the SADs of that high byte
        const int s = sad[i];
        if (s >= 0 && ((s >> 8) & 255) == hi) atomicAdd(&s_hist[s & 255], 1);
    }
    __syncthreads();
    if (tid < AFV_WAVE) stereo_pick_bin(s_hist, rank, tid, &s_bin, &s_rank);
    __syncthreads();
    const float median = (float)((hi << 8) | s_bin);
    const float k21 = 1.5f * 1.4f;
    const float th_dist = k21 * median;  // :633
    for (int i = tid; i < n; i += SM_THREADS) {
        const int s = sad[i];
        if (s < 0) continue;
        if ((float)s >= th_dist) {  // :635-644: the walk from the top of the sorted pairs is this test per pair
            u_right[i] = -1.0f;
            depth[i] = -1.0f;
        } else {
            atomicAdd(&s_kept, 1);
        }
    }
    __syncthreads();
    if (tid == 0) *n_stereo = s_kept;
}

__global__ void k_stereo_rgbd(const afv_keypoint *__restrict__ kps, const float *__restrict__ x_un, int n, const float *__restrict__ img, int w, int h,
                              float mbf, float *__restrict__ u_right, float *__restrict__ depth) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const afv_keypoint kp = kps[i];
    const int r = (int)kp.y, c = (int)kp.x;  // :661 imDepth.at<float>(v, u): truncation
    float ur = -1.0f, dp = -1.0f;
    if (r >= 0 && r < h && c >= 0 && c < w) {
        const float d = img[(size_t)r * w + c];
        if (d > 0.0f) {  // :663
            const float q = mbf / d;
            dp = d;
            ur = x_un[i] - q;  // :666
        }
    }
    u_right[i] = ur;
    depth[i] = dp;
}

extern "C" void afv_launch_stereo_match(const DevStereoJob *job, hipStream_t stream) {
    if (job->n_l < 1) return;
    hipLaunchKernelGGL(k_stereo_match, dim3((job->n_l + ST_WAVES - 1) / ST_WAVES), dim3(ST_THREADS), 0, stream, *job);
}
extern "C" void afv_launch_stereo_median(float *u_right, float *depth, const int *sad, int n, int *n_stereo, hipStream_t stream) {
    hipLaunchKernelGGL(k_stereo_median, dim3(1), dim3(SM_THREADS), 0, stream, u_right, depth, sad, n, n_stereo);
}
extern "C" void afv_launch_stereo_rgbd(const afv_keypoint *kps, const float *x_un, int n, const float *img, int w, int h, float mbf, float *u_right,
                                       float *depth, hipStream_t stream) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_stereo_rgbd, dim3((n + 255) / 256), dim3(256), 0, stream, kps, x_un, n, img, w, h, mbf, u_right, depth);
}
