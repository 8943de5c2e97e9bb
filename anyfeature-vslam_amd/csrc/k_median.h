// k_median.h - the m-th smallest entry of a row of descriptor distances without sorting or storing the row, as
// MapPoint::ComputeDistinctiveDescriptors needs it (src/MapPoint.cc:329-333: the row sorted, entry floor(0.5 (N - 1)) taken).  One copy
// of the program text for the kernels that run it: k_distinctive / k_distinctive_f32 (k_match.hip: rows uploaded by the host) and
// k_refresh_desc (k_refresh.hip: rows addressed through (slot, idx) in the keyframe table).
#pragma once
#include "afv_wave.h"

// A lane per row.  The smallest key v in [lo, hi] with #{j : key(d(i, j)) <= v} > m  <=>  the m-th smallest (0-based) distance of row i.
// The keys are Hamming distances (lo = 0, hi = 8 * bytes: <= 10 steps) or the bit patterns of non-negative floats, which order like the
// numbers (lo = 0, hi = the bits of +inf: <= 31 steps).  count_le(mid) = #{j : key(d(i, j)) <= mid} of the calling lane's row; every
// lane of the wavefront calls it in every step (a lane whose interval has closed keeps its answer), so it may hold wave-uniform loads.
template <class CountLE>
__device__ __forceinline__ unsigned afv_bisect_mth(unsigned lo, unsigned hi, int m, CountLE count_le) {
    while (__any(lo < hi)) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        const int cnt = count_le(mid);
        if (lo < hi) {
            if (cnt > m) hi = mid;
            else lo = mid + 1u;
        }
    }
    return lo;
}

// the least median over the lanes, then the first row that has it (strict <, :333): {median key, row}; rows ascend inside a lane, so a
// lane keeps its first row on a tie by taking a later one only on a strictly smaller median
struct AfvBestRow {
    unsigned median, row;
};
__device__ __forceinline__ AfvBestRow afv_wave_best_row(unsigned best_med, unsigned best_row) {
    const unsigned gm = afv_wave_min_u32(best_med);
    const unsigned gr = afv_wave_min_u32(best_med == gm ? best_row : 0xffffffffu);
    return AfvBestRow{gm, gr};
}
