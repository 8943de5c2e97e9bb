// refresh_host.cpp — MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth as tests/_refresh_ref.py restates them,
// as a scalar host program over plain arrays: what a host does today for every point a bundle adjustment moved.  tools/time_refresh.py
// times it against afv_table_refresh_points and tests/test_refresh_ref_cpu.py holds it to the restatement bit for bit.
// Build: g++ -O3 -ffp-contract=off -std=c++17 -shared -fPIC (the tests, the timing tool), or -DREFRESH_HOST_MAIN for a stand-alone program
// on a small constructed scene.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

enum { RF_DONE = 0, RF_SKIPPED = 1, RF_NO_OBSERVATIONS = 2, RF_NO_REF = 3, RF_BAD_DISTANCE = 4 };
enum { PTF_SET = 1, PTF_BAD = 2 };

int hamming(const uint8_t *a, const uint8_t *b, int bytes) {  // pad bytes are not part of a row
    int d = 0;
    for (int i = 0; i < bytes; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

float l2sqr(const float *a, const float *b, int n) {  // normL2Sqr<float, double>, narrowed
    double s = 0;
    int i = 0;
    for (; i <= n - 4; i += 4) {
        const double v0 = (double)(a[i] - b[i]), v1 = (double)(a[i + 1] - b[i + 1]), v2 = (double)(a[i + 2] - b[i + 2]), v3 = (double)(a[i + 3] - b[i + 3]);
        s += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
    }
    for (; i < n; ++i) {
        const double v = (double)(a[i] - b[i]);
        s += v * v;
    }
    return (float)s;
}

float dist3(const float *X, const float *O, float *n) {  // |X - O| = sqrt(a0 + (a1 + a2))
    n[0] = X[0] - O[0]; n[1] = X[1] - O[1]; n[2] = X[2] - O[2];
    return sqrtf(n[0] * n[0] + (n[1] * n[1] + n[2] * n[2]));
}

// MapPoint.cc:311-340 over the N good rows: the matrix, per row the sort, strict <
template <class T, class Dist>
int least_median_row(int N, Dist dist, T *median_out) {
    std::vector<T> D((size_t)N * N, T(0));
    for (int i = 0; i < N; ++i)
        for (int j = i + 1; j < N; ++j) D[(size_t)i * N + j] = D[(size_t)j * N + i] = dist(i, j);
    int best = 0;
    bool have = false;
    T best_median = T(0);
    std::vector<T> v((size_t)N);
    for (int i = 0; i < N; ++i) {
        std::copy(D.begin() + (size_t)i * N, D.begin() + (size_t)(i + 1) * N, v.begin());
        std::sort(v.begin(), v.end());
        const T median = v[(size_t)(0.5 * (N - 1))];
        if (!have || median < best_median) {
            best_median = median;
            best = i;
            have = true;
        }
    }
    *median_out = best_median;
    return best;
}

}  // namespace

// The table: rows [nslots][cap][pitch bytes], sigma2 / size [nslots][cap].  The call: the arrays of afv_table_refresh_points with pt_ptr
// [np + 1] in place of obs_point.  The store: SoA over its capacity, pos / normal [capacity][3], rows [capacity][pitch bytes].
extern "C" void refresh_host(int cap, int pitch, int desc_bytes, int float_dim, const uint8_t *rows, const float *sigma2, const float *size, int nk,
                             const int32_t *slots, const float *centres, const float *max_size, const uint8_t *kf_bad, int np, const int32_t *point_ids,
                             const int32_t *ref_kf, const int32_t *pt_ptr, const int32_t *obs_kf, const int32_t *obs_idx, int descriptors, int normals,
                             const float *pos, float *normal, float *min_d, float *max_d, float *ref_size, float *ref_dist, float *ref_sigma,
                             const uint8_t *flags, uint8_t *store_rows, int32_t *status, int32_t *best_obs, int32_t *best_median) {
    (void)nk;
    std::vector<int> good;
    for (int p = 0; p < np; ++p) {
        const int id = point_ids[p], b = pt_ptr[p], n = pt_ptr[p + 1] - b;
        status[p] = RF_DONE;
        best_obs[p] = -1;
        best_median[p] = 0;  // R3
        if (!(flags[id] & PTF_SET) || (flags[id] & PTF_BAD)) {
            status[p] = RF_SKIPPED;
            continue;
        }
        if (n == 0) {
            status[p] = RF_NO_OBSERVATIONS;
            continue;
        }
        auto row_of = [&](int e) { return rows + ((size_t)slots[obs_kf[e]] * cap + obs_idx[e]) * pitch; };
        if (descriptors) {
            good.clear();
            for (int e = b; e < b + n; ++e)
                if (!(kf_bad && kf_bad[obs_kf[e]])) good.push_back(e);
            const int N = (int)good.size();
            if (N > 0) {
                int best;
                if (float_dim) {
                    float med;
                    best = least_median_row<float>(N, [&](int i, int j) {
                        return l2sqr(reinterpret_cast<const float *>(row_of(good[i])), reinterpret_cast<const float *>(row_of(good[j])), float_dim);
                    }, &med);
                    std::memcpy(&best_median[p], &med, 4);
                } else {
                    int med;
                    best = least_median_row<int>(N, [&](int i, int j) { return hamming(row_of(good[i]), row_of(good[j]), desc_bytes); }, &med);
                    best_median[p] = med;
                }
                best_obs[p] = good[best];
                std::memcpy(store_rows + (size_t)id * pitch, row_of(good[best]), (size_t)pitch);
            }
        }
        if (normals) {
            const float *X = pos + 3 * (size_t)id;
            float acc[3] = {0.0f, 0.0f, 0.0f}, nv[3];
            bool bad = false;
            int e_ref = -1;
            for (int e = b; e < b + n; ++e) {
                const int k = obs_kf[e];
                const float d = dist3(X, centres + 3 * (size_t)k, nv);
                if (!std::isfinite(d) || d == 0) bad = true;
                for (int q = 0; q < 3; ++q) acc[q] = acc[q] + nv[q] / d;
                if (k == ref_kf[p]) e_ref = e;
            }
            if (ref_kf[p] < 0 || e_ref < 0) {
                status[p] = RF_NO_REF;  // R1
                continue;
            }
            if (bad) {
                status[p] = RF_BAD_DISTANCE;  // R2
                continue;
            }
            const int ref = ref_kf[p];
            const float dist = dist3(X, centres + 3 * (size_t)ref, nv);
            const size_t f = (size_t)slots[ref] * cap + obs_idx[e_ref];
            const float sz = size[f], mx = dist * sz;
            for (int q = 0; q < 3; ++q) normal[3 * (size_t)id + q] = acc[q] / (float)n;
            ref_dist[id] = dist;
            ref_size[id] = sz;
            ref_sigma[id] = sqrtf(sigma2[f]);
            max_d[id] = mx;
            min_d[id] = mx / max_size[ref];
        }
    }
}

#ifdef REFRESH_HOST_MAIN
int main() {
    // three keyframes on a line, two points: one seen by all three (rows at 0, 5, 7 bits), one seen by two with the second keyframe bad
    const int cap = 2, pitch = 32, nk = 3, np = 2;
    std::vector<uint8_t> rows((size_t)nk * cap * pitch, 0);
    const int bits[3] = {0, 5, 7};
    for (int k = 0; k < nk; ++k)
        for (int i = 0; i < cap; ++i) rows[((size_t)k * cap + i) * pitch] = (uint8_t)((1 << bits[k]) - 1);
    std::vector<float> sigma2((size_t)nk * cap, 1.44f), size((size_t)nk * cap, 31.0f);
    const int32_t slots[3] = {0, 1, 2}, ids[2] = {0, 1}, ref[2] = {0, 2}, ptp[3] = {0, 3, 5}, okf[5] = {0, 1, 2, 1, 2}, oidx[5] = {0, 0, 0, 1, 1};
    const float centres[9] = {0, 0, 0, 1, 0, 0, 2, 0, 0}, max_size[3] = {100.0f, 100.0f, 100.0f};
    const uint8_t kf_bad[3] = {0, 1, 0}, flags[2] = {1, 1};
    float pos[6] = {0, 0, 10, 1, 1, 8}, normal[6] = {}, mn[2] = {}, mx[2] = {}, rs[2] = {}, rd[2] = {}, rg[2] = {};
    std::vector<uint8_t> store((size_t)2 * pitch, 0xee);
    int32_t status[2], best[2], med[2];
    refresh_host(cap, pitch, 32, 0, rows.data(), sigma2.data(), size.data(), nk, slots, centres, max_size, kf_bad, np, ids, ref, ptp, okf, oidx, 1, 1, pos,
                 normal, mn, mx, rs, rd, rg, flags, store.data(), status, best, med);
    for (int p = 0; p < np; ++p)
        std::printf("point %d status %d best_obs %d median %d ref_distance %.6f max %.4f min %.6f\n", p, status[p], best[p], med[p], rd[p], mx[p], mn[p]);
    return status[0] == RF_DONE && status[1] == RF_DONE && best[0] == 0 && best[1] == 4 ? 0 : 1;
}
#endif
