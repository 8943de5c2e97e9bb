// stereo_host_walk.cpp — the host walk a stereo integrator ran before afv_frame_stereo_match: Frame::ComputeStereoMatches
// (src/Frame.cc:465-645) on one core over host arrays, with the semantics of tests/_stereo_ref.py (deviations A, B, C of
// include/afv_hip.h).  tools/time_stereo.py compiles it (g++ -O2 -ffp-contract=off -shared), times it next to the device path and compares
// the two outputs bit for bit.  32-byte binary descriptors only.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

struct KeyPoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

static int hamming32(const uint8_t *a, const uint8_t *b) {
    int d = 0;
    for (int i = 0; i < 32; i += 8) d += __builtin_popcountll(*reinterpret_cast<const uint64_t *>(a + i) ^ *reinterpret_cast<const uint64_t *>(b + i));
    return d;
}

extern "C" int stereo_host_walk(const KeyPoint *kl, const float *size_l, const uint8_t *desc_l, int n, const KeyPoint *kr, const float *size_r,
                                const uint8_t *desc_r, int nr, const uint8_t *const *pyr_l, const uint8_t *const *pyr_r, const int *lw, const int *lh,
                                int nlevels, float mbf, float fx, float th_high, float th_low, float *u_right, float *depth) {
    const float th_orb = (th_high + th_low) / 2.0f;
    const int n_rows = lh[0];
    std::vector<std::vector<int>> rows((size_t)n_rows);
    for (int iR = 0; iR < nr; ++iR) {
        const float r = 2.0f * size_r[iR];
        const int maxr = (int)std::ceil(kr[iR].y + r), minr = (int)std::floor(kr[iR].y - r);
        for (int yi = std::max(minr, 0); yi <= std::min(maxr, n_rows - 1); ++yi) rows[(size_t)yi].push_back(iR);
    }
    const float mb = mbf / fx, min_d = 0, max_d = mbf / mb;
    std::vector<std::pair<int, int>> dist_idx;
    for (int iL = 0; iL < n; ++iL) {
        u_right[iL] = -1.0f;
        depth[iL] = -1.0f;
        const int level = kl[iL].octave;
        const float vL = kl[iL].y, uL = kl[iL].x;
        const int row = (int)vL;
        if (row < 0 || row >= n_rows) continue;
        const std::vector<int> &cand = rows[(size_t)row];
        if (cand.empty()) continue;
        const float min_u = uL - max_d, max_u = uL - min_d;
        if (max_u < 0) continue;
        float best = th_high;
        int best_r = 0;
        for (int iR : cand) {
            if (kr[iR].octave < level - 1 || kr[iR].octave > level + 1) continue;
            const float uR = kr[iR].x;
            if (uR >= min_u && uR <= max_u) {
                const float d = (float)hamming32(desc_l + (size_t)iL * 32, desc_r + (size_t)iR * 32);
                if (d < best) {
                    best = d;
                    best_r = iR;
                }
            }
        }
        if (!(best < th_orb)) continue;
        const float s = 1.0f / size_l[iL];
        const int su = (int)std::round(uL * s), sv = (int)std::round(vL * s), su0 = (int)std::round(kr[best_r].x * s);
        if (level < 0 || level >= nlevels) continue;
        const int w = lw[level], h = lh[level];
        if (su0 < 0 || su0 + 11 >= w) continue;
        if (sv - 5 < 0 || sv + 5 >= h || su - 5 < 0 || su + 5 >= w || su0 - 10 < 0) continue;
        const uint8_t *imL = pyr_l[level], *imR = pyr_r[level];
        const int lc = imL[(size_t)sv * w + su];
        int sads[11], best_sad = 0x7fffffff, best_inc = 0;
        for (int inc = -5; inc <= 5; ++inc) {
            const int rc = imR[(size_t)sv * w + su0 + inc];
            int acc = 0;
            for (int dy = -5; dy <= 5; ++dy) {
                const uint8_t *pl = imL + (size_t)(sv + dy) * w + su - 5, *pr = imR + (size_t)(sv + dy) * w + su0 + inc - 5;
                for (int dx = 0; dx < 11; ++dx) acc += std::abs(((int)pl[dx] - lc) - ((int)pr[dx] - rc));
            }
            sads[inc + 5] = acc;
            if (acc < best_sad) {
                best_sad = acc;
                best_inc = inc;
            }
        }
        if (best_inc == -5 || best_inc == 5) continue;
        const float d1 = (float)sads[best_inc + 4], d2 = (float)sads[best_inc + 5], d3 = (float)sads[best_inc + 6];
        const float delta = (d1 - d3) / (2.0f * (d1 + d3 - 2.0f * d2));
        if (delta < -1 || delta > 1) continue;
        float best_u = size_l[iL] * ((float)su0 + (float)best_inc + delta);
        float disparity = uL - best_u;
        if (disparity >= min_d && disparity < max_d) {
            if (disparity <= 0) {
                disparity = 0.01f;
                best_u = (float)((double)uL - 0.01);
            }
            depth[iL] = mbf / disparity;
            u_right[iL] = best_u;
            dist_idx.push_back(std::make_pair(best_sad, iL));
        }
    }
    if (dist_idx.empty()) return 0;
    std::sort(dist_idx.begin(), dist_idx.end());
    const float median = (float)dist_idx[dist_idx.size() / 2].first;
    const float th_dist = 1.5f * 1.4f * median;
    int kept = (int)dist_idx.size();
    for (int i = (int)dist_idx.size() - 1; i >= 0; --i) {
        if ((float)dist_idx[(size_t)i].first < th_dist) break;
        u_right[dist_idx[(size_t)i].second] = -1;
        depth[dist_idx[(size_t)i].second] = -1;
        --kept;
    }
    return kept;
}
