// bow_host_walk — the host path an integrator had before afv_table_score_bow: DBoW2's L1Scoring::score over std::map BowVectors
// (adapter/afv_adapter.hpp's BowVector), one core.  Compiled and started by tools/time_table_bow.py.
// usage: bow_host_walk <bows.bin> <nq> <scores.out>   (bows.bin: int32 K, then per keyframe int32 n, int32 word[n], double value[n])
// Scores queries 0 .. nq-1 against all K keyframes, prints the seconds that took, writes the scores [nq][K] as doubles.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

using BowVector = std::map<unsigned, double>;

static double score(const BowVector &v1, const BowVector &v2) {
    auto a = v1.begin(), b = v2.begin();
    double s = 0;
    bool any = false;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) {
            s += std::fabs(a->second - b->second) - std::fabs(a->second) - std::fabs(b->second);
            any = true;
            ++a;
            ++b;
        } else if (a->first < b->first) {
            a = v1.lower_bound(b->first);
        } else {
            b = v2.lower_bound(a->first);
        }
    }
    return any ? -s / 2.0 : 0.0;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t K = 0;
    if (std::fread(&K, 4, 1, f) != 1) return 2;
    std::vector<BowVector> bows((size_t)K);
    for (auto &b : bows) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1) return 2;
        std::vector<int32_t> w((size_t)n);
        std::vector<double> v((size_t)n);
        if (n && (std::fread(w.data(), 4, (size_t)n, f) != (size_t)n || std::fread(v.data(), 8, (size_t)n, f) != (size_t)n)) return 2;
        for (int i = 0; i < n; ++i) b[(unsigned)w[(size_t)i]] = v[(size_t)i];
    }
    std::fclose(f);
    const int nq = std::atoi(argv[2]);
    std::vector<double> out((size_t)nq * K);
    const auto t0 = std::chrono::steady_clock::now();
    for (int q = 0; q < nq; ++q)
        for (int k = 0; k < K; ++k) out[(size_t)q * K + k] = score(bows[(size_t)q], bows[(size_t)k]);
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%.6f\n", dt);
    FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    std::fwrite(out.data(), 8, out.size(), o);
    std::fclose(o);
    return 0;
}
