// kfdb_selftest — afv::KeyFrameDatabase (afv_adapter.hpp) as a plain C++ process, started by tests/test_gpu_table_bow.py.
// Input (text): K; then K + 1 BowVectors (the keyframes of slots 0 .. K-1 and the relocalisation frame), each as a line with its
// length and a line of "word value" pairs (values as hexadecimal floats); then K lines "n slot..." (GetBestCovisibilityKeyFrames of every
// slot); then "loop_slot n connected...".  Slots 0 .. K-2 join the database.
// Output: "reloc: slots", "scores: the frame's score against every slot", "minscore: value", "loop: slots".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "afv_adapter.hpp"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int K = 0;
    in >> K;
    if (K < 2) return 2;
    std::vector<afv::BowVector> bows((size_t)K + 1);
    size_t cap = 1;
    for (auto &b : bows) {
        int n = 0;
        in >> n;
        for (int i = 0; i < n; ++i) {
            unsigned w;
            std::string hex;
            in >> w >> hex;
            b[w] = std::strtod(hex.c_str(), nullptr);
        }
        cap = std::max(cap, b.size());
    }
    std::vector<std::vector<int>> covis((size_t)K);
    for (auto &c : covis) {
        int n = 0;
        in >> n;
        c.resize((size_t)n);
        for (int &v : c) in >> v;
    }
    int loop_slot = 0, nconn = 0;
    in >> loop_slot >> nconn;
    std::vector<int> connected((size_t)nconn);
    for (int &v : connected) in >> v;
    if (!in) return 2;

    afv_orb_params p;
    afv_default_orb_params(&p);
    afv_ctx *ctx = nullptr;
    int rc = afv_create(0, &p, &ctx);
    if (rc != AFV_OK) { std::fprintf(stderr, "afv_create: %s\n", afv_strerror(rc)); return 1; }
    afv_table *t = nullptr;
    rc = afv_table_create(ctx, K, (int)cap, &t);
    if (rc != AFV_OK) { std::fprintf(stderr, "afv_table_create: %s\n", afv_strerror(rc)); return 1; }
    const std::vector<uint8_t> one(32, 0x5a);  // a slot scores only when it holds features
    for (int s = 0; s < K; ++s) {
        std::vector<int32_t> w;
        std::vector<double> v;
        for (const auto &kv : bows[(size_t)s]) w.push_back((int32_t)kv.first), v.push_back(kv.second);
        rc = afv_table_set(t, s, one.data(), nullptr, 1);
        if (rc == AFV_OK) rc = afv_table_set_bowvec(t, s, w.data(), v.data(), (int)w.size());
        if (rc != AFV_OK) { std::fprintf(stderr, "filling slot %d: %s (%s)\n", s, afv_strerror(rc), afv_last_error(ctx)); return 1; }
    }
    afv::KeyFrameDatabase db(ctx, t, K);
    for (int s = 0; s + 1 < K; ++s) db.add(s);
    const afv::KeyFrameDatabase::Covisibles best = [&](int s) { return covis[(size_t)s]; };
    std::printf("reloc:");
    for (int s : db.DetectRelocalizationCandidates(bows[(size_t)K], best)) std::printf(" %d", s);
    std::printf("\nscores:");
    {   // the frame against EVERY slot (the database leaves the last one out)
        std::vector<int32_t> w, common((size_t)K);
        std::vector<double> v, score((size_t)K);
        for (const auto &kv : bows[(size_t)K]) w.push_back((int32_t)kv.first), v.push_back(kv.second);
        afv_bow_query q{};
        q.struct_size = sizeof(q);
        q.kind = AFV_BOW_QUERY_HOST;
        q.n = (int32_t)w.size();
        q.word = w.data();
        q.value = v.data();
        rc = afv_table_score_bow(t, &q, 1, nullptr, common.data(), score.data(), nullptr);
        if (rc != AFV_OK) { std::fprintf(stderr, "afv_table_score_bow: %s\n", afv_strerror(rc)); return 1; }
        for (double sc : score) std::printf(" %a", sc);
    }
    const float ms = db.min_score_to_connected(loop_slot, connected);
    std::printf("\nminscore: %a\nloop:", (double)ms);
    for (int s : db.DetectLoopCandidates(loop_slot, ms, connected, best)) std::printf(" %d", s);
    std::printf("\n");
    afv_table_destroy(t);
    afv_destroy(ctx);
    return 0;
}
