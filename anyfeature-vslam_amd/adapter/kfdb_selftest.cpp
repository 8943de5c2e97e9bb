// kfdb_selftest — afv::KeyFrameDatabase (afv_adapter.hpp) as a plain C++ process, started by tests/test_gpu_table_bow.py.
// Input (text): K; then K + 1 BowVectors (the keyframes of slots 0 .. K-1 and the relocalisation frame), each as a line with its
// length and a line of "word value" pairs (values as hexadecimal floats); then K lines "n slot..." (GetBestCovisibilityKeyFrames of every
// slot); then "loop_slot n connected...".  Slots 0 .. K-2 join the database.
// Output: "reloc: slots", "scores: the frame's score against every slot", "minscore: value", "loop: slots".
//
// Second input form, an operation script (tests/test_gpu_kfdb_scenes.py): the first token is the word "script", then K and the table's
// capacity; K lines "n word value ..." (the BowVector of slot s; n = -1 leaves the slot empty); K lines "n slot..." (the covisibles, ids
// outside the table allowed); then one operation per line:
//   add s | erase s | reloc n word value ... | loop s minScore n connected... | minscore s n connected...
// minScore is a hexadecimal float or the word "last" (the result of the last minscore line).  Nothing joins the database by itself.
// Output: one line per query, "reloc: slots", "loop: slots" or "minscore: value".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "afv_adapter.hpp"

static bool read_bow(std::istream &in, afv::BowVector &b, int &n) {
    n = 0;
    in >> n;
    for (int i = 0; i < n; ++i) {
        unsigned w;
        std::string hex;
        in >> w >> hex;
        b[w] = std::strtod(hex.c_str(), nullptr);
    }
    return (bool)in;
}

static void print_slots(const char *what, const std::vector<int> &slots) {
    std::printf("%s:", what);
    for (int s : slots) std::printf(" %d", s);
    std::printf("\n");
}

static int run_script(std::istream &in) {
    int K = 0, cap = 0;
    in >> K >> cap;
    if (!in || K < 1 || cap < 1) return 2;
    std::vector<afv::BowVector> bows((size_t)K);
    std::vector<int> present((size_t)K, 0);
    for (int s = 0; s < K; ++s) {
        int n = 0;
        if (!read_bow(in, bows[(size_t)s], n) || n > cap) return 2;
        present[(size_t)s] = n >= 0;
    }
    std::vector<std::vector<int>> covis((size_t)K);
    for (auto &c : covis) {
        int n = 0;
        in >> n;
        if (!in || n < 0) return 2;
        c.resize((size_t)n);
        for (int &v : c) in >> v;
    }
    if (!in) return 2;
    afv_orb_params p;
    afv_default_orb_params(&p);
    afv_ctx *ctx = nullptr;
    int rc = afv_create(0, &p, &ctx);
    if (rc != AFV_OK) { std::fprintf(stderr, "afv_create: %s\n", afv_strerror(rc)); return 1; }
    afv_table *t = nullptr;
    rc = afv_table_create(ctx, K, cap, &t);
    if (rc != AFV_OK) { std::fprintf(stderr, "afv_table_create: %s\n", afv_strerror(rc)); return 1; }
    const std::vector<uint8_t> one(32, 0x5a);  // a slot scores only when it holds features
    for (int s = 0; s < K; ++s) {
        if (!present[(size_t)s]) continue;
        std::vector<int32_t> w;
        std::vector<double> v;
        for (const auto &kv : bows[(size_t)s]) w.push_back((int32_t)kv.first), v.push_back(kv.second);
        rc = afv_table_set(t, s, one.data(), nullptr, 1);
        if (rc == AFV_OK) rc = afv_table_set_bowvec(t, s, w.data(), v.data(), (int)w.size());
        if (rc != AFV_OK) { std::fprintf(stderr, "filling slot %d: %s (%s)\n", s, afv_strerror(rc), afv_last_error(ctx)); return 1; }
    }
    int status = 0;
    {
        afv::KeyFrameDatabase db(ctx, t, K);
        const afv::KeyFrameDatabase::Covisibles best = [&](int s) { return s >= 0 && s < K ? covis[(size_t)s] : std::vector<int>(); };
        float last = 1.0f;
        std::string op;
        while (in >> op) {
            int s = 0, n = 0;
            if (op == "add" || op == "erase") {
                in >> s;
                if (op == "add") db.add(s);
                else db.erase(s);
            } else if (op == "reloc") {
                afv::BowVector q;
                if (!read_bow(in, q, n)) { status = 2; break; }
                print_slots("reloc", db.DetectRelocalizationCandidates(q, best));
            } else if (op == "loop" || op == "minscore") {
                std::string ms;
                in >> s;
                if (op == "loop") in >> ms;
                in >> n;
                if (!in || n < 0) { status = 2; break; }
                std::vector<int> connected((size_t)n);
                for (int &v : connected) in >> v;
                if (op == "minscore") {
                    last = db.min_score_to_connected(s, connected);
                    std::printf("minscore: %a\n", (double)last);
                } else {
                    const float min_score = ms == "last" ? last : (float)std::strtod(ms.c_str(), nullptr);
                    print_slots("loop", db.DetectLoopCandidates(s, min_score, connected, best));
                }
            } else {
                status = 2;
                break;
            }
            if (!in) { status = 2; break; }
        }
    }
    afv_table_destroy(t);
    afv_destroy(ctx);
    return status;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    {
        std::string head;
        const std::streampos at = in.tellg();
        in >> head;
        if (head == "script") return run_script(in);
        in.clear();
        in.seekg(at);
    }
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
