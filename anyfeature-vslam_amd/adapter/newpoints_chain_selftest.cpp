// newpoints_chain_selftest — afv::NewMapPoints::CreateNewMapPointsChain (afv_adapter.hpp: the neighbour loop in ONE
// afv_table_create_new_points call) as a plain C++ process, started by tests/test_gpu_newpts_chain_adapter.py.  Every float travels as a
// hexadecimal float.
// Input (text), the format of newpoints_selftest extended by the starting masks: "cap nkf n first_id capacity th_low"; per keyframe n lines
// "x y sigma2 size b0 .. b31"; per neighbour (nkf - 1 of them) a line with the floats of afv_tri_points_job after struct_size and a line
// "F12[9] ex ey"; then per keyframe (the current one first) a line of n bytes 0 / 1: its mask "already has a map point".
// Output: one line "id slot1 idx1 slot2 idx2" per created point in creation order, then per point "p id" and its seven fields (pos[3]
// normal[3] minD maxD refSize refDist refSigma) as hexadecimal floats and its flags, then per keyframe "m slot" and the n bytes of its
// mask after the call.
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "afv_adapter.hpp"

static float hexf(std::istream &in) {
    std::string t;
    in >> t;
    return std::strtof(t.c_str(), nullptr);
}

static void check(int rc, const char *what) {
    if (rc != AFV_OK) { std::fprintf(stderr, "%s: %s\n", what, afv_strerror(rc)); std::exit(1); }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cap = 0, nkf = 0, n = 0, first_id = 0, capacity = 0;
    in >> cap >> nkf >> n >> first_id >> capacity;
    const float th_low = hexf(in);
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    afv_table *table = nullptr;
    check(afv_table_create(ctx, nkf, cap, &table), "afv_table_create");
    std::vector<int32_t> idx((size_t)n);
    for (int i = 0; i < n; ++i) idx[(size_t)i] = i;
    const int32_t node_id[1] = {0}, seg_ptr[2] = {0, n};
    for (int k = 0; k < nkf; ++k) {
        std::vector<float> x((size_t)n), y((size_t)n), s2((size_t)n), size((size_t)n);
        std::vector<uint8_t> rows((size_t)n * 32);
        for (int i = 0; i < n; ++i) {
            x[(size_t)i] = hexf(in); y[(size_t)i] = hexf(in); s2[(size_t)i] = hexf(in); size[(size_t)i] = hexf(in);
            for (int b = 0; b < 32; ++b) { int v; in >> v; rows[(size_t)i * 32 + b] = (uint8_t)v; }
        }
        check(afv_table_set(table, k, rows.data(), nullptr, n), "afv_table_set");
        check(afv_table_set_featvec(table, k, node_id, seg_ptr, idx.data(), 1), "afv_table_set_featvec");
        check(afv_table_set_geometry(table, k, x.data(), y.data(), s2.data()), "afv_table_set_geometry");
        check(afv_table_set_scale(table, k, size.data(), nullptr, nullptr, nullptr), "afv_table_set_scale");
    }
    std::vector<afv_tri_points_job> jobs((size_t)nkf - 1);
    std::vector<afv_table_tri_job> tri((size_t)nkf - 1);
    std::vector<int32_t> neighbours;
    for (int k = 0; k + 1 < nkf; ++k) {
        afv_tri_points_job &j = jobs[(size_t)k];
        j = afv_tri_points_job{};
        float f[47];  // the floats of the record follow each other from Rcw1 on
        static_assert(sizeof(afv_tri_points_job) == offsetof(afv_tri_points_job, Rcw1) + sizeof(f), "afv_tri_points_job");
        for (float &v : f) v = hexf(in);
        std::memcpy(reinterpret_cast<char *>(&j) + offsetof(afv_tri_points_job, Rcw1), f, sizeof(f));
        afv_table_tri_job &t = tri[(size_t)k];
        t = afv_table_tri_job{};
        for (float &v : t.F12) v = hexf(in);
        t.ex = hexf(in); t.ey = hexf(in);
        t.th_low = th_low;
        neighbours.push_back(k + 1);
    }
    {
        afv::DeviceMapPoints points(ctx, capacity);
        afv::NewMapPoints lm(ctx, table, cap);
        std::vector<std::vector<uint8_t>> has_mp((size_t)nkf, std::vector<uint8_t>((size_t)cap, 0));
        for (int k = 0; k < nkf; ++k)
            for (int i = 0; i < n; ++i) { int v; in >> v; has_mp[(size_t)k][(size_t)i] = (uint8_t)v; }
        const std::vector<afv::NewMapPoints::Created> made = lm.CreateNewMapPointsChain(points, 0, neighbours, jobs, tri, has_mp, first_id);
        for (const auto &c : made) std::printf("%d %d %d %d %d\n", c.id, c.slot1, c.idx1, c.slot2, c.idx2);
        for (const auto &c : made) {
            float pos[3], nrm[3], f5[5];
            uint8_t flags = 0;
            check(afv_points_get(points.handle(), &c.id, 1, pos, nrm, &f5[0], &f5[1], &f5[2], &f5[3], &f5[4], &flags, nullptr), "afv_points_get");
            std::printf("p %d", c.id);
            for (float v : pos) std::printf(" %a", v);
            for (float v : nrm) std::printf(" %a", v);
            for (float v : f5) std::printf(" %a", v);
            std::printf(" %d\n", (int)flags);
        }
        for (int k = 0; k < nkf; ++k) {
            std::printf("m %d", k);
            for (int i = 0; i < n; ++i) std::printf(" %d", (int)has_mp[(size_t)k][(size_t)i]);
            std::printf("\n");
        }
    }
    afv_table_destroy(table);
    afv_destroy(ctx);
    return 0;
}
