// sim3_selftest — afv::Sim3Solver (afv_adapter.hpp) as a plain C++ process, started by tests/test_gpu_sim3_adapter.py.  Every float travels
// as a hexadecimal float.
// Input (text): "cap nc n1 n2 npoints fix_scale seed nhyp minInliers maxIterations"; the camera of the current keyframe (16 floats: Rcw[9]
// tcw[3] fx fy cx cy); n1 lines "sigma2 mp1"; per candidate its camera (16 floats), n2 sigma2 values and n1 lines "mp2 idx2"; npoints lines
// "x y z bad".
// Output: per candidate the trace of LoopClosing's loop - iterate(5) until a transform or bNoMore - one line per call:
// "c mnIterations bNoMore nInliers mnBestInliers best found" and, when found, "T" with 16 floats, "R" with 9 + 3 + 1 (the getters) and "i"
// with the indices of vbInliers that are set.
#include <cstdio>
#include <cstdlib>
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

static afv::Sim3Solver::Camera camera(std::istream &in) {
    afv::Sim3Solver::Camera c;
    for (float &v : c.Rcw) v = hexf(in);
    for (float &v : c.tcw) v = hexf(in);
    c.fx = hexf(in); c.fy = hexf(in); c.cx = hexf(in); c.cy = hexf(in);
    return c;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cap = 0, nc = 0, n1 = 0, n2 = 0, npoints = 0, fix_scale = 0, nhyp = 0, min_inliers = 0, max_its = 0;
    unsigned long long seed = 0;
    in >> cap >> nc >> n1 >> n2 >> npoints >> fix_scale >> seed >> nhyp >> min_inliers >> max_its;
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    afv_table *table = nullptr;
    check(afv_table_create(ctx, nc + 1, cap, &table), "afv_table_create");
    auto fill = [&](int slot, int n, const std::vector<float> &s2) {
        const std::vector<uint8_t> rows((size_t)n * 32, 0);
        const std::vector<float> xy((size_t)n, 0.0f);
        check(afv_table_set(table, slot, rows.data(), nullptr, n), "afv_table_set");
        check(afv_table_set_geometry(table, slot, xy.data(), xy.data(), s2.data()), "afv_table_set_geometry");
    };
    const afv::Sim3Solver::Camera cam_cur = camera(in);
    std::vector<float> s2((size_t)n1);
    std::vector<int32_t> mp1((size_t)n1);
    for (int i = 0; i < n1; ++i) { s2[(size_t)i] = hexf(in); in >> mp1[(size_t)i]; }
    fill(0, n1, s2);
    std::vector<afv::Sim3Solver::Camera> cams;
    std::vector<int32_t> cands;
    std::vector<std::vector<int32_t>> mp2((size_t)nc, std::vector<int32_t>((size_t)n1)), idx2((size_t)nc, std::vector<int32_t>((size_t)n1));
    for (int c = 0; c < nc; ++c) {
        cams.push_back(camera(in));
        cands.push_back(c + 1);
        std::vector<float> t2((size_t)n2);
        for (float &v : t2) v = hexf(in);
        fill(c + 1, n2, t2);
        for (int i = 0; i < n1; ++i) in >> mp2[(size_t)c][(size_t)i] >> idx2[(size_t)c][(size_t)i];
    }
    {
        afv::DeviceMapPoints points(ctx, npoints);
        std::vector<int32_t> ids((size_t)npoints);
        std::vector<float> xyz((size_t)npoints * 3);
        std::vector<uint8_t> bad((size_t)npoints);
        for (int p = 0; p < npoints; ++p) {
            ids[(size_t)p] = p;
            for (int k = 0; k < 3; ++k) xyz[(size_t)p * 3 + k] = hexf(in);
            int b = 0;
            in >> b;
            bad[(size_t)p] = (uint8_t)b;
        }
        points.SetWorldPos(ids, xyz.data());
        points.SetFlags(ids, bad.data(), nullptr);
        std::vector<afv::Sim3Solver> solvers =
            afv::Sim3Solver::Batch(ctx, table, cap, points, 0, cam_cur, cands, cams, n1, mp1, mp2, idx2, fix_scale != 0, seed, {}, nhyp);
        for (int c = 0; c < nc; ++c) {
            afv::Sim3Solver &s = solvers[(size_t)c];
            if (!s.SetRansacParameters(0.99, min_inliers, max_its)) { std::fprintf(stderr, "SetRansacParameters refused\n"); return 1; }
            if (s.SetRansacParameters(0.99, 2, max_its) || s.SetRansacParameters(0.99, min_inliers, nhyp + 1)) return 1;
            bool no_more = false, found = false;
            while (!no_more && !found) {
                std::vector<bool> vb;
                int n_in = 0;
                float T[16];
                found = s.iterate(5, no_more, vb, n_in, T);
                std::printf("%d %d %d %d %d %d %d\n", c, s.mnIterations, no_more ? 1 : 0, n_in, s.mnBestInliers, s.best, found ? 1 : 0);
                if (found) {
                    std::printf("T");
                    for (float v : T) std::printf(" %a", v);
                    std::printf("\nR");
                    for (int k = 0; k < 9; ++k) std::printf(" %a", s.GetEstimatedRotation()[k]);
                    for (int k = 0; k < 3; ++k) std::printf(" %a", s.GetEstimatedTranslation()[k]);
                    std::printf(" %a\ni", s.GetEstimatedScale());
                    for (size_t i = 0; i < vb.size(); ++i)
                        if (vb[i]) std::printf(" %zu", i);
                    std::printf("\n");
                }
            }
        }
    }
    afv_table_destroy(table);
    afv_destroy(ctx);
    return 0;
}
