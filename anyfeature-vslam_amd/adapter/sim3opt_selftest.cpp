// sim3opt_selftest — afv::OptimizeSim3 / afv::OptimizeSim3Batch (afv_adapter.hpp) as a plain C++ process, started by
// tests/test_gpu_sim3opt_adapter.py.  Every float travels as a hexadecimal float.
// Input (text): "cap nc n1 n2 npoints fix_scale th2"; the camera of the current keyframe (16 floats: Rcw[9] tcw[3] fx fy cx cy); n1 lines
// "x y inf mp1"; per candidate its camera (16 floats), its start (13 floats: R12 t12 s12), n2 lines "x y inf" and n1 lines "mp2 idx2";
// npoints lines "x y z bad".
// Output: per candidate of the batch "c nIn n_corr n_bad more early it0 it1 tr0 tr1", "S" with R12[9] t12[3] s12 chi2[2] lambda[2] and "m"
// with vpMatches1 after the call; then the same three lines for candidate 0 through the one-candidate call, with c = -1.
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

static void report(int c, const afv::OptimizeSim3Answer &a, const std::vector<int32_t> &matches) {
    const afv_sim3opt_result &r = a.trace;
    std::printf("%d %d %d %d %d %d %d %d %d %d\nS", c, a.nInliers, r.n_corr, r.n_bad, r.more_iterations, r.early, r.iterations[0], r.iterations[1],
                r.trials[0], r.trials[1]);
    for (double v : a.g2oS12.R) std::printf(" %a", v);
    for (double v : a.g2oS12.t) std::printf(" %a", v);
    std::printf(" %a %a %a %a %a\nm", a.g2oS12.s, r.chi2[0], r.chi2[1], r.lambda[0], r.lambda[1]);
    for (int32_t m : matches) std::printf(" %d", m);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cap = 0, nc = 0, n1 = 0, n2 = 0, npoints = 0, fix_scale = 0;
    in >> cap >> nc >> n1 >> n2 >> npoints >> fix_scale;
    const float th2 = hexf(in);
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    afv_table *table = nullptr;
    check(afv_table_create(ctx, nc + 1, cap, &table), "afv_table_create");
    auto fill = [&](int slot, int n) {
        const std::vector<uint8_t> rows((size_t)n * 32, 0);
        std::vector<float> x((size_t)n), y((size_t)n), inf((size_t)n);
        const std::vector<float> s2((size_t)n, 1.0f);
        for (int i = 0; i < n; ++i) { x[(size_t)i] = hexf(in); y[(size_t)i] = hexf(in); inf[(size_t)i] = hexf(in); }
        check(afv_table_set(table, slot, rows.data(), nullptr, n), "afv_table_set");
        check(afv_table_set_geometry(table, slot, x.data(), y.data(), s2.data()), "afv_table_set_geometry");
        check(afv_table_set_inf(table, slot, inf.data()), "afv_table_set_inf");
    };
    const afv::Sim3Solver::Camera cam_cur = camera(in);
    std::vector<int32_t> mp1((size_t)n1);
    {   // keyframe 1: "x y inf mp1" per line
        const std::vector<uint8_t> rows((size_t)n1 * 32, 0);
        std::vector<float> x((size_t)n1), y((size_t)n1), inf((size_t)n1);
        const std::vector<float> s2((size_t)n1, 1.0f);
        for (int i = 0; i < n1; ++i) { x[(size_t)i] = hexf(in); y[(size_t)i] = hexf(in); inf[(size_t)i] = hexf(in); in >> mp1[(size_t)i]; }
        check(afv_table_set(table, 0, rows.data(), nullptr, n1), "afv_table_set");
        check(afv_table_set_geometry(table, 0, x.data(), y.data(), s2.data()), "afv_table_set_geometry");
        check(afv_table_set_inf(table, 0, inf.data()), "afv_table_set_inf");
    }
    std::vector<afv::Sim3Solver::Camera> cams;
    std::vector<int32_t> cands;
    std::vector<afv::Sim3d> starts;
    std::vector<std::vector<int32_t>> mp2((size_t)nc, std::vector<int32_t>((size_t)n1)), idx2((size_t)nc, std::vector<int32_t>((size_t)n1));
    for (int c = 0; c < nc; ++c) {
        cams.push_back(camera(in));
        cands.push_back(c + 1);
        afv::Sim3d s;
        for (double &v : s.R) v = (double)hexf(in);
        for (double &v : s.t) v = (double)hexf(in);
        s.s = (double)hexf(in);
        starts.push_back(s);
        fill(c + 1, n2);
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
        std::vector<std::vector<int32_t>> matches = mp2;
        const std::vector<afv::OptimizeSim3Answer> all =
            afv::OptimizeSim3Batch(ctx, table, cap, points, 0, cam_cur, cands, cams, n1, mp1, matches, idx2, starts, th2, fix_scale != 0);
        for (int c = 0; c < nc; ++c) report(c, all[(size_t)c], matches[(size_t)c]);
        std::vector<int32_t> alone = mp2[0];
        afv::Sim3d S = starts[0];
        const int n_in = afv::OptimizeSim3(ctx, table, cap, points, 0, cam_cur, cands[0], cams[0], n1, mp1, alone, idx2[0], S, th2, fix_scale != 0);
        afv::OptimizeSim3Answer a = all[0];
        a.nInliers = n_in;
        a.g2oS12 = S;
        report(-1, a, alone);
    }
    afv_table_destroy(table);
    afv_destroy(ctx);
    return 0;
}
