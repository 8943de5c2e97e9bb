// gba_selftest — afv::GlobalBundleAdjustment and afv::CorrectPointsSE3 (afv_adapter.hpp) as a plain C++ process, started by
// tests/test_gpu_gba_adapter.py.  Every float travels as a hexadecimal float.
// Input (text): "cap nk npoints store_cap nobs iterations robust write_points m ncorr"; per keyframe "slot fixed n", its 17 floats (Rcw[9]
// tcw[3] fx fy cx cy mbf) and n lines "x y u_right inf"; npoints lines "id x y z bad"; nobs lines "point_id slot idx"; m lines of 24
// floats (Tcw_before: R[9] t[3], Twc_after: R[9] t[3]); ncorr lines "point_id pair".
// Output: "T it0 it1 tr0 tr1 n_edges n_removed_first n_erase stopped", "D chi2[2] lambda[2]", per optimised keyframe "K slot R[9] t[3]",
// per point "X x y z", "S" with the state of every observation, "P" with the store's positions after the adjustment, "C" with the
// status of every corrected point, "Q" with the store's positions after the correction.
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

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cap = 0, nk = 0, npoints = 0, store_cap = 0, nobs = 0, iterations = 0, robust = 0, write_points = 0, m = 0, ncorr = 0;
    in >> cap >> nk >> npoints >> store_cap >> nobs >> iterations >> robust >> write_points >> m >> ncorr;
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    afv_table *table = nullptr;
    check(afv_table_create(ctx, nk + 1, cap, &table), "afv_table_create");
    std::vector<afv::BundleKeyFrame> kfs((size_t)nk);
    for (afv::BundleKeyFrame &K : kfs) {
        int fixed = 0, n = 0;
        in >> K.slot >> fixed >> n;
        K.fixed = fixed != 0;
        for (float &v : K.Rcw) v = hexf(in);
        for (float &v : K.tcw) v = hexf(in);
        K.fx = hexf(in); K.fy = hexf(in); K.cx = hexf(in); K.cy = hexf(in); K.mbf = hexf(in);
        const std::vector<uint8_t> rows((size_t)n * 32, 0);
        std::vector<float> x((size_t)n), y((size_t)n), ur((size_t)n), inf((size_t)n);
        const std::vector<float> s2((size_t)n, 1.0f);
        for (int i = 0; i < n; ++i) { x[(size_t)i] = hexf(in); y[(size_t)i] = hexf(in); ur[(size_t)i] = hexf(in); inf[(size_t)i] = hexf(in); }
        check(afv_table_set(table, K.slot, rows.data(), nullptr, n), "afv_table_set");
        check(afv_table_set_geometry(table, K.slot, x.data(), y.data(), s2.data()), "afv_table_set_geometry");
        check(afv_table_set_u_right(table, K.slot, ur.data()), "afv_table_set_u_right");
        check(afv_table_set_inf(table, K.slot, inf.data()), "afv_table_set_inf");
    }
    {
        afv::DeviceMapPoints points(ctx, store_cap);
        std::vector<int32_t> ids((size_t)npoints);
        std::vector<float> xyz((size_t)npoints * 3);
        std::vector<uint8_t> bad((size_t)npoints);
        for (int p = 0; p < npoints; ++p) {
            in >> ids[(size_t)p];
            for (int k = 0; k < 3; ++k) xyz[(size_t)p * 3 + k] = hexf(in);
            int b = 0;
            in >> b;
            bad[(size_t)p] = (uint8_t)b;
        }
        points.SetWorldPos(ids, xyz.data());
        points.SetFlags(ids, bad.data(), nullptr);
        std::vector<afv::BundleObservation> obs((size_t)nobs);
        for (afv::BundleObservation &o : obs) in >> o.point >> o.slot >> o.idx;
        std::vector<afv::SE3f> before((size_t)m), after_T((size_t)m);
        for (int q = 0; q < m; ++q) {
            for (float &v : before[(size_t)q].R) v = hexf(in);
            for (float &v : before[(size_t)q].t) v = hexf(in);
            for (float &v : after_T[(size_t)q].R) v = hexf(in);
            for (float &v : after_T[(size_t)q].t) v = hexf(in);
        }
        std::vector<int32_t> cids((size_t)ncorr), pair((size_t)ncorr);
        for (int i = 0; i < ncorr; ++i) in >> cids[(size_t)i] >> pair[(size_t)i];
        const afv::BundleAnswer A = afv::GlobalBundleAdjustment(ctx, table, points, kfs, ids, obs, iterations, nullptr, robust != 0, write_points != 0);
        const afv_lba_result &r = A.trace;
        std::printf("T %d %d %d %d %d %d %d %d\n", r.iterations[0], r.iterations[1], r.trials[0], r.trials[1], r.n_edges, r.n_removed_first, r.n_erase,
                    r.stopped);
        std::printf("D %a %a %a %a\n", r.chi2[0], r.chi2[1], r.lambda[0], r.lambda[1]);
        for (const auto &kp : A.poses) {
            std::printf("K %d", kp.first);
            for (double v : kp.second.R) std::printf(" %a", v);
            for (double v : kp.second.t) std::printf(" %a", v);
            std::printf("\n");
        }
        for (int p = 0; p < npoints; ++p) std::printf("X %a %a %a\n", A.xyz[(size_t)p * 3], A.xyz[(size_t)p * 3 + 1], A.xyz[(size_t)p * 3 + 2]);
        std::printf("S");
        for (uint8_t s : A.edge_state) std::printf(" %d", (int)s);
        std::printf("\n");
        std::vector<float> got((size_t)npoints * 3);
        auto dump = [&](const char *tag) {
            check(afv_points_get(points.handle(), ids.data(), npoints, got.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                  "afv_points_get");
            for (int p = 0; p < npoints; ++p) std::printf("%s %a %a %a\n", tag, got[(size_t)p * 3], got[(size_t)p * 3 + 1], got[(size_t)p * 3 + 2]);
        };
        dump("P");
        const std::vector<uint8_t> st = afv::CorrectPointsSE3(ctx, points, cids, pair, before, after_T);
        std::printf("C");
        for (uint8_t s : st) std::printf(" %d", (int)s);
        std::printf("\n");
        dump("Q");
    }
    afv_table_destroy(table);
    afv_destroy(ctx);
    return 0;
}
