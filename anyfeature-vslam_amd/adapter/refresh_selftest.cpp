// refresh_selftest — afv::LocalBundleAdjustment followed by afv::RefreshAfterBundleAdjustment (afv_adapter.hpp) as a plain C++ process,
// started by tests/test_gpu_refresh_adapter.py.  Every float travels as a hexadecimal float, every row as 64 hexadecimal digits.
// Input (text): "cap nk npoints store_cap nobs"; per keyframe "slot fixed n bad", maxKeyPtSize, its 17 floats (Rcw[9] tcw[3] fx fy cx cy mbf)
// and n lines "x y u_right inf size sigma2 row"; npoints lines "id x y z ref_slot"; nobs lines "point_id slot idx".
// Output: per point "R status best_obs median", then per point "P" with pos[3] normal[3] min max ref_size ref_distance ref_sigma as the
// store holds them afterwards, then per point "D row".
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
    int cap = 0, nk = 0, npoints = 0, store_cap = 0, nobs = 0;
    in >> cap >> nk >> npoints >> store_cap >> nobs;
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    afv_table *table = nullptr;
    check(afv_table_create(ctx, nk + 1, cap, &table), "afv_table_create");
    std::vector<afv::BundleKeyFrame> kfs((size_t)nk);
    std::vector<float> max_size((size_t)nk);
    std::vector<uint8_t> kf_bad((size_t)nk);
    for (int k = 0; k < nk; ++k) {
        afv::BundleKeyFrame &K = kfs[(size_t)k];
        int fixed = 0, n = 0, bad = 0;
        in >> K.slot >> fixed >> n >> bad;
        K.fixed = fixed != 0;
        kf_bad[(size_t)k] = (uint8_t)bad;
        max_size[(size_t)k] = hexf(in);
        for (float &v : K.Rcw) v = hexf(in);
        for (float &v : K.tcw) v = hexf(in);
        K.fx = hexf(in); K.fy = hexf(in); K.cx = hexf(in); K.cy = hexf(in); K.mbf = hexf(in);
        std::vector<uint8_t> rows((size_t)n * 32, 0);
        std::vector<float> x((size_t)n), y((size_t)n), ur((size_t)n), inf((size_t)n), size((size_t)n), s2((size_t)n);
        for (int i = 0; i < n; ++i) {
            x[(size_t)i] = hexf(in); y[(size_t)i] = hexf(in); ur[(size_t)i] = hexf(in); inf[(size_t)i] = hexf(in);
            size[(size_t)i] = hexf(in); s2[(size_t)i] = hexf(in);
            std::string row;
            in >> row;
            for (int b = 0; b < 32; ++b) rows[(size_t)i * 32 + b] = (uint8_t)std::stoi(row.substr((size_t)2 * b, 2), nullptr, 16);
        }
        check(afv_table_set(table, K.slot, rows.data(), nullptr, n), "afv_table_set");
        check(afv_table_set_geometry(table, K.slot, x.data(), y.data(), s2.data()), "afv_table_set_geometry");
        check(afv_table_set_u_right(table, K.slot, ur.data()), "afv_table_set_u_right");
        check(afv_table_set_inf(table, K.slot, inf.data()), "afv_table_set_inf");
        check(afv_table_set_scale(table, K.slot, size.data(), nullptr, nullptr, nullptr), "afv_table_set_scale");
    }
    {
        afv::DeviceMapPoints points(ctx, store_cap);
        std::vector<int32_t> ids((size_t)npoints), ref((size_t)npoints);
        std::vector<float> xyz((size_t)npoints * 3);
        for (int p = 0; p < npoints; ++p) {
            in >> ids[(size_t)p];
            for (int k = 0; k < 3; ++k) xyz[(size_t)p * 3 + k] = hexf(in);
            in >> ref[(size_t)p];
        }
        points.SetWorldPos(ids, xyz.data());
        std::vector<afv::BundleObservation> obs((size_t)nobs);
        for (afv::BundleObservation &o : obs) in >> o.point >> o.slot >> o.idx;
        const afv::BundleAnswer A = afv::LocalBundleAdjustment(ctx, table, points, kfs, ids, obs);
        const afv::RefreshAnswer R = afv::RefreshAfterBundleAdjustment(ctx, table, points, kfs, A, max_size, kf_bad, ids, ref, obs, true);
        for (int p = 0; p < npoints; ++p) std::printf("R %d %d %d\n", R.status[(size_t)p], R.best_obs[(size_t)p], R.best_median[(size_t)p]);
        const size_t n = (size_t)npoints;
        std::vector<float> pos(n * 3), nrm(n * 3), mn(n), mx(n), rs(n), rd(n), rg(n);
        std::vector<uint8_t> rows(n * 32);
        check(afv_points_get(points.handle(), ids.data(), npoints, pos.data(), nrm.data(), mn.data(), mx.data(), rs.data(), rd.data(), rg.data(), nullptr,
                             rows.data()), "afv_points_get");
        for (size_t p = 0; p < n; ++p)
            std::printf("P %a %a %a %a %a %a %a %a %a %a %a\n", pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], nrm[3 * p], nrm[3 * p + 1], nrm[3 * p + 2], mn[p],
                        mx[p], rs[p], rd[p], rg[p]);
        for (size_t p = 0; p < n; ++p) {
            std::printf("D ");
            for (int b = 0; b < 32; ++b) std::printf("%02x", rows[p * 32 + (size_t)b]);
            std::printf("\n");
        }
    }
    afv_table_destroy(table);
    afv_destroy(ctx);
    return 0;
}
