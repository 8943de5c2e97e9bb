// kffuse_selftest — afv::FuseIntoKeyFrames and afv::FuseIntoKeyFramesSim3 (afv_adapter.hpp) as a plain C++ process, started by
// tests/test_gpu_kffuse_adapter.py.  Every float travels as a hexadecimal float, every row as 64 hexadecimal digits.
// Input (text): "cap nk store_cap npoints nq th_low"; the camera "min_x max_x min_y max_y cols rows inv_w inv_h"; per keyframe "slot n", its 17
// floats (Rcw[9] tcw[3] fx fy cx cy mbf), the 16 floats of its Scw, and n lines "x y u_right inf size point_id row"; npoints lines
// "id x y z nx ny nz min max ref_size ref_distance ref_sigma bad row"; then nq ids: ONE list for all targets.
// Output: per keyframe "F slot nFused" and nq lines "best occupant status" of Fuse no. 1, then the same under "S" for Fuse no. 2.
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

static void hexrow(std::istream &in, uint8_t *row) {
    std::string t;
    in >> t;
    for (int b = 0; b < 32; ++b) row[b] = (uint8_t)std::stoi(t.substr((size_t)2 * b, 2), nullptr, 16);
}

static void check(int rc, const char *what) {
    if (rc != AFV_OK) { std::fprintf(stderr, "%s: %s\n", what, afv_strerror(rc)); std::exit(1); }
}

static void print(const char *tag, const std::vector<afv::FuseTarget> &targets, const afv::FuseAnswer &A) {
    for (size_t k = 0; k < targets.size(); ++k) {
        std::printf("%s %d %d\n", tag, targets[k].slot, A.nFused[k]);
        for (size_t q = 0; q < A.best[k].size(); ++q) std::printf("%d %d %d\n", A.best[k][q], A.occupant[k][q], (int)A.status[k][q]);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cap = 0, nk = 0, store_cap = 0, npoints = 0, nq = 0;
    in >> cap >> nk >> store_cap >> npoints >> nq;
    const float th_low = hexf(in);
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    afv_table *table = nullptr;
    check(afv_table_create(ctx, nk + 1, cap, &table), "afv_table_create");
    afv_table_camera cam{};
    cam.struct_size = (uint32_t)sizeof(cam);
    cam.min_x = hexf(in); cam.max_x = hexf(in); cam.min_y = hexf(in); cam.max_y = hexf(in);
    in >> cam.grid_cols >> cam.grid_rows;
    cam.grid_inv_w = hexf(in); cam.grid_inv_h = hexf(in);
    check(afv_table_set_camera(table, &cam), "afv_table_set_camera");
    std::vector<int32_t> slots;
    std::vector<std::array<float, 16>> Scw((size_t)nk);
    for (int k = 0; k < nk; ++k) {
        int slot = 0, n = 0;
        in >> slot >> n;
        slots.push_back(slot);
        float pose[17];
        for (float &v : pose) v = hexf(in);
        for (float &v : Scw[(size_t)k]) v = hexf(in);
        std::vector<uint8_t> rows((size_t)n * 32, 0);
        std::vector<float> x((size_t)n), y((size_t)n), ur((size_t)n), inf((size_t)n), size((size_t)n), s2((size_t)n);
        std::vector<int32_t> plane((size_t)n);
        for (int i = 0; i < n; ++i) {
            x[(size_t)i] = hexf(in); y[(size_t)i] = hexf(in); ur[(size_t)i] = hexf(in); inf[(size_t)i] = hexf(in); size[(size_t)i] = hexf(in);
            s2[(size_t)i] = size[(size_t)i] * size[(size_t)i];
            in >> plane[(size_t)i];
            hexrow(in, rows.data() + (size_t)i * 32);
        }
        check(afv_table_set(table, slot, rows.data(), nullptr, n), "afv_table_set");
        check(afv_table_set_geometry(table, slot, x.data(), y.data(), s2.data()), "afv_table_set_geometry");
        check(afv_table_set_u_right(table, slot, ur.data()), "afv_table_set_u_right");
        check(afv_table_set_inf(table, slot, inf.data()), "afv_table_set_inf");
        check(afv_table_set_scale(table, slot, size.data(), nullptr, nullptr, nullptr), "afv_table_set_scale");
        float Ow[3];
        afv::CameraCentre(pose, pose + 9, Ow);
        check(afv_table_set_pose(table, slot, pose, pose + 9, Ow, pose[12], pose[13], pose[14], pose[15], pose[16]), "afv_table_set_pose");
        check(afv_table_set_map_points(table, slot, plane.data()), "afv_table_set_map_points");
    }
    {
        afv::DeviceMapPoints points(ctx, store_cap);
        const size_t np = (size_t)npoints;
        std::vector<int32_t> ids(np);
        std::vector<float> xyz(np * 3), nrm(np * 3), f5[5];
        for (auto &v : f5) v.resize(np);
        std::vector<uint8_t> bad(np), rows(np * 32);
        for (size_t p = 0; p < np; ++p) {
            in >> ids[p];
            for (int k = 0; k < 3; ++k) xyz[p * 3 + (size_t)k] = hexf(in);
            for (int k = 0; k < 3; ++k) nrm[p * 3 + (size_t)k] = hexf(in);
            for (auto &v : f5) v[p] = hexf(in);
            int b = 0;
            in >> b;
            bad[p] = (uint8_t)b;
            hexrow(in, rows.data() + p * 32);
        }
        points.Set(ids, xyz.data(), nrm.data(), f5[0].data(), f5[1].data(), f5[2].data(), f5[3].data(), f5[4].data());
        points.SetFlags(ids, bad.data(), nullptr);
        points.SetDescriptors(ids, rows.data());
        std::vector<int32_t> list((size_t)nq);
        for (int32_t &v : list) in >> v;
        std::vector<afv::FuseTarget> targets;
        for (int32_t s : slots) targets.push_back(afv::FuseTarget{s, &list});
        print("F", targets, afv::FuseIntoKeyFrames(ctx, table, points, targets, th_low));
        print("S", targets, afv::FuseIntoKeyFramesSim3(ctx, table, points, targets, Scw, th_low));
    }
    afv_table_destroy(table);
    afv_destroy(ctx);
    return 0;
}
