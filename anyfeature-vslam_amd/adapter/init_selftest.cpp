// init_selftest — afv::Initializer (afv_adapter.hpp) as a plain C++ process, started by tests/test_gpu_init_adapter.py.  Every float travels
// as a hexadecimal float.
// Input (text): "n1 n2 iterations seed", then "fx fy cx cy sigma", n1 lines "x y match" (frame 1), n2 lines "x y" (frame 2).
// Output: "ok route reason n best_h best_f n_motion best_motion", "R" with 9 floats, "t" with 3, per motion hypothesis "m nGood cos",
// then per feature of frame 1 "p triangulated x y z".
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

static void fill(afv::DeviceFrame &f, const std::vector<float> &x, const std::vector<float> &y) {
    const size_t n = x.size();
    std::vector<afv_keypoint> kps(n);
    for (size_t i = 0; i < n; ++i) {
        kps[i] = afv_keypoint{};
        kps[i].x = x[i]; kps[i].y = y[i]; kps[i].size = 31.0f;
    }
    const std::vector<uint8_t> desc(n * 32, 0);
    const std::vector<float> size(n, 1.0f);
    check(afv_frame_set_features(f.handle(), kps.data(), desc.data(), (int)n, size.data(), nullptr), "afv_frame_set_features");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int n1 = 0, n2 = 0, iterations = 0;
    unsigned long long seed = 0;
    in >> n1 >> n2 >> iterations >> seed;
    const float fx = hexf(in), fy = hexf(in), cx = hexf(in), cy = hexf(in), sigma = hexf(in);
    std::vector<float> x1((size_t)n1), y1((size_t)n1), x2((size_t)n2), y2((size_t)n2);
    std::vector<int> matches((size_t)n1);
    for (int i = 0; i < n1; ++i) { x1[(size_t)i] = hexf(in); y1[(size_t)i] = hexf(in); in >> matches[(size_t)i]; }
    for (int i = 0; i < n2; ++i) { x2[(size_t)i] = hexf(in); y2[(size_t)i] = hexf(in); }
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    {
        afv::DeviceFrame F1(ctx, -4000.0f, -4000.0f, 4000.0f, 4000.0f), F2(ctx, -4000.0f, -4000.0f, 4000.0f, 4000.0f);
        fill(F1, x1, y1);
        fill(F2, x2, y2);
        afv::Initializer ini(F1, fx, fy, cx, cy, sigma, iterations, seed);
        float R21[9], t21[3];
        std::vector<std::array<float, 3>> vP3D;
        std::vector<bool> vbTriangulated;
        const bool ok = ini.Initialize(F2, matches, R21, t21, vP3D, vbTriangulated);
        const afv_init_trace &T = ini.trace;
        std::printf("%d %d %d %d %d %d %d %d\n", ok ? 1 : 0, ini.route, T.reason, T.n, T.best_h, T.best_f, T.n_motion, T.best_motion);
        std::printf("R");
        for (float v : R21) std::printf(" %a", (double)v);
        std::printf("\nt");
        for (float v : t21) std::printf(" %a", (double)v);
        std::printf("\n");
        for (int i = 0; i < T.n_motion; ++i) std::printf("m %d %a\n", T.n_good[i], (double)T.cos_parallax[i]);
        for (int i = 0; i < n1; ++i)
            std::printf("p %d %a %a %a\n", vbTriangulated[(size_t)i] ? 1 : 0, (double)vP3D[(size_t)i][0], (double)vP3D[(size_t)i][1], (double)vP3D[(size_t)i][2]);
    }
    afv_destroy(ctx);
    return 0;
}
