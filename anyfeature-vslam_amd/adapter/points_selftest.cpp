// points_selftest — afv::DeviceMapPoints and the point searches of afv::DeviceFrame (afv_adapter.hpp) as a plain C++ process, started by
// tests/test_gpu_points_adapter.py.  Every float travels as a hexadecimal float.
// Input (text): "capacity n"; n lines "id x y z nx ny nz minD maxD refSize refDist refSigma bad observed b0 .. b31"; a line with Rcw[9] tcw[3]
// Ow[3] fx fy cx cy mbf; "width height nf"; nf lines "x y size angle b0 .. b31" (the frame's features); "nl"; nl lines "size angle" (the
// last frame); "nq" and nq ids; "radiusTh viewingCosLimit th nnratio".
// Output: "local n: assign..", "inview: ..", "last n: assign..", "reloc n: assign..", "fuse n: best..".
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

static void line(const char *tag, int n, const std::vector<int32_t> &v) {
    std::printf("%s %d:", tag, n);
    for (int32_t x : v) std::printf(" %d", x);
    std::printf("\n");
}

static void fill_frame(afv_frame *f, const std::vector<afv_keypoint> &kps, const std::vector<uint8_t> &desc, const std::vector<float> &size) {
    const int rc = afv_frame_set_features(f, kps.data(), desc.data(), (int)kps.size(), size.data(), nullptr);
    if (rc != AFV_OK) { std::fprintf(stderr, "afv_frame_set_features: %s\n", afv_strerror(rc)); std::exit(1); }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cap = 0, n = 0;
    in >> cap >> n;
    std::vector<int32_t> ids((size_t)n);
    std::vector<float> pos((size_t)n * 3), nrm((size_t)n * 3), f5[5];
    for (auto &v : f5) v.resize((size_t)n);
    std::vector<uint8_t> bad((size_t)n), obs((size_t)n), rows((size_t)n * 32);
    for (int i = 0; i < n; ++i) {
        in >> ids[(size_t)i];
        for (int k = 0; k < 3; ++k) pos[(size_t)i * 3 + k] = hexf(in);
        for (int k = 0; k < 3; ++k) nrm[(size_t)i * 3 + k] = hexf(in);
        for (auto &v : f5) v[(size_t)i] = hexf(in);
        int b = 0, o = 0;
        in >> b >> o;
        bad[(size_t)i] = (uint8_t)b;
        obs[(size_t)i] = (uint8_t)o;
        for (int k = 0; k < 32; ++k) { int v; in >> v; rows[(size_t)i * 32 + k] = (uint8_t)v; }
    }
    float pose[20];
    for (float &v : pose) v = hexf(in);
    float width = hexf(in), height = hexf(in);
    int nf = 0;
    in >> nf;
    std::vector<afv_keypoint> kps((size_t)nf);
    std::vector<float> size((size_t)nf);
    std::vector<uint8_t> desc((size_t)nf * 32);
    for (int i = 0; i < nf; ++i) {
        kps[(size_t)i] = afv_keypoint{};
        kps[(size_t)i].x = hexf(in); kps[(size_t)i].y = hexf(in);
        size[(size_t)i] = hexf(in);
        kps[(size_t)i].angle = hexf(in);
        for (int k = 0; k < 32; ++k) { int v; in >> v; desc[(size_t)i * 32 + k] = (uint8_t)v; }
    }
    int nl = 0;
    in >> nl;
    std::vector<afv_keypoint> lkps((size_t)nl);
    std::vector<float> lsize((size_t)nl), langle((size_t)nl);
    for (int i = 0; i < nl; ++i) {
        lkps[(size_t)i] = afv_keypoint{};
        lsize[(size_t)i] = hexf(in);
        langle[(size_t)i] = lkps[(size_t)i].angle = hexf(in);
    }
    int nq = 0;
    in >> nq;
    std::vector<int32_t> q((size_t)nq);
    for (int32_t &v : q) in >> v;
    const float radiusTh = hexf(in), cosLimit = hexf(in), th = hexf(in), nnratio = hexf(in);
    if (!in || nq > nl) return 2;

    afv_orb_params p;
    afv_default_orb_params(&p);
    afv_ctx *ctx = nullptr;
    const int rc = afv_create(0, &p, &ctx);
    if (rc != AFV_OK) { std::fprintf(stderr, "afv_create: %s\n", afv_strerror(rc)); return 1; }
    {
        afv::DeviceMapPoints points(ctx, cap);
        points.SetWorldPos(ids, pos.data());
        points.UpdateNormalAndDepth(ids, nrm.data(), f5[0].data(), f5[1].data(), f5[2].data(), f5[3].data(), f5[4].data());
        points.SetFlags(ids, bad.data(), obs.data());
        points.SetDescriptors(ids, rows.data());
        afv::DeviceFrame cur(ctx, 0.0f, 0.0f, width, height), last(ctx, 0.0f, 0.0f, width, height);
        fill_frame(cur.handle(), kps, desc, size);
        fill_frame(last.handle(), lkps, std::vector<uint8_t>((size_t)nl * 32, 0), lsize);
        cur.SetPose(pose, pose + 9, pose + 12, pose[15], pose[16], pose[17], pose[18], pose[19]);
        std::vector<int32_t> out;
        std::vector<uint8_t> in_view;
        int m = cur.SearchLocalPoints(points, q, radiusTh, cosLimit, th, nnratio, out, in_view);
        line("local", m, out);
        std::printf("inview:");
        for (uint8_t v : in_view) std::printf(" %d", (int)v);
        std::printf("\n");
        m = cur.SearchByProjectionLast(points, last, q, radiusTh, th, nnratio, true, out);
        line("last", m, out);
        m = cur.SearchByProjectionReloc(points, q, langle.data(), radiusTh, th, nnratio, true, out);
        line("reloc", m, out);
        m = cur.FusePoints(points, q, radiusTh, th, false, out);
        line("fuse", m, out);
    }
    afv_destroy(ctx);
    return 0;
}
