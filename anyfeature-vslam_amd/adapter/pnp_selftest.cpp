// pnp_selftest — afv::PnPsolver (afv_adapter.hpp) as a plain C++ process, started by tests/test_gpu_pnp_adapter.py.  Every float travels as
// a hexadecimal float.
// Input (text): "nf nc npoints seed nhyp minInliers maxIterations"; "epsilon th2 width height"; the frame's pose and intrinsics (19 floats:
// Rcw[9] tcw[3] Ow[3] fx fy cx cy); nf lines "x y octave"; per candidate nf point ids; npoints lines "x y z flags" (bit 0 set, bit 1 bad).
// Output: per candidate the trace of Relocalization's loop - iterate(5) until a pose or bNoMore - one line per call:
// "c mnIterations bNoMore nInliers mnBestInliers best found" and, when found, "T" with 16 floats and "i" with the indices of vbInliers
// that are set.
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
    int nf = 0, nc = 0, npoints = 0, nhyp = 0, min_inliers = 0, max_its = 0;
    unsigned long long seed = 0;
    in >> nf >> nc >> npoints >> seed >> nhyp >> min_inliers >> max_its;
    const float epsilon = hexf(in), th2 = hexf(in), width = hexf(in), height = hexf(in);
    float pose[19];
    for (float &v : pose) v = hexf(in);
    std::vector<afv_keypoint> kps((size_t)nf);
    for (int i = 0; i < nf; ++i) {
        kps[(size_t)i] = afv_keypoint{};
        kps[(size_t)i].x = hexf(in); kps[(size_t)i].y = hexf(in);
        in >> kps[(size_t)i].octave;
    }
    std::vector<std::vector<int32_t>> pts((size_t)nc, std::vector<int32_t>((size_t)nf));
    for (auto &row : pts)
        for (int32_t &v : row) in >> v;
    std::vector<int32_t> set_ids, bad_ids;
    std::vector<float> xyz;
    for (int p = 0; p < npoints; ++p) {
        float q[3];
        for (float &v : q) v = hexf(in);
        int flags = 0;
        in >> flags;
        if (flags & 1) { set_ids.push_back(p); xyz.insert(xyz.end(), q, q + 3); }
        if (flags & 2) bad_ids.push_back(p);
    }
    if (!in) return 2;
    afv_orb_params prm;
    afv_default_orb_params(&prm);
    afv_ctx *ctx = nullptr;
    check(afv_create(0, &prm, &ctx), "afv_create");
    {
        afv::DeviceMapPoints points(ctx, npoints);
        points.SetWorldPos(set_ids, xyz.data());
        const std::vector<uint8_t> ones(bad_ids.size(), 1);
        if (!bad_ids.empty()) points.SetFlags(bad_ids, ones.data(), nullptr);
        afv::DeviceFrame cur(ctx, 0.0f, 0.0f, width, height);
        const std::vector<uint8_t> desc((size_t)nf * 32, 0);
        check(afv_frame_set_features(cur.handle(), kps.data(), desc.data(), nf, nullptr, nullptr), "afv_frame_set_features");
        cur.SetPose(pose, pose + 9, pose + 12, pose[15], pose[16], pose[17], pose[18], 0.0f);
        std::vector<afv::PnPsolver> solvers = afv::PnPsolver::Batch(ctx, cur, nf, points, pts, seed, nhyp, min_inliers, epsilon, th2);
        for (int c = 0; c < nc; ++c) {
            afv::PnPsolver &s = solvers[(size_t)c];
            if (!s.SetRansacParameters(0.99, min_inliers, max_its, 4, epsilon, th2)) { std::fprintf(stderr, "SetRansacParameters refused\n"); return 1; }
            if (s.SetRansacParameters(0.99, min_inliers + 1, max_its, 4, epsilon, th2) || s.SetRansacParameters(0.99, min_inliers, nhyp + 1, 4, epsilon, th2) ||
                s.SetRansacParameters(0.99, min_inliers, max_its, 5, epsilon, th2))
                return 1;
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
                    std::printf("\ni");
                    for (size_t i = 0; i < vb.size(); ++i)
                        if (vb[i]) std::printf(" %zu", i);
                    std::printf("\n");
                }
            }
        }
    }
    afv_destroy(ctx);
    return 0;
}
