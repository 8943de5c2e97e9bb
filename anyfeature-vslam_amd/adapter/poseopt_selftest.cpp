// poseopt_selftest — DeviceFrame::PoseOptimization of afv_adapter.hpp as a plain C++ process, started by tests/test_gpu_poseopt.py.  Every
// float travels as a hexadecimal float.
// Input (text): "capacity n"; n lines "id x y z"; a line with Rcw[9] tcw[3] Ow[3] fx fy cx cy mbf; "width height nf"; nf lines
// "x y uRight octave pointId" (the frame's features and F.pts).
// Output: "ngood: n", "pose: Rcw[9] tcw[3]", "outlier: ..", "stored: Rcw[9] tcw[3] Ow[3]" (what the frame holds after the call).
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

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int cap = 0, n = 0;
    in >> cap >> n;
    std::vector<int32_t> ids((size_t)n);
    std::vector<float> pos((size_t)n * 3);
    for (int i = 0; i < n; ++i) {
        in >> ids[(size_t)i];
        for (int k = 0; k < 3; ++k) pos[(size_t)i * 3 + k] = hexf(in);
    }
    float pose[20];
    for (float &v : pose) v = hexf(in);
    const float width = hexf(in), height = hexf(in);
    int nf = 0;
    in >> nf;
    std::vector<afv_keypoint> kps((size_t)nf);
    std::vector<float> ur((size_t)nf);
    std::vector<int32_t> pts((size_t)nf);
    for (int i = 0; i < nf; ++i) {
        kps[(size_t)i] = afv_keypoint{};
        kps[(size_t)i].x = hexf(in); kps[(size_t)i].y = hexf(in);
        ur[(size_t)i] = hexf(in);
        in >> kps[(size_t)i].octave >> pts[(size_t)i];
    }
    if (!in) return 2;

    afv_orb_params p;
    afv_default_orb_params(&p);
    afv_ctx *ctx = nullptr;
    int rc = afv_create(0, &p, &ctx);
    if (rc != AFV_OK) { std::fprintf(stderr, "afv_create: %s\n", afv_strerror(rc)); return 1; }
    {
        afv::DeviceMapPoints points(ctx, cap);
        points.SetWorldPos(ids, pos.data());
        afv::DeviceFrame cur(ctx, 0.0f, 0.0f, width, height);
        const std::vector<uint8_t> desc((size_t)nf * 32, 0);
        rc = afv_frame_set_features(cur.handle(), kps.data(), desc.data(), nf, nullptr, ur.data());
        if (rc != AFV_OK) { std::fprintf(stderr, "afv_frame_set_features: %s\n", afv_strerror(rc)); return 1; }
        cur.SetPose(pose, pose + 9, pose + 12, pose[15], pose[16], pose[17], pose[18], pose[19]);
        std::vector<uint8_t> outlier;
        afv_pose_job job{};
        job.struct_size = sizeof(job);
        job.pts = pts.data();
        afv_pose_result r{};
        r.struct_size = sizeof(r);
        rc = afv_frame_pose_optimize(cur.handle(), points.handle(), &job, 1, &r);  // the record itself, for the pose floats
        if (rc != AFV_OK) { std::fprintf(stderr, "afv_frame_pose_optimize: %s\n", afv_strerror(rc)); return 1; }
        const int ngood = cur.PoseOptimization(points, pts, outlier);
        if (ngood != r.n_good) { std::fprintf(stderr, "the two calls differ: %d %d\n", ngood, r.n_good); return 1; }
        std::printf("ngood: %d\npose:", ngood);
        for (int k = 0; k < 9; ++k) std::printf(" %a", (double)r.Rcw[k]);
        for (int k = 0; k < 3; ++k) std::printf(" %a", (double)r.tcw[k]);
        std::printf("\noutlier:");
        for (uint8_t v : outlier) std::printf(" %d", (int)v);
        std::printf("\nstored:");
        for (int k = 0; k < 9; ++k) std::printf(" %a", (double)cur.Rcw()[k]);
        for (int k = 0; k < 3; ++k) std::printf(" %a", (double)cur.tcw()[k]);
        for (int k = 0; k < 3; ++k) std::printf(" %a", (double)cur.Ow()[k]);
        std::printf("\n");
    }
    afv_destroy(ctx);
    return 0;
}
