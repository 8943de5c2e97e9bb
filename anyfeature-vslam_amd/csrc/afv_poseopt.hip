// afv_poseopt.hip — host side of Optimizer::PoseOptimization on a resident frame (include/afv_hip.h, "pose optimisation"; kernel:
// k_poseopt.hip).  A call stages pts[N] and the initial pose of every job, runs one launch and fetches the results.
#include "afv_runtime.h"

extern "C" int afv_frame_pose_optimize(afv_frame *f, afv_points *points, const afv_pose_job *jobs, int njobs, afv_pose_result *results) {
    if (!f || !points || !jobs || !results) return AFV_EINVAL;
    if (njobs < 1 || njobs > AFV_POSE_MAX_JOBS) return AFV_EINVAL;
    if (!afv_frame_is_live(f) || !afv_points_is_live(points) || points->c != f->c) return AFV_EINVAL;
    if (!f->has_features || !f->has_grid || f->n < 1 || f->n > AFV_POSE_MAX_FEATURES || !f->has_pose) return AFV_EINVAL;
    std::vector<afv_pose_job> J;
    if (!afv_load_jobs(jobs, njobs, sizeof(afv_pose_job), J)) return AFV_EINVAL;
    // the result records are strided by their own struct_size, as the job records are
    const uint32_t rs = results[0].struct_size;
    if (rs != sizeof(afv_pose_result)) return AFV_EINVAL;  // (the one layout there is: a later one is told apart by its size here)
    auto result_at = [&](int j) { return reinterpret_cast<afv_pose_result *>(reinterpret_cast<uint8_t *>(results) + (size_t)j * rs); };
    const int n = f->n;
    for (int j = 0; j < njobs; ++j) {
        if (result_at(j)->struct_size != rs) return AFV_EINVAL;
        if (!J[j].pts || (J[j].Rcw == nullptr) != (J[j].tcw == nullptr)) return AFV_EINVAL;
        for (int i = 0; i < n; ++i)
            if (J[j].pts[i] >= points->cap) return AFV_EINVAL;
    }
    afv_ctx *c = f->c;
    return guarded(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        Blob b(c);
        const size_t N = (size_t)n;
        const size_t o_pts = b.reserve_scratch((size_t)njobs * N * 4), o_pose = b.reserve_scratch((size_t)njobs * 48);
        for (int j = 0; j < njobs; ++j) {
            std::memcpy(b.h.data() + o_pts + (size_t)j * N * 4, J[j].pts, N * 4);
            float *pose = reinterpret_cast<float *>(b.h.data() + o_pose + (size_t)j * 48);
            std::memcpy(pose, J[j].Rcw ? J[j].Rcw : f->Rcw, 36);
            std::memcpy(pose + 9, J[j].tcw ? J[j].tcw : f->tcw, 12);
        }
        const size_t in_bytes = b.h.size();
        const size_t o_out = b.reserve_scratch((size_t)njobs * sizeof(DevPoseOut)), o_flag = b.reserve_scratch((size_t)njobs * N);
        const int rc = ensure_match_buffer(c, b.h.size());
        if (rc) return rc;
        uint8_t *B = c->d_match;
        HIPCHK(c, b.upload(in_bytes));
        DevPoseArgs A{};
        for (int k = 0; k < 3; ++k) A.pos[k] = points->P.pos[k];
        A.flags = points->P.flags;
        A.cap = points->cap;
        A.x = f->d_x; A.y = f->d_y; A.ur = f->d_ur; A.inf = f->d_inf;
        A.n = n;
        A.fx = f->fx; A.fy = f->fy; A.cx = f->cx; A.cy = f->cy; A.bf = f->mbf;
        A.pts = reinterpret_cast<const int *>(B + o_pts);
        A.poses = reinterpret_cast<const float *>(B + o_pose);
        A.out = reinterpret_cast<DevPoseOut *>(B + o_out);
        A.outlier = B + o_flag;
        afv_launch_pose_optimize(&A, njobs, c->stream);
        HIPCHK(c, hipGetLastError());
        std::vector<DevPoseOut> outs((size_t)njobs);
        HIPCHK(c, b.fetch(outs.data(), o_out, (size_t)njobs * sizeof(DevPoseOut), c->stream));
        for (int j = 0; j < njobs; ++j)
            if (result_at(j)->outlier) HIPCHK(c, b.fetch(result_at(j)->outlier, o_flag + (size_t)j * N, N, c->stream));
        HIPCHK(c, b.wait());
        for (int j = 0; j < njobs; ++j) {
            afv_pose_result *r = result_at(j);
            const DevPoseOut &o = outs[(size_t)j];
            std::memcpy(r->Rcw, o.R, sizeof(r->Rcw));
            std::memcpy(r->tcw, o.t, sizeof(r->tcw));
            r->n_good = o.n_good; r->n_edges = o.n_edges; r->rounds = o.rounds;
            for (int k = 0; k < 4; ++k) {
                r->iterations[k] = o.iterations[k]; r->trials[k] = o.trials[k];
                r->chi2[k] = o.chi2[k]; r->lambda[k] = o.lambda[k];
            }
        }
        return AFV_OK;
    });
}
