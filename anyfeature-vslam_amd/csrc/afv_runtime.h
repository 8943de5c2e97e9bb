// afv_runtime.h — host-side internals shared by the translation units behind the C-ABI (afv_api.hip, afv_extract.hip, afv_comm.hip,
// afv_match_jobs.hip, afv_project.hip, afv_frame.hip, afv_points.hip, afv_stereo.hip): the context, the pinned staging arena (Blob), the
// kernel launcher prototypes and the job descriptions of the matcher pipelines.  Not part of the public interface.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "afv_device.h"
#include "afv_host.h"  // AFV_LOCAL, HIPCHK, guarded, cv_round, align_up, the level quotas, the pinned-memory probes
#include "afv_jobs.h"

// ---- kernel launchers (k_*.hip) ----
extern "C" void afv_launch_resize(const uint8_t *src, int sw, int sh, int spitch, size_t sframe, uint8_t *dst, int dw, int dh,
                                  int dpitch, size_t dframe, const short2 *xt, const short2 *yt, int frame_base, int nframes, int *zero_counts,
                                  int n_zero, int *zero_one, hipStream_t stream);
extern "C" int afv_resize_window_ok(int sw, int sh, int dw, int dh);
extern "C" void afv_launch_pyramid_fused(const FrameSrc *src0, uint8_t *pyr, const PyrFuseArgs *args, size_t lds_bytes, int frame_base, int nframes,
                                         hipStream_t stream);
extern "C" int afv_pyramid_fused_prepare(size_t lds_bytes);
extern "C" void afv_launch_fast_nms(const Geo *geo, int total_tiles, const FrameSrc *src0, const uint8_t *pyr, uint32_t *cand_packed,
                                    int *cand_count, int frame_base, int nframes, hipStream_t stream);
extern "C" size_t afv_harris_queue_per_frame(const Geo *g);
extern "C" void afv_launch_retain_harris(const Geo *geo_dev, int nlevels, const FrameSrc *src0, const uint8_t *pyr,
                                         const uint32_t *cand_packed, const int *cand_count, uint32_t *l1, int *l1_count,
                                         float *l1_resp, uint2 *queue, int *queue_n, int frame_base, int nframes, int small, hipStream_t stream);
extern "C" size_t afv_select_lds_bytes(int M);
extern "C" void afv_launch_select(const Geo *geo_dev, int nlevels, const uint32_t *cand_packed, const float *cand_resp,
                                  const int *cand_count, uint32_t *kept_xy, float *kept_resp, uint16_t *kept_node, SelPoint *sel,
                                  int *sel_count, int M, int frame_base, int nframes, int wide, hipStream_t stream);
extern "C" int afv_describe_blocks_per_frame(const Geo *g);
// second destination of the describe kernel's outputs (afv_frame_extract: the frame's device arrays next to the pinned host copy); all null = none
struct DescribeMirror {
    afv_keypoint *kps;
    uint8_t *desc;
    int *n;
};
extern "C" void afv_launch_describe(const Geo *geo_dev, int blocks_per_frame, const FrameSrc *src0, const uint8_t *pyr,
                                    const SelPoint *sel, const int *sel_count, afv_keypoint *kps, uint8_t *desc,
                                    int cap_per_frame, int *n_out, int *status, int frame_base, int nframes, const DescribeMirror *mirror,
                                    hipStream_t stream);
extern "C" void afv_launch_describe_given(const Geo *geo_dev, const FrameSrc *src0, const uint8_t *pyr, const afv_keypoint *given, int n, uint8_t *desc,
                                          int frame, hipStream_t stream);
extern "C" void afv_launch_blur_level(const uint8_t *img, int w, int h, int pitch, uint8_t *out, hipStream_t stream);

extern "C" void afv_launch_match_bow(const DevMatchJob *jobs, int njobs, hipStream_t stream);
extern "C" void afv_launch_match_bow_seg(const DevMatchJob *jobs, int njobs, const void *tasks, int ntasks, int *hist, uint8_t *bins,
                                         const int *bin_off, int any_ori, hipStream_t stream);
extern "C" int afv_match_topk_slices(int cap, int engine, int want);
extern "C" void afv_launch_match_topk(const uint8_t *desc, const int *nset, int cap, const int *pa, const int *pb, int npairs,
                                      void *topk_scratch, int pair_base, int engine, int nslices, void *slice_scratch, int *tickets,
                                      int words, hipStream_t stream);
extern "C" void afv_launch_match_resolve(const uint8_t *desc, const float *ang, int ang_stride, const int *nset, int cap, const int *pa,
                                         const int *pb, int npairs, float th, float ratio, int check_ori, int *match, int *nmatches,
                                         const void *topk_scratch, int pair_base, int engine, int words, hipStream_t stream);
extern "C" void afv_launch_match_tri(const DevTriJob *jobs, int njobs, int max_n1, hipStream_t stream);
extern "C" void afv_launch_match_l2(const float *d1, int n1, const float *d2, int n2, int dim, const uint8_t *v1,
                                    const uint8_t *v2, float th, float ratio, int *out, int *nmatches, hipStream_t stream);

extern "C" void afv_launch_distinctive_f32(const float *desc, int dim, const int *set_ptr, int nsets, int *best_idx, float *best_median, hipStream_t stream);
extern "C" void afv_launch_distinctive(const uint32_t *desc, const int *set_ptr, int nsets, int words, int desc_bytes, int *best_idx, int *best_median,
                                       hipStream_t stream);
extern "C" void afv_launch_match_projection(const DevProjJob *jobs, int njobs, int max_nq, size_t wg_lds, const DevProjJob *one, int *ticket,
                                            hipStream_t stream);
extern "C" int afv_project_prepare(void);
extern "C" int afv_match_prepare(void);
extern "C" int afv_select_prepare(int M);
extern "C" int afv_debug_pass_cap;
extern "C" size_t afv_project_wg_lds(int kind_init, int n, int nq, int float_rows);
extern "C" size_t afv_frame_grid_lds(int cols, int rows, int cap);
extern "C" int afv_frame_prepare(void);
extern "C" size_t afv_featvec_build_lds(int cap, int width);
extern "C" void afv_launch_frame_grid(const DevGridJob *jobs, int njobs, size_t lds_bytes, hipStream_t stream);
extern "C" void afv_launch_frame_grid1(const DevGridJob *job, size_t lds_bytes, hipStream_t stream);
extern "C" void afv_launch_frame_gather(const uint8_t *table, const int *nset, int nsets, int cap, const int *slot, const int *idx, int nq,
                                        void *out, int *bad, int words, hipStream_t stream);
extern "C" void afv_launch_featvec_build(const int *leaf, const int *nid, const int *dense, int n, int cap, int width, const uint8_t *stopped,
                                         int *seg_idx, int *n_kept, int *h_leaf, int *h_nid, int *h_dense, hipStream_t stream);
extern "C" void afv_launch_table_promote(const void *args, int n, int cap, int words, hipStream_t stream);
extern "C" void afv_launch_match_fuse(const DevProjJob *jobs, int njobs, int max_nq, const DevProjJob *one, hipStream_t stream);
extern "C" size_t afv_match_l2_scratch_bytes(int n1, int n2, int *ntiles_out, int *cols_per_tile_out);
extern "C" int afv_launch_match_l2_tiled(const float *d1, int n1, const float *d2, int n2, int dim, const uint8_t *v1, const uint8_t *v2,
                                         float th, float ratio, int *out, int *nmatches, void *scratch, int ntiles, int cols_per_tile,
                                         hipStream_t stream);
extern "C" int afv_launch_match_l2_pairs(const float *desc, const int *nset, int cap, int dim, const int *pa, const int *pb, int npairs,
                                         int pair_base, float th, float ratio, const float *ang, int *out, int *nmatches, void *scratch,
                                         hipStream_t stream);
extern "C" void afv_launch_match_init(const DevProjJob *jobs, int njobs, int max_nq, size_t wg_lds, const DevProjJob *one, int *ticket,
                                      hipStream_t stream);

// ---- k_stereo.hip: Frame::ComputeStereoMatches / ComputeStereoFromRGBD ----
struct DevStereoJob {
    const afv_keypoint *kps_l, *kps_r;   // mvKeys / mvKeysRight (distorted)
    const float *size_l, *size_r;        // keyPtsSize
    const uint32_t *desc_l, *desc_r;     // rows of `words` dwords (binary, zero padded) or `fdim` floats
    int n_l, n_r, words, fdim;
    float th_high, th_orb, mbf, max_d;
    int n_rows, nlevels;
    int lw[AFV_MAX_LEVELS], lh[AFV_MAX_LEVELS];
    const uint8_t *pyr_l[AFV_MAX_LEVELS], *pyr_r[AFV_MAX_LEVELS];  // level l: lw[l] x lh[l] bytes, tightly packed
    float *u_right, *depth;              // [n_l] outputs
    int *sad, *best_r, *n_stereo;
};
extern "C" void afv_launch_stereo_match(const DevStereoJob *job, hipStream_t stream);
extern "C" void afv_launch_stereo_median(float *u_right, float *depth, const int *sad, int n, int *n_stereo, hipStream_t stream);
extern "C" void afv_launch_stereo_rgbd(const afv_keypoint *kps, const float *x_un, int n, const float *img, int w, int h, float mbf, float *u_right,
                                       float *depth, hipStream_t stream);

// ---- k_points.hip: the resident map-point store and the projections in front of the projection searches ----
#define AFV_PTF_SET 1u       // flag bits of a point
#define AFV_PTF_BAD 2u
#define AFV_PTF_OBSERVED 4u
struct DevPointPlanes {      // the store (SoA over `cap` ids)
    float *pos[3], *normal[3], *min_d, *max_d, *ref_size, *ref_dist, *ref_sigma;
    uint8_t *flags;
    uint8_t *desc;           // [cap] rows of 4 * words bytes
    int cap, words;
};
struct DevPointsJob {        // k_points_project: a kernel argument
    DevPointPlanes P;
    const int *ids;
    int nq, flavour;
    float R[9], t[3], Ow[3], fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;
    float rs_th;             // radius_scale * radius_th, one float product made on the host
    float cos_limit, tol;
    const float *last_size;  // LASTFRAME: keyPtsSize of the last frame, indexed by q
    float *qu, *qv, *qr, *qmin, *qmax, *q_ur, *q_er;
    uint8_t *qvalid, *qocc;
    uint4 *qd;               // [nq] gathered rows; null: no gather
    int *count, *ticket;     // the context's accumulator of queries in view and its ticket, both zero at rest
    int *count_out;          // where the last workgroup leaves the sum
    float *o_size, *o_sigma, *o_cos;  // afv_frame_project_points only (may be null)
};
struct DevPointsMove {       // k_points_move: n ids between packed arrays (host order) and the planes; null = field not moved
    DevPointPlanes P;
    const int *ids;
    int n, gather;           // gather 0: packed -> planes (a setter); 1: planes -> packed (afv_points_get)
    float *pos, *normal, *min_d, *max_d, *ref_size, *ref_dist, *ref_sigma;
    uint8_t *bad, *observed, *flags;
    int mark_set;
};
extern "C" void afv_launch_points_project(const DevPointsJob *job, hipStream_t stream);
// afv_table_fuse_points (host side: afv_kffuse.hip): one record per target keyframe.  The camera fields carry the names k_points_project
// reads from its job: one text evaluates the geometry for both
struct DevKfFuseJob {
    float R[9], t[3], Ow[3], fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;
    float rs_th, cos_limit, tol;
    const int *ids;          // [nq]
    int nq, n;               // queries; features of the slot
    const int *plane;        // [n] the slot's mvpMapPoints
    float *qu, *qv, *qr, *qmin, *qmax, *q_ur;
    uint8_t *qvalid;         // 1: the query goes into the search
    uint8_t *status;         // [nq] 0 / 1 / 2, AFV_KF_PENDING for a query the search decides
    uint4 *qd;               // [nq] rows of the id list; null: another job of the call gathers them
    const int *best;         // [nq] what k_match_fuse leaves
    int *occupant;           // [nq]
};
#define AFV_KF_PENDING 255
extern "C" void afv_launch_kffuse_project(const DevPointPlanes *P, const DevKfFuseJob *jobs, int njobs, int max_nq, hipStream_t stream);
extern "C" void afv_launch_kffuse_finish(const DevPointPlanes *P, const DevKfFuseJob *jobs, int njobs, int max_nq, hipStream_t stream);
extern "C" void afv_launch_points_move(const DevPointsMove *job, hipStream_t stream);
// descriptor rows of n ids: from packed rows of the store's pitch (table == null), from rows (slot, idx) of a keyframe table, or (gather)
// out of the store into packed rows
extern "C" void afv_launch_points_rows(const DevPointPlanes *P, const int *ids, int n, uint8_t *packed, const uint8_t *table, int table_cap,
                                       const int *slot, const int *idx, int gather, hipStream_t stream);

// ---- k_triangulate.hip: the match loop of LocalMapping::CreateNewMapPoints over table slots (host side: afv_triangulate.hip) ----
#define AFV_TRI_T 256        // lanes per workgroup: one per feature of keyframe a
struct DevTriPair {          // one (a, b) pair: the caller's record and where the planes of the two slots start
    float R1[9], t1[3], O1[3], R2[9], t2[3], O2[3];
    float fx1, fy1, cx1, cy1, invfx1, invfy1, fx2, fy2, cx2, cy2, invfx2, invfy2;
    float mb1, mb2, mbf1, ratio_factor, max_size1;
    int n1, n2;
    const float *x1, *y1, *sigma2_1, *ur1, *size1, *depth1, *xd1, *yd1;
    const float *x2, *y2, *sigma2_2, *ur2, *size2, *depth2, *xd2, *yd2;
    const uint8_t *rows1;    // the descriptor rows of slot a
};
struct DevTriArgs {          // a kernel argument of both launches
    const DevTriPair *pairs;
    const int *match12;      // [npairs][cap]
    int npairs, cap, nblk;   // nblk = workgroups per pair
    uint8_t *status, *route; // [npairs][cap]
    float *x3d;              // [npairs][cap][3]
    int *blk_count;          // [npairs][nblk] accepted matches per workgroup (launch 1 writes, launch 2 reads)
    int *new_id, *n_new;     // [npairs][cap], [npairs]
    int *total;              // one int: accepted matches of the call
    DevPointPlanes P;        // the store (has_points)
    int has_points, first_id;
};
extern "C" void afv_launch_tri_points(const DevTriArgs *args, hipStream_t stream);
extern "C" void afv_launch_tri_store(const DevTriArgs *args, hipStream_t stream);

// ---- k_newpoints.hip: the neighbour loop of CreateNewMapPoints as a chain of launches (host side: afv_newpoints.hip) ----
struct DevNewPtsArgs {       // a kernel argument of both launches of every neighbour; the neighbour index is the second argument
    const DevTriJob *search; // [nn] the search of neighbour k: valid1 = mask_cur, valid2 = row k of mask_nb
    const DevTriPair *pairs; // [nn] a = the current keyframe, b = neighbour k
    int nn, cap, nblk;       // nblk = workgroups per launch
    uint8_t *mask_cur;       // [cap] "already has a map point" of the current keyframe: the store launch of neighbour k writes, the judge
                             // launch of neighbour k + 1 reads
    uint8_t *mask_nb;        // [nn][cap] the neighbours' masks
    int *match12;            // [nn][cap]
    uint8_t *status, *route; // [nn][cap]
    float *x3d;              // [nn][cap][3]
    int *new_id, *n_new;     // [nn][cap], [nn]
    int *blk_count;          // [nn][nblk] accepted matches per workgroup (the judge launch writes, the store launch reads)
    int *next_id;            // [nn + 1] the id base of neighbour k: launch k reads cell k, one thread of it writes cell k + 1
    int *stop;               // [nn + 1] the capacity rule: set from the first neighbour on whose points do not fit the store
    DevPointPlanes P;        // the store (has_points)
    int has_points;
};
extern "C" void afv_launch_newpts_judge(const DevNewPtsArgs *args, int k, hipStream_t stream);
extern "C" void afv_launch_newpts_store(const DevNewPtsArgs *args, int k, hipStream_t stream);

// ---- k_sim3.hip: Sim3Solver's constructor and all its RANSAC hypotheses (host side: afv_sim3.hip) ----
#define AFV_SIM3_T 256       // lanes per workgroup of both launches
struct DevSim3Cand {         // one candidate: the caller's record and where the sigma2 planes of the two slots start
    float R1[9], t1[3], R2[9], t2[3];
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    unsigned long long seed;
    int fix_scale, n1;
    const float *sigma2_1, *sigma2_2;
};
struct DevSim3Args {         // a kernel argument of both launches
    const DevSim3Cand *cands;
    const int *mp1, *mp2, *idx1, *idx2;  // [nc][cap]; idx1 null: i1
    int nc, cap, nhyp, mask_words;
    const float *pos[3];     // the store: XYZ planes and flags over `pcap` ids
    const uint8_t *flags;
    int pcap;
    int *n, *index1;         // [nc], [nc][cap]
    float *x1, *x2;          // [nc][cap][3] mvX3Dc1 / mvX3Dc2
    float *im1, *im2;        // [nc][cap][2] mvP1im1 / mvP2im2
    float *max_err;          // [nc][cap][2]
    int *count;              // [nc][nhyp]
    uint8_t *degenerate;     // [nc][nhyp]
    float *sim3;             // [nc][nhyp][13]
    uint32_t *inliers;       // [nc][nhyp][mask_words]
};
extern "C" void afv_launch_sim3_gather(const DevSim3Args *args, hipStream_t stream);
extern "C" void afv_launch_sim3_hypotheses(const DevSim3Args *args, hipStream_t stream);

// ---- k_sim3opt.hip: Optimizer::OptimizeSim3 for every candidate of a loop check (host side: afv_sim3opt.hip) ----
#define AFV_SIM3OPT_T 256    // lanes per workgroup of the gather; the solve runs one wavefront per job
struct DevSim3OptJob {       // one job: the caller's record and where the planes of the two slots start
    float R1[9], t1[3], R2[9], t2[3];
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    float R12[9], t12[3], s12, th2;
    int fix_scale, n1;
    const float *x1, *y1, *inf1, *x2, *y2, *inf2;
};
struct DevSim3OptEdge {      // one correspondence as the gather leaves it
    float p1[3], p2[3];      // P3D1c, P3D2c
    float obs1[2], obs2[2];
    float inf1, inf2;
};
struct DevSim3OptArgs {      // a kernel argument of both launches
    const DevSim3OptJob *jobs;
    const int *mp1, *mp2, *idx2;  // [nc][cap]
    int nc, cap;
    const float *pos[3];     // the store: XYZ planes and flags over `pcap` ids
    const uint8_t *flags;
    int pcap;
    int *n, *index1;         // [nc], [nc][cap]: the edges' features in ascending order
    DevSim3OptEdge *edges;   // [nc][cap]
    uint8_t *active;         // [nc][cap] by edge: 1 while the edge is in the graph
    afv_sim3opt_result *results;  // [nc]
    uint8_t *state;          // [nc][cap] by feature
};
extern "C" void afv_launch_sim3opt_gather(const DevSim3OptArgs *args, hipStream_t stream);
extern "C" void afv_launch_sim3opt_solve(const DevSim3OptArgs *args, hipStream_t stream);

// ---- k_lba.hip: LocalBundleAdjustment / BundleAdjustment (host side: afv_lba.hip; the arithmetic: afv_lba_math.h) ----
struct LbView;
struct LbCam;
struct DevLbaGather {        // k_lba_gather: what the call reads from the table and the store, and where it goes in the view
    const float *geo, *inf;  // the table's planes: geo [4][nsets][cap], inf [nsets][cap]
    size_t plane;            // nsets * cap
    int cap;
    const int *slots, *obs_idx, *point_ids;  // [nk], [ne], [np]
    const float *cams;       // [nk][17]: Rcw, tcw, fx, fy, cx, cy, bf
    const float *pos[3];     // the store
    const uint8_t *flags;
    double *obs;             // [5][ne]
    uint8_t *stereo, *p_on;
    LbCam *cam;
};
struct DevLbaFinish {        // k_lba_finish
    double *kf_out, *xyz_out;
    float *pos[3];
    const int *point_ids;
    int write_points;
};
extern "C" void afv_launch_lba_gather(const LbView *V, const DevLbaGather *G, hipStream_t stream);
extern "C" void afv_launch_lba_round(const LbView *V, int max_it, int robust, hipStream_t stream);
extern "C" void afv_launch_lba_iteration(const LbView *V, hipStream_t stream);  // linearise, build, begin
extern "C" void afv_launch_lba_trial(const LbView *V, hipStream_t stream);      // invert, schur, solve, step, trial, judge
extern "C" void afv_launch_lba_check(const LbView *V, int final_check, hipStream_t stream);
extern "C" void afv_launch_lba_finish(const LbView *V, const DevLbaFinish *F, hipStream_t stream);
extern "C" void afv_launch_lba_trial_head(const LbView *V, hipStream_t stream);  // invert: what stands before the solve of either route
extern "C" void afv_launch_lba_trial_tail(const LbView *V, hipStream_t stream);  // step, trial, judge: what stands after it

// ---- k_gba.hip: the block-sparse solve of afv_table_global_bundle_adjust and afv_points_correct_se3 (the arithmetic: afv_gba_math.h) ----
struct GbView;
struct DevGbaCorrect {       // k_gba_correct_points: a kernel argument
    float *pos[3];           // the store's position planes
    const uint8_t *flags;
    const int *ids, *pair;   // [n]; pair: a position in T_before / T_after, -1: none
    const float *T_before, *T_after;  // [m][12]: R row-major, t
    uint8_t *status;         // [n]
    int n;
};
extern "C" void afv_launch_gba_solve(const LbView *V, const GbView *G, hipStream_t stream);  // schur (and the zeroing of the fill), factor
extern "C" void afv_launch_gba_correct_points(const DevGbaCorrect *J, hipStream_t stream);

// ---- k_refresh.hip: ComputeDistinctiveDescriptors / UpdateNormalAndDepth of resident map points (host side: afv_refresh.hip) ----
struct DevRefresh {          // a kernel argument of both launches
    DevPointPlanes P;        // the store, written in place
    const uint8_t *desc;     // the table's rows [nsets][cap][4 * words]
    const float *sigma2;     // the table's sigma2 plane [nsets][cap]
    const float *size;       // the table's keyPtsSize plane [nsets][cap] (normals only)
    int cap, desc_bytes, float_dim;
    const int *slots;        // [nk]
    const float *centres, *max_size;  // [nk][3], [nk]
    const uint8_t *kf_bad;   // [nk]
    const int *point_ids, *ref_kf, *pt_ptr;  // [np], [np], [np + 1]
    const int *obs_kf, *obs_idx;      // [ne]
    int np;
    int *c_row, *c_obs;      // [ne] scratch: table row and observation of the c-th good observation of a point, at pt_ptr[p] + c
    int *status, *best_obs, *best_median;  // [np]
    int desc_writes_status;  // the descriptor launch is the only one
};
extern "C" void afv_launch_refresh_desc(const DevRefresh *A, hipStream_t stream);
extern "C" void afv_launch_refresh_normals(const DevRefresh *A, hipStream_t stream);

// ---- k_init.hip: Initializer::Initialize between two resident frames (host side: afv_init.hip) ----
#define AFV_INIT_PREP_T 256  // lanes of k_init_prepare (I5: the width of Normalize's partial sums)
#define AFV_INIT_REC_T 512   // lanes of k_init_reconstruct: 8 wavefronts over the 8 motion hypotheses of H or the 4 of F
struct DevInitArgs {         // a kernel argument of the three launches
    const float *x1, *y1, *x2, *y2;  // mvKeysUn of the two frames, read in place
    int n1, n2;
    const int *matches12;    // [n1]
    int iterations, mask_words;      // mask_words: what the host's count of the matches needs, at least 1
    unsigned long long seed;
    float fx, fy, cx, cy, sigma;
    int *n;                  // N
    int *pairs;              // [n1][2] (i1, i2) in ascending i1
    float *norm;             // [2][4] meanX, meanY, sX, sY of frame 1, frame 2
    int *sets;               // [iterations][8]
    float *score;            // [2][iterations]
    float *model;            // [2][iterations][9]
    uint8_t *degenerate;     // [2][iterations]
    uint32_t *inliers;       // [2][iterations][mask_words]
    float *cosv;             // [8][n1] CheckRT's cosines by match
    float *p3dk;             // [8][n1][3] its points by match
    uint8_t *status;         // [8][n1] by match: bit 0 pushed (counted in nGood), bit 1 isGood
    afv_init_trace *trace;
    int *answer;             // ok, route
    float *Rt;               // R21[9], t21[3]
    float *p3d;              // [n1][3]
    uint8_t *triangulated;   // [n1]
};
extern "C" void afv_launch_init(const DevInitArgs *args, hipStream_t stream);

// ---- k_pnp.hip: PnPsolver's constructor, all its EPnP RANSAC hypotheses and the refinement of every record (host side: afv_pnp.hip) ----
#define AFV_PNP_T 256        // lanes per workgroup of k_pnp_gather
struct DevPnpCand {          // one candidate: the caller's record
    unsigned long long seed;
    int min_inliers;
    float epsilon, th2;
    int pad;
};
struct DevPnpArgs {          // a kernel argument of the three launches
    const DevPnpCand *cands;
    const int *pts;          // [nc][nf] point id | -1
    int nc, nf, nhyp, mask_words;
    const float *x, *y, *sigma2;  // the frame: mvKeysUn and the sigma2 plane over nf features, read in place
    float fx, fy, cx, cy;
    const float *pos[3];     // the store: XYZ planes and flags over `pcap` ids
    const uint8_t *flags;
    int pcap;
    int *n, *min_inliers, *index;  // [nc], [nc], [nc][nf]
    float *p2d, *p3dw, *max_err;   // [nc][nf][2], [nc][nf][3], [nc][nf]
    int *count;              // [nc][nhyp]
    uint8_t *degenerate;     // [nc][nhyp]
    float *pose;             // [nc][nhyp][12]
    uint32_t *inliers;       // [nc][nhyp][mask_words]
    uint8_t *refined;        // [nc][nhyp]
    int *refined_count;
    float *refined_pose;
    uint32_t *refined_inliers;
};
extern "C" void afv_launch_pnp(const DevPnpArgs *args, hipStream_t stream);

// ---- k_poseopt.hip: Optimizer::PoseOptimization on a resident frame (host side: afv_poseopt.hip) ----
struct DevPoseOut {          // what the workgroup of a job leaves
    float R[9], t[3];
    int n_good, n_edges, rounds;
    int iterations[4], trials[4];
    double chi2[4], lambda[4];
};
struct DevPoseArgs {         // k_pose_optimize: a kernel argument
    const float *pos[3];     // the store: XYZ planes and flags over `cap` ids
    const uint8_t *flags;
    int cap;
    const float *x, *y, *ur, *inf;  // the frame: mvKeysUn, mvuRight, keyPtsInf over n features, read in place
    int n;
    float fx, fy, cx, cy, bf;
    const int *pts;          // [njobs][n] point id | -1
    const float *poses;      // [njobs][12] Rcw row-major, tcw
    DevPoseOut *out;         // [njobs]
    uint8_t *outlier;        // [njobs][n]
};
extern "C" void afv_launch_pose_optimize(const DevPoseArgs *args, int njobs, hipStream_t stream);

extern "C" void afv_launch_bow_transform(const DevVocab *v, const uint32_t *desc, int n, int levelsup, int *leaf_node,
                                         int *node_at_level, int *rank_at_level, hipStream_t stream);
extern "C" int afv_launch_bow_transform_f32(const DevVocab *v, const float *desc, int n, int dim, int levelsup, int *leaf_node, int *node_at_level,
                                            int *rank_at_level, hipStream_t stream);
// BowVector / L1 score kernels (k_bowvec.hip)
struct DevBowQuery {
    const int32_t *word;
    const double *value;
    int n;
    int pad;
};
extern "C" void afv_launch_bowvec_build(const int *leaf, int n, const double *weight, const int32_t *word_id, const double *word_weight,
                                        int32_t *out_word, double *out_value, int *out_n, hipStream_t stream);
extern "C" void afv_launch_score_bow(const DevBowQuery *q, int nq, const int32_t *bow_word, const double *bow_value, const int32_t *bow_n,
                                     const uint8_t *slot_state, int nsets, int cap, int32_t *common, double *score, int32_t *first_common,
                                     hipStream_t stream);
#define AFV_BOW_MAX_ENTRIES 8192  // entries of one BowVector the kernels take (= AFV_MAX_SIDE, the largest frame)
struct afv_vocab {
    DevVocab dev{};
    int desc_bytes = 32;
    int float_dim = 0;           // > 0: node descriptors are float_dim floats (afv_vocab_create_f32), `desc_bytes` = 4 * float_dim
    void *d_rec = nullptr;       // breadth-first records (k_bow.hip)
    uint8_t *d_stopped = nullptr;
    std::vector<uint8_t> h_stopped;  // host copy of the stop list (empty: none)
    std::vector<int> depth_width;    // nodes per depth (index = depth, 0 = the root)
    double *d_weight = nullptr;      // [nnodes] by DBoW2 node id (afv_vocab_set_weights; nullptr: the vocabulary builds no BowVectors)
    int32_t *d_word_id = nullptr;    // [nnodes] word id of a leaf, -1 for inner nodes
    double *d_word_weight = nullptr; // [largest word id + 1] the leaf weights again, by word id
};

// the device-resident Frame (afv_frame.hip)
struct afv_frame {
    afv_ctx *c = nullptr;
    afv_frame_params p{};
    int cap = 0, n = 0;
    int desc_bytes = 32, words = 8;  // descriptor size and dwords per (zero-padded) device row: 8 up to 32 bytes, 16 up to 64
    int float_dim = 0;               // > 0: the rows are float_dim floats (desc_bytes = 4 * float_dim, words = float_dim): L2^2 distances
    float inv_w = 0, inv_h = 0;
    bool has_features = false, has_grid = false, has_fv = false;
    // device arrays, one allocation
    uint8_t *d_block = nullptr;
    afv_keypoint *d_kps = nullptr;
    uint8_t *d_desc = nullptr;
    float *d_x = nullptr, *d_y = nullptr, *d_size = nullptr, *d_angle = nullptr, *d_sigma2 = nullptr, *d_inf = nullptr, *d_ur = nullptr;
    int *d_n = nullptr, *d_cell_ptr = nullptr, *d_leaf = nullptr, *d_nid = nullptr, *d_dense = nullptr, *d_seg_idx = nullptr, *d_nkept = nullptr;
    int4 *d_cell_ent = nullptr;
    uint8_t *d_oct0 = nullptr;         // octave == 0 per feature (the query filter of SearchForInitialization)
    // host side of the FeatureVector: node structure for the merge-join
    std::vector<int32_t> fv_node_id, fv_seg_ptr;
    int fv_total = 0;
    // the BowVector (afv_frame_bow_transform on a vocabulary with weights): entries ascending by word id
    int32_t *d_bow_word = nullptr;   // [cap]
    double *d_bow_value = nullptr;   // [cap]
    int *d_bow_n = nullptr;
    bool has_bow = false;
    int bow_n = 0;
    // stereo / RGB-D (afv_stereo.hip): mvDepth next to d_ur, the test outputs of the stereo search, the kept pyramid
    float *d_depth = nullptr;        // [cap]
    int *d_sad = nullptr, *d_best_r = nullptr, *d_nstereo = nullptr;  // [cap], [cap], one int
    bool has_depth = false;          // d_depth holds values (else mvDepth reads -1)
    bool has_stereo = false;         // d_sad / d_best_r hold the last afv_frame_stereo_match
    uint8_t *d_pyr = nullptr;        // the frame's own pyramid: level l tightly packed at pyr_off[l] (an allocation of its own, made on first use)
    size_t pyr_bytes = 0, pyr_off[AFV_MAX_LEVELS]{};
    int pyr_levels = 0, pyr_w[AFV_MAX_LEVELS]{}, pyr_h[AFV_MAX_LEVELS]{};
    bool has_pyramid = false;
    // afv_frame_set_pose (afv_points.hip): what k_points_project takes as kernel arguments
    bool has_pose = false;
    float Rcw[9]{}, tcw[3]{}, Ow[3]{}, fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
};

// the device-resident map-point store (afv_points.hip)
struct afv_points {
    afv_ctx *c = nullptr;
    int cap = 0;
    int desc_bytes = 32, words = 8, float_dim = 0;  // as afv_frame
    uint8_t *d_block = nullptr;  // the planes, one allocation
    DevPointPlanes P{};
    uint8_t *d_stage = nullptr;  // device staging of the setters / afv_points_get (grow-only)
    size_t stage_bytes = 0;
    uint8_t *h_pin = nullptr;    // its pinned host image: a setter fills it, uploads it and returns
    size_t pin_bytes = 0;
    hipEvent_t ev = nullptr;     // the last upload out of h_pin (the next setter waits for it before it refills the image)
    bool ev_armed = false;
    uint32_t *d_covis = nullptr; // afv_table_local_points (afv_covis.hip): [2][cap] first-occurrence words (0xFFFFFFFF at rest), positions; made on first use
};

#define AFV_MAX_SIDE 8192

struct afv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // second lane for split batches (fills the ramps, tails and latency-bound kernels of the first)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t stream_copy = nullptr;                         // copy lane of the host-buffer batch pipeline (created on first use)
    std::vector<hipEvent_t> pipe_ev;                           // 3 events per chunk in flight
    int pipe_chunk = 64;                                       // frames per pipeline chunk
    int pipe_ahead = 8;                                        // uploads run this many chunks ahead of the compute
    int split_min_frames = 64;     // batches of at least this many frames / pairs are split over the two streams
    int match_engine = AFV_MATCH_ENGINE_MFMA;  // phase 1 of the brute-force pair matcher; afv_set_match_engine
    int resolve_engine = 2;        // phase 2: 0 = ordered walk on one wavefront (64-row rounds), 1 = workgroup-wide fixed point, 2 = by call size
    int resolve_wg_max_pairs = 256; // ... 2: calls of at most this many pairs take the fixed point; afv_set_match_resolve
    int proj_engine = 2;           // ordered phase of the projection searches: 0 = ordered walk, 1 = workgroup fixed point, 2 = 1 when it fits
    int proj_wg_lds_max = 0;       // dynamic LDS bytes the workgroup engines may use (0: unavailable); afv_project_prepare at afv_create
    int frame_lds_max = 0;         // dynamic LDS bytes k_frame_grid / k_featvec_build may use; afv_frame_prepare at afv_create
    int *d_proj_ticket = nullptr;  // hand-off ticket of the one-launch search (k_proj_search1), zero at rest
    int *d_points_count = nullptr; // k_points_project: {in-view accumulator, workgroup ticket}, zero at rest (made with the first map-point store)
    int proj_fuse = 1;             // 1: single-job searches rank and resolve in one launch (afv_set_projection_fuse)
    std::vector<afv_frame *> frames;  // frames alive on this context (destroyed with it)
    std::vector<afv_points *> points; // ... and its map-point stores (afv_points.hip)
    int split_chunks = 0;          // ... into this many chunks; 0 = about 85 frames each; afv_set_split_chunks
    int split_schedule = 1;        // 1: a lane per half of the batch, its pyramid first, the caller's lane ends last; the pair matcher unsplit
                                   // 0: chunks alternating over the lanes, the matcher split too; afv_set_split_schedule
    // small-batch ("latency") path: kernels shaped for one or a few frames; afv_set_small_batch_path
    int small_mode = 1;            // 0 = never, 1 = batches of at most small_max_frames, 2 = always
    int small_max_frames = 4;
    int pf_tw = 16, pf_th = 8;     // top-level tile of the one-launch pyramid (k_pyramid_fused): 204 workgroups for one 640 x 480 frame - the
                                   // kernel's level loop is bound by the vector ALU of the CUs it runs on (32 x 16 tiles: 54 CUs, 7.7 us of levels)
    bool pf_ok = false;            // the current geometry has a one-launch pyramid (else: level-by-level launches)
    PyrFuseArgs pf{};
    size_t pf_lds = 0;
    uint8_t *d_pf_blob = nullptr;  // device image of the plan (afv_device.h)
    size_t pf_blob_cap = 0;
    afv_orb_params p{};
    Geo geo{};          // current geometry (host copy)
    Geo cap_geo{};      // geometry of (max_width, max_height): sizes every allocation
    Geo *d_geo = nullptr;
    bool geo_valid = false;
    short2 *d_tab = nullptr;  // resize tables, all levels
    size_t tab_off_x[AFV_MAX_LEVELS]{}, tab_off_y[AFV_MAX_LEVELS]{};
    size_t tab_elems = 0;
    uint8_t *d_pyr = nullptr;
    uint32_t *d_cand_packed = nullptr, *d_kept_xy = nullptr;
    uint32_t *d_l1 = nullptr;          // per (frame, level): the candidates that survive retainBest on the FAST score ...
    float *d_l1_resp = nullptr;        // ... and their Harris responses
    int *d_l1_count = nullptr;
    uint2 *d_hq = nullptr;             // Harris work queue, `hq_per_frame` items per frame; a launch over the frames
    int *d_hq_n = nullptr;             // [f0, f0 + nf) owns the slice starting at frame f0 and the counter d_hq_n[f0]
    size_t hq_per_frame = 0;
    float *d_kept_resp = nullptr;
    uint16_t *d_kept_node = nullptr;
    int *d_cand_count = nullptr, *d_sel_count = nullptr;
    SelPoint *d_sel = nullptr;
    int select_M = 64;
    bool select_wide_ok = true;   // the 1024-thread quadtree kernel got its LDS (afv_select_prepare at afv_create)
    // staging of the host-pointer entry points
    uint8_t *d_frames = nullptr;
    size_t frames_pitch = 0, frames_stride = 0;
    uint8_t *d_out_block = nullptr;  // [n][kps][desc] of the host-pointer calls in one allocation; the three pointers below point into it
    size_t out_kps_off = 0, out_desc_off = 0, out_bytes = 0;
    afv_keypoint *d_kps = nullptr;
    uint8_t *d_desc = nullptr;
    int *d_n = nullptr, *d_status = nullptr;
    int stage_cap = 0;
    // matcher staging (grow only)
    uint8_t *d_match = nullptr;
    size_t match_bytes = 0;
    uint8_t *h_stage = nullptr;  // pinned host image of d_match (matcher staging both ways), grow-only
    size_t stage_bytes = 0;
    bool stage_pinned = false;
    void *d_topk = nullptr;  // [npairs][cap] 2 x int4: key record per row (seven (distance, column) keys + the exact-prefix length)
    size_t topk_bytes = 0;
    // column-sliced phase 1 (small-batch path): per-slice records [npairs][cap][nslices] 2 x int4 and the row-tile tickets (zero at rest)
    void *d_l2_scratch = nullptr;  // key records of the float-descriptor pair matcher (afv_match_l2_pairs_device), its own buffer
    size_t l2_bytes = 0;
    int l2_chunk_pairs = 2048;     // pairs per launch of that matcher; afv_set_l2_chunk_pairs
    void *d_slice = nullptr;
    size_t slice_bytes = 0;
    int *d_tickets = nullptr;
    size_t tickets_n = 0;
    // last extraction (debug getters)
    FrameSrc last_src{};
    int last_nframes = 0;
    std::string last_error;
    // live stage timing
    bool prof = false;             // the CURRENT call is timed (set per entry-point call from prof_every and the call counters)
    int prof_every = 0;            // 0 = profiling off; n = time the stages of every n-th extraction / pair-match call
    unsigned prof_tick_extract = 0, prof_tick_match = 0;
    std::vector<hipEvent_t> prof_ev[AFV_NUM_STAGES];  // pairs (begin, end)
    size_t prof_used[AFV_NUM_STAGES]{};
    int prof_launches[AFV_NUM_STAGES]{};
    float prof_ms[AFV_NUM_STAGES]{};
    long long prof_units[AFV_NUM_STAGES]{};  // frames (pairs for the match stage) covered by the timed launches
};

struct StageTimer {  // RAII: record begin/end events around one stage on the launch stream
    afv_ctx *c;
    int stage;
    hipStream_t s;
    hipEvent_t e1 = nullptr;
    StageTimer(afv_ctx *c_, int stage_, hipStream_t s_, int units = 0) : c(c_), stage(stage_), s(s_) {
        if (!c->prof) return;
        c->prof_units[stage] += units;
        auto &v = c->prof_ev[stage];
        size_t &u = c->prof_used[stage];
        if (u + 2 > v.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            v.push_back(a);
            v.push_back(b);
        }
        (void)hipEventRecord(v[u], s);
        e1 = v[u + 1];
        u += 2;
    }
    ~StageTimer() {
        if (e1) (void)hipEventRecord(e1, s);
    }
};

// Fills and device-to-device copies that a later launch depends on.  hipMemset / hipMemcpy(device -> device) run on the NULL stream and
// may return before they have run; the contexts' streams are created non-blocking, so nothing orders a launch on them behind such an
// operation (round 6: a fresh context's first sliced match could meet ticket words the fill had not reached yet - or have its counts
// wiped by a fill that ran late).  These run on the context's own stream and the host waits for them.
static inline hipError_t afv_fill(afv_ctx *c, void *p, int v, size_t n) {
    if (!n) return hipSuccess;
    const hipError_t e = hipMemsetAsync(p, v, n, c->stream);
    return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}
static inline hipError_t afv_copy_dd(afv_ctx *c, void *dst, const void *src, size_t n) {
    if (!n) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDefault, c->stream);
    return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

// the small-batch ("latency") path: kernels shaped for one or a few frames / pairs; afv_set_small_batch_path
static inline bool small_batch_path(const afv_ctx *c, int nf) { return c->small_mode == 2 || (c->small_mode == 1 && nf <= c->small_max_frames); }
// phase 2 of a brute-force pair call.  The workgroup-wide fixed point is the faster form while every pair has a CU to itself (one pair of
// unrelated frames 23 -> 10 us, of overlapping video frames 61 -> 28 us; 256 overlapping pairs per call: 0.16 against 0.19 ms of
// resolve tail), but it evaluates every live row in every pass: a batch that fills the chip several times over is throughput-bound
// and faster with the one-wavefront walk (10 000 jobs: 3.52 M jobs/s against 3.30 M)
static inline int resolve_engine_for(const afv_ctx *c, int npairs) {
    return c->resolve_engine == 2 ? (npairs <= c->resolve_wg_max_pairs ? 1 : 0) : c->resolve_engine;
}

// versioned job arrays (include/afv_hip.h, "JOB RECORDS THAT CARRY struct_size"): the caller's array, whatever layout it was compiled
// against, copied into the current one; fields its layout does not have are zero.  false = AFV_EINVAL (missing / inconsistent / absurd
// struct_size)
template <class T>
static inline bool afv_load_jobs(const T *jobs, int njobs, size_t first_layout_bytes, std::vector<T> &out) {
    if (!jobs || njobs < 1) return false;
    const uint8_t *base = reinterpret_cast<const uint8_t *>(jobs);
    uint32_t ss;
    std::memcpy(&ss, base, sizeof(ss));
    if (ss < first_layout_bytes || ss > 4 * sizeof(T) || (ss & 3)) return false;
    out.resize((size_t)njobs);
    for (int i = 0; i < njobs; ++i) {
        const uint8_t *p = base + (size_t)i * ss;
        uint32_t si;
        std::memcpy(&si, p, sizeof(si));
        if (si != ss) return false;
        std::memset(static_cast<void *>(&out[i]), 0, sizeof(T));
        std::memcpy(static_cast<void *>(&out[i]), p, std::min<size_t>(ss, sizeof(T)));
        out[i].struct_size = (uint32_t)sizeof(T);
    }
    return true;
}

// ---- matcher staging ----
// Host image of the device staging buffer.  It lives in the context's pinned arena, so the one H2D copy of a call and the
// D2H copies of its results are true async DMA transfers (no pageable bounce inside the runtime); results land at the same
// offsets in the arena and are handed to the caller's arrays after the stream sync.
struct HostImage {
    afv_ctx *c;
    size_t n = 0;
    uint8_t *data() { return c->h_stage; }
    size_t size() const { return n; }
    void resize(size_t m, bool zero) {
        if (m > c->stage_bytes) {
            const size_t want = align_up(m + m / 2, 1 << 20);
            uint8_t *np = nullptr;
            bool pinned = hipHostMalloc(reinterpret_cast<void **>(&np), want, hipHostMallocDefault) == hipSuccess && np;
            if (!pinned) {
                (void)hipGetLastError();
                np = static_cast<uint8_t *>(std::malloc(want));
                if (!np) throw std::bad_alloc();
            }
            if (n) std::memcpy(np, c->h_stage, n);
            if (c->h_stage) {
                if (c->stage_pinned) (void)hipHostFree(c->h_stage);
                else std::free(c->h_stage);
            }
            c->h_stage = np;
            c->stage_bytes = want;
            c->stage_pinned = pinned;
        }
        if (zero && m > n) std::memset(c->h_stage + n, 0, m - n);
        n = m;
    }
};

struct Blob {
    HostImage h;
    struct Pending { void *dst; size_t off, bytes; };
    std::vector<Pending> pending;
    explicit Blob(afv_ctx *c) : h{c} {}
    size_t put(const void *src, size_t bytes, size_t align = 16) {
        const size_t off = align_up(h.size(), align);
        h.resize(off + bytes, src == nullptr);
        if (src && bytes) std::memcpy(h.data() + off, src, bytes);
        return off;
    }
    size_t reserve(size_t bytes, size_t align = 16) {  // zero-filled (counters, histograms, padded rows rely on it)
        const size_t off = align_up(h.size(), align);
        h.resize(off + bytes, true);
        return off;
    }
    size_t reserve_scratch(size_t bytes, size_t align = 16) {  // device-only scratch: never copied, never filled
        const size_t off = align_up(h.size(), align);
        h.resize(off + bytes, false);
        return off;
    }
    // queue a device -> caller copy of [off, off + bytes): DMA into the arena now, memcpy to dst in finish()
    hipError_t fetch(void *dst, size_t off, size_t bytes, hipStream_t s) {
        if (!bytes) return hipSuccess;
        pending.push_back(Pending{dst, off, bytes});
        return hipMemcpyAsync(h.data() + off, h.c->d_match + off, bytes, hipMemcpyDeviceToHost, s);
    }
    void finish() {
        for (const Pending &p : pending) std::memcpy(p.dst, h.data() + p.off, p.bytes);
        pending.clear();
    }
    // the call's one host -> device copy: the first in_bytes of the image (the inputs and the records) on the context's stream
    AFV_LOCAL hipError_t upload(size_t in_bytes) { return hipMemcpyAsync(h.c->d_match, h.data(), in_bytes, hipMemcpyHostToDevice, h.c->stream); }
    // the end of a call: the host waits for the stream, then the fetched ranges go to the caller's arrays
    AFV_LOCAL hipError_t wait() {
        const hipError_t e = hipStreamSynchronize(h.c->stream);
        if (e == hipSuccess) finish();
        return e;
    }
};

// scratch of a column-sliced phase 1 over `npairs` pairs (grow-only; growing implies a device sync, tickets are zeroed once)
static inline int ensure_slice_scratch(afv_ctx *c, int npairs, int cap, int nslices) {
    if (nslices <= 1) return AFV_OK;
    const size_t need = (size_t)npairs * cap * 32 * nslices, nt = (size_t)npairs * ((cap + 255) / 256);
    if (need > c->slice_bytes || nt > c->tickets_n) HIPCHK(c, hipDeviceSynchronize());
    if (need > c->slice_bytes) {
        if (c->d_slice) (void)hipFree(c->d_slice);
        c->d_slice = nullptr;
        c->slice_bytes = 0;
        HIPCHK(c, hipMalloc(&c->d_slice, need));
        c->slice_bytes = need;
    }
    if (nt > c->tickets_n) {
        if (c->d_tickets) (void)hipFree(c->d_tickets);
        c->d_tickets = nullptr;
        c->tickets_n = 0;
        HIPCHK(c, hipMalloc(&c->d_tickets, nt * sizeof(int)));
        HIPCHK(c, afv_fill(c, c->d_tickets, 0, nt * sizeof(int)));
        c->tickets_n = nt;
    }
    return AFV_OK;
}

static inline int ensure_match_buffer(afv_ctx *c, size_t bytes) {
    if (bytes <= c->match_bytes) return AFV_OK;
    if (c->d_match) (void)hipFree(c->d_match);
    c->d_match = nullptr;
    c->match_bytes = 0;
    const size_t want = align_up(bytes + bytes / 2, 1 << 20);
    HIPCHK(c, hipMalloc(&c->d_match, want));
    c->match_bytes = want;
    return AFV_OK;
}

// descriptors -> rows of `words` dwords (zero padded)
static inline size_t put_desc(Blob &b, const uint8_t *d, int n, int desc_bytes, int words) {
    const size_t off = b.reserve((size_t)std::max(n, 1) * words * 4);
    for (int i = 0; i < n; ++i) {
        uint8_t *row = b.h.data() + off + (size_t)i * words * 4;
        std::memset(row, 0, (size_t)words * 4);
        std::memcpy(row, d + (size_t)i * desc_bytes, (size_t)desc_bytes);
    }
    return off;
}

// ---- the keyframe table (afv_comm.hip; afv_frame.hip gathers query descriptors from it) ----
struct HostFeatVec {  // host copy of one keyframe's FeatureVector (node ids, CSR pointers, feature indices)
    std::vector<int32_t> node_id, seg_ptr, seg_idx;
};

struct KfPose {  // afv_table_set_pose
    float R[9], t[3], Ow[3], fx, fy, cx, cy, mbf;
};
struct afv_table {
    afv_ctx *c = nullptr;
    int nsets = 0, cap = 0;
    int desc_bytes = 32, words = 8;  // descriptor size and dwords per zero-padded row: 8 up to 32 bytes, 16 up to 64 (afv_table_create_bytes)
    int float_dim = 0;               // > 0: rows of float_dim floats (afv_table_create_f32): desc_bytes = 4 * float_dim, words = float_dim, no padding - the fields of a float frame
    uint8_t *d_desc = nullptr;  // [nsets][cap][4 * words]
    float *d_angle = nullptr;   // [nsets][cap]
    int32_t *d_n = nullptr;     // [nsets]
    int32_t *d_idx = nullptr;   // [nsets][cap] FeatureVector feature indices in node order (afv_table_set_featvec), lazily allocated
    float *d_geo = nullptr;     // [4][nsets][cap]: x, y, sigma2, mvuRight (afv_table_set_geometry / _u_right; -1 = monocular), lazily allocated
    float *d_scale = nullptr;   // [4][nsets][cap]: keyPtsSize, mvDepth (-1 = none), distorted mvKeys x, y (afv_table_set_scale), lazily allocated
    uint8_t *d_valid = nullptr; // [nsets][cap] "map point exists && !isBad()" (afv_table_set_valid), lazily allocated, default 1
    std::vector<int32_t> h_n;
    std::vector<HostFeatVec> fv;
    std::vector<uint8_t> has_fv, has_geo;  // per set: afv_table_set_featvec / afv_table_set_geometry called since the last afv_table_set
    std::vector<uint8_t> has_scale;        // per set: afv_table_set_scale called (or a frame promoted) since the last afv_table_set
    float *d_inf = nullptr;     // [nsets][cap] GetKeyPt2DInf (afv_table_set_inf / a promoted frame's keyPtsInf), lazily allocated
    std::vector<uint8_t> has_inf;          // per set: the information plane was stored since the last afv_table_set
    std::vector<uint8_t> fv_body_on_device;  // per set: the FeatureVector body came from a frame (afv_table_set_from_frame): no host copy yet
    // BowVector planes (afv_table_set_bowvec / afv_table_set_from_frame), lazily allocated together
    int32_t *d_bow_word = nullptr;  // [nsets][cap] word ids ascending
    double *d_bow_value = nullptr;  // [nsets][cap]
    int32_t *d_bow_n = nullptr;     // [nsets]
    std::vector<int32_t> h_bow_n;
    std::vector<uint8_t> has_bow;   // per set: a BowVector was stored since the last afv_table_set
    // grow-only device buffers of the pair entry points + their pinned host image
    int32_t *d_pairs = nullptr;  // [2][pair_cap]
    int32_t *d_out = nullptr;    // [pair_cap][cap]
    int32_t *d_nm = nullptr;     // [pair_cap]
    int32_t *h_pin = nullptr;    // pinned: [2][pair_cap] pairs, then [pair_cap] counts, then [pair_cap][cap] matches
    int pair_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // fusing map points into slots (afv_kffuse.hip): the camera, a pose per slot (host side: it travels as a job record), the keyframe's
    // mvpMapPoints and the grid of KeyFrame::GetFeaturesInArea per slot; everything lazily allocated
    bool has_camera = false;
    afv_table_camera cam{};
    std::vector<KfPose> kf_pose;               // [nsets] once a pose or a plane was set
    std::vector<uint8_t> kf_has_pose, kf_has_mp, kf_grid_ok;  // per set; kf_grid_ok: the slot's grid is that of its planes and the camera
    int32_t *d_mp = nullptr;         // [nsets][cap] point id | -1
    int *d_kf_cell_ptr = nullptr;    // [nsets][grid_cols * grid_rows + 1]
    int4 *d_kf_cell_ent = nullptr;   // [nsets][cap]
    int kf_cells = 0;                // cells the grid planes were allocated for
};
// afv_comm.hip, for the scratch test hooks (afv_api.hip): the pair buffers of every table of context `c`, in the order the tables were
// made - per table d_pairs, d_out, d_nm appended to `dev`, the pinned image h_pin to `pin`
struct ScratchSeg { void *p; size_t n; };
AFV_LOCAL void afv_tables_pair_scratch(afv_ctx *c, std::vector<ScratchSeg> &dev, std::vector<ScratchSeg> &pin);
// afv_kffuse.hip: what the table's own entry points (afv_comm.hip) tell the fuse state of a slot
AFV_LOCAL void afv_kffuse_slot_reset(afv_table *t, int slot);   // afv_table_set / a promoted frame: pose, plane and grid are forgotten
AFV_LOCAL void afv_kffuse_grid_stale(afv_table *t, int slot);   // the geometry or the scale planes changed (slot < 0: every slot)
AFV_LOCAL int afv_kffuse_clone(const afv_table *src, afv_table *dst);
AFV_LOCAL void afv_kffuse_free(afv_table *t);
AFV_LOCAL int afv_kffuse_broadcast(afv_comm *m, afv_table *t, int root);  // behind the planes of afv_table_broadcast, on every rank

// ---- the pair matchers (afv_api.hip), shared with afv_comm.hip ----
int afv_match_pairs_core(afv_ctx *c, const uint8_t *d_desc, const float *d_ang, int ang_stride, const int32_t *d_n, int cap,
                         const int32_t *d_pair_a, const int32_t *d_pair_b, int npairs, float th_low, float nnratio,
                         int check_orientation, int32_t *d_match, int32_t *d_nmatches, hipStream_t s, int words);
// chunked launches of the float pair matcher (k_match_l2.hip) behind afv_match_l2_pairs_device and the pair entry points of a float table;
// d_ang != null: ang[set][cap] in degrees, the rotation histogram is applied
int afv_match_l2_pairs_core(afv_ctx *c, const float *d_desc, const float *d_ang, const int32_t *d_n, int cap, int dim, const int32_t *d_pair_a,
                            const int32_t *d_pair_b, int npairs, float th_low, float nnratio, int32_t *d_match, int32_t *d_nmatches, hipStream_t s);
// ---- the BoW-guided matchers and SearchForTriangulation (afv_match_jobs.hip): one staging and launch path behind the host-array, table-slot
// and frame entry points ----
// A FeatureVector as CSR over `nnodes` ascending node ids, for a side of n features: seg_ptr[0] == 0, monotone pointers, strictly ascending
// ids, seg_ptr[nnodes] <= n, every index in [0, n) and listed once (DBoW2 puts a feature into the one node it descends through; the per-node
// kernels rely on it).  AFV_OK or AFV_EINVAL; O(n)
int afv_featvec_check(const int32_t *node_id, const int32_t *seg_ptr, const int32_t *seg_idx, int nnodes, int n);
struct MatchSide {  // where one side of a job lives
    int n = 0;
    int desc_bytes = 32, words = 8, fdim = 0;  // row width, dwords per device row, floats per row (0: binary)
    bool on_device = false;          // rows / idx / angle / geometry are device pointers (table slot, resident frame); else host arrays to stage
    const uint8_t *rows = nullptr;   // host: n packed rows of desc_bytes
    const int32_t *idx = nullptr;    // FeatureVector feature indices in node order; null: identity
    const int32_t *idx_host = nullptr;  // host copy of a device `idx` (the row map of triangulation reads it)
    const uint8_t *valid = nullptr;  // [n] or null; its own flag: triangulation over the table brings host masks to device rows
    bool valid_on_device = false;
    const float *angle = nullptr;
    const int32_t *node_id = nullptr, *seg_ptr = nullptr;  // host, always
    int nnodes = 0;
    const float *x = nullptr, *y = nullptr, *sigma2 = nullptr, *u_right = nullptr;  // triangulation only
};
struct MatchJobSpec {  // one job: its sides (indices into MatchBatch::sides) and settings
    int side1, side2;
    float th, ratio;
    int check_ori, mode;  // AFV_MATCH_KF_KF / AFV_MATCH_KF_FRAME
    const float *F12 = nullptr;  // triangulation: fundamental matrix, epipole, bOnlyStereo
    float ex = 0, ey = 0;
    int only_stereo = 0;
};
struct MatchBatch {
    std::vector<MatchSide> sides;  // a side that several jobs name is staged once
    std::vector<MatchJobSpec> jobs;
    bool tri = false;          // SearchForTriangulation (else SearchByBoW)
    bool whole_range = false;  // a side without nodes = one segment over both sides (brute force: host arrays); else no segment (tables)
    bool per_node = false;     // always the per-node kernel (tables); else only when a job has more than one segment
    int out_stride = 0;        // > 0: out[njobs][out_stride]; 0: ragged rows of n1 (KF-Frame: n2) ints per job, packed
};
// out may be null (counts only); rows start at -1, nmatches[njobs]
int afv_match_jobs_run(afv_ctx *c, const MatchBatch &B, int32_t *out, int32_t *nmatches);
// the pieces of the table routes that afv_newpoints.hip stages itself (its launches are not those of afv_match_jobs_run):
// afv_match_jobs.hip - the merge-join of two FeatureVectors and the feature -> shared node map of side 1;
// afv_comm.hip - a slot as a side, "the slot holds what the call needs", the host copy of a promoted slot's FeatureVector body;
// afv_triangulate.hip - the slot check of afv_table_triangulate and the device record of a pair
AFV_LOCAL void join_featvecs(const MatchSide &A, const MatchSide &B, bool whole_range, std::vector<Seg> &segs);
AFV_LOCAL int build_row_seg(const MatchSide &A, const Seg *segs, int nseg, std::vector<int> &row_seg);
AFV_LOCAL MatchSide table_side(const afv_table *t, int slot);
AFV_LOCAL int check_slot_ready(const afv_table *t, int s, bool need_geo, const char *who);
AFV_LOCAL int table_fetch_fv_body(afv_table *t, int slot);
AFV_LOCAL int tri_check_slot(const afv_table *t, int s);
AFV_LOCAL void tri_fill_pair(const afv_table *t, int a, int b, const afv_tri_points_job &j, DevTriPair &D);
// plain brute-force KF-KF jobs over 32-byte rows take the two-phase pair matcher (top-k + resolve over a table of two sets per job);
// *taken = false: the batch is not of that kind, nothing was done
int afv_match_bow_plain32(afv_ctx *c, const afv_match_job *jobs, int njobs, int32_t *out, int32_t *nmatches, bool *taken);
int afv_check_resolve_guard(afv_ctx *c, const int32_t *nmatches, int n);
void afv_table_release_all(afv_ctx *c);  // afv_destroy: tables / communicators still alive die with their context
void afv_frame_release_all(afv_ctx *c);  // ... and so do its frames
bool afv_frame_is_live(const afv_frame *f);  // afv_frame.hip: the pointer names a frame that was not destroyed
void afv_points_release_all(afv_ctx *c); // ... and its map-point stores
bool afv_points_is_live(const afv_points *p);  // afv_points.hip: the pointer names a store that was not destroyed
int afv_frame_after_extract(afv_frame *f, hipStream_t s);  // afv_frame.hip: k_frame_grid behind the describe kernel of afv_frame_extract
// afv_stereo.hip: a keep_pyramid frame takes device copies of the levels of frame slot 0 of the extraction that just ran on stream s
int afv_frame_keep_pyramid(afv_frame *f, const FrameSrc &src, hipStream_t s);
int afv_extract_into_frame(afv_ctx *c, afv_frame *f, const uint8_t *gray, int width, int height, int stride_bytes, afv_keypoint *kps,
                           uint8_t *desc32, int cap, int *n_out);  // afv_extract.hip: afv_orb_extract with the frame as second destination
// what afv_create (afv_api.hip) needs from the extractor's geometry (afv_extract.hip): level sizes, quotas and buffer layout of `max_batch`
// frames of w x h, and the bytes of the pyramid / the elements of a candidate array that layout takes.  Hidden: the library's
// dynamic symbol table stays as it was when one file held both sides
AFV_LOCAL int afv_build_geometry(const afv_orb_params &p, int w, int h, int max_batch, Geo &g);
AFV_LOCAL size_t afv_geo_pyr_bytes(const Geo &g, int max_batch);
AFV_LOCAL size_t afv_geo_cand_elems(const Geo &g, int max_batch);
// the host side of E12 (FeatureExtractor.cpp:132-172): keyPtsSize of octave `o` as afv_orb_size_sigma computes it
float afv_size_of_octave(const afv_ctx *c, int octave);
// ---- the projection searches (afv_project.hip): one staging and launch path behind the host-array entry points (afv_project.hip), the
// searches against a resident frame (afv_frame.hip) and the searches through map-point ids (afv_points.hip).  A route describes each job
// once - where every array lives - and afv_project_run stages, launches and collects ----
enum { AFV_KIND_PROJ = 0, AFV_KIND_FUSE = 1, AFV_KIND_INIT = 2 };
struct ProjSide {  // the feature side of a job: the frame searched in
    int n = 0, desc_bytes = 32, words = 8, fdim = 0;  // features; row width, dwords per device row, floats per row (0: binary)
    // desc .. u_right are device pointers and the grid (cell_ptr / cell_ent) comes with them (a resident frame); else they are host arrays
    // to stage (desc: n packed rows of desc_bytes) and k_frame_grid builds the grid behind the upload
    bool on_device = false;
    const void *desc = nullptr;
    const float *x = nullptr, *y = nullptr, *size = nullptr, *angle = nullptr, *inf = nullptr, *u_right = nullptr;
    const int *cell_ptr = nullptr;
    const int4 *cell_ent = nullptr;
    float min_x = 0, min_y = 0, inv_w = 0, inv_h = 0;  // Frame::AssignFeaturesToGrid: mnMinX / mnMinY, mfGridElementWidthInv / HeightInv
    int grid_cols = 0, grid_rows = 0;
    const uint8_t *occupied = nullptr;  // [n] or null; host, always
};
// the whole query side made on the device from the ids of resident map points (afv_points.hip): k_points_project runs ahead of the search
// kernels and writes qu .. q_er_max, qvalid, qoccupies and the gathered rows into the call's staging area
struct PointQueries {
    DevPointsJob job{};            // planes, pose, flavour, rules; afv_project_run fills in ids and the outputs
    const int32_t *ids = nullptr;  // host [nq]
    uint8_t *in_view = nullptr;    // host [nq] out, may be null
    int32_t n_in_view = 0;         // out
};
struct ProjQueries {  // the query side of a job: where each of its arrays comes from
    int nq = 0;
    enum Rows { HOST_ROWS, DEVICE_ROWS, TABLE_ROWS, POINT_IDS } from = HOST_ROWS;
    const void *desc = nullptr;              // HOST_ROWS: nq packed rows to stage; DEVICE_ROWS: rows of the feature side's pitch (another frame's)
    const afv_table *ref_table = nullptr;    // TABLE_ROWS: rows (slot, idx) of a keyframe table, gathered on the device behind the upload
    const int32_t *ref_slot = nullptr, *ref_idx = nullptr;  // ... host arrays of nq ints
    PointQueries *points = nullptr;          // POINT_IDS: rows, geometry, qvalid, qoccupies and the stereo pair are made on the device
    const uint8_t *valid = nullptr;          // [nq] or null ...
    const float *angle = nullptr;
    bool valid_on_device = false, angle_on_device = false;  // ... each a host array to stage or a device pointer
    const float *u = nullptr, *v = nullptr, *r = nullptr, *min_size = nullptr, *max_size = nullptr;  // host
    const float *ur = nullptr, *er_max = nullptr;                                                   // host, stereo only
    const uint8_t *occupies = nullptr;                                                              // host, [nq] or null
};
struct ProjJobSpec {
    ProjSide f;
    ProjQueries q;
    float th = 0, ratio = 0, tol = 0, inv_tol = 0;
    int check_ori = 0, mode = 0;
    // mvuRight takes part (FeatureMatcher.cc:114-119, :1367-1372, :880-894) - decided by the route: host arrays that carry u_right; a
    // resident frame (it always carries the plane, -1 = monocular) when the caller sends the queries' side of the gate.
    // SearchForInitialization has no such branch whatever this says
    bool stereo = false;
};
// what afv_proj_job and afv_proj_queries both carry - the queries as host arrays, the occupancy mask, the settings - into a spec
template <class T>
static inline void afv_proj_host_fields(const T &j, ProjJobSpec &J) {
    J.f.occupied = j.occupied;
    ProjQueries &q = J.q;
    q.nq = j.nq; q.desc = j.qdesc; q.valid = j.qvalid; q.angle = j.qangle; q.occupies = j.qoccupies;
    q.u = j.qu; q.v = j.qv; q.r = j.qr; q.min_size = j.qmin_size; q.max_size = j.qmax_size;
    q.ur = j.q_ur; q.er_max = j.q_er_max;
    J.th = j.th_high; J.ratio = j.nnratio; J.check_ori = j.check_orientation; J.mode = j.mode;
}
// kind: AFV_KIND_*; assign: n ints per job (PROJ) or nq (FUSE, INIT), packed in job order; nmatches[njobs].  A side or a query array on the
// device: njobs == 1
AFV_LOCAL int afv_project_run(afv_ctx *c, const ProjJobSpec *specs, int njobs, int kind, int32_t *assign, int32_t *nmatches);
// afv_frame.hip: the spec fields a resident frame decides - the frame as feature side (with_inf: keyPtsInf for the chi-square gate of Fuse)
// and the size tolerance (Frame.cc:73-74)
AFV_LOCAL ProjJobSpec afv_frame_proj_spec(const afv_frame *f, bool with_inf);
