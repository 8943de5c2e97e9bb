/*
 * afv_hip.h — C-ABI of libafv_hip.so: MI355X (gfx950) ORB32 extraction + descriptor matching.
 *
 * Drop-in boundary for AnyFeature-VSLAM's front end.  Every entry point is plain C:
 * pointers, sizes, POD structs; returns 0 on success or a negative AFV_E* code; never throws, never
 * terminates the process.  One afv_ctx owns one HIP stream and its scratch buffers: use one context per
 * calling thread (Tracking / LocalMapping / LoopClosing each call matchers concurrently in the reference,
 * FeatureMatcher.cc §3.2) — a context is NOT re-entrant, different contexts are independent.
 *
 * Reference interfaces replaced (file:line under the reference tree):
 *   afv_orb_extract*            FeatureExtractor::operator() 6/3-arg (src/FeatureExtractor.cpp:111-129) ->
 *                               FeatureExtractor_orb32::detectAndCompute (src/Feature_orb32.cpp:11-18):
 *                               detectKeypoints(:26-40, cv::ORB::detect) + filterKeypoints(:63-65 ->
 *                               DistributeOctTree src/ORBextractor.cc:239-458) + computeDescriptors(:42-53,
 *                               cv::ORB::compute per level) + mergeKeypointLevels (FeatureExtractor.cpp:296-308)
 *   afv_orb_size_sigma          computeSize / computeSigma (src/FeatureExtractor.cpp:132-172)
 *   afv_match_bow*              FeatureMatcher::SearchByBoW(KF,KF) (src/FeatureMatcher.cc:561-660) and
 *                               SearchByBoW(KF,Frame) (:186-283), incl. the rotation histogram (:1579-1668);
 *                               with no node segments = the brute-force form (north_star "Hamming brute force")
 *   afv_match_triangulation*    FeatureMatcher::SearchForTriangulation (:662-790) + CheckDistEpipolarLine (:165-182)
 *   afv_match_l2                DescriptorDistance_sift128 (src/Feature_sift128.cpp:132-134) inside the
 *                               SearchByBoW(KF,KF) control flow (config #3)
 *   afv_hamming256              DescriptorDistance_orb32 (src/Feature_orb32.cpp:67-84)
 *   afv_points_*, afv_frame_search_points / _fuse_points / _project_points
 *                               Frame::isInFrustum (src/Frame.cc:276-331) and the projection loops of SearchByProjection(cur, last)
 *                               (src/FeatureMatcher.cc:1312-1351), the relocalisation search (:1425-1465) and Fuse (:811-858) over
 *                               device-resident map points: four rule sets and one deviation (D1), listed at "resident map points"
 */
#ifndef AFV_HIP_H
#define AFV_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AFV_MAX_LEVELS 8
#define AFV_DESC_BYTES 32

enum {
    AFV_OK = 0,
    AFV_EINVAL = -1,     /* bad argument (null pointer, size out of range for the context) */
    AFV_ENODEV = -2,     /* no usable HIP device / device ordinal out of range */
    AFV_ENOMEM = -3,     /* device or host allocation failed */
    AFV_EHIP = -4,       /* a HIP runtime call or kernel failed; see afv_last_error() */
    AFV_ECAPACITY = -5,  /* caller-provided output capacity too small; outputs truncated */
    AFV_EUNSUPPORTED = -6,
    AFV_ETIMEOUT = -7    /* a device-side wait gave up (a level pipeline stalled for ~1 s: preemption, a debugger, a profiler); nothing
                            about the inputs is wrong - the call can be repeated (afv_akaze_extract does so once by itself) */
};

/* ABI revision of this header.  It goes up whenever a record, an argument list or a limit changes incompatibly; a host built against
 * another revision must not call into the library (check once: afv_abi_version() == AFV_ABI_VERSION).
 *   5  (round 5) afv_proj_job / afv_tri_job / afv_table_tri_job start with struct_size; frame grids hold at most 8192 cells (was 65536)
 *   6  (round 6) afv_orb_detect / afv_orb_compute; afv_frame_params.desc_bytes; afv_vocab_create_f32 / afv_bow_transform_f32; afv_proj_job.float_dim; grids / frames whose one-workgroup build does not fit the
 *      LDS are refused with AFV_EUNSUPPORTED at creation instead of failing at the first launch
 *      (still 6: afv_table_create_bytes, then afv_table_create_f32 were added as exports; no record changed) */
#define AFV_ABI_VERSION 6
int afv_abi_version(void);

typedef struct afv_ctx afv_ctx;

/* bit-compatible with cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id;} */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} afv_keypoint;

typedef struct {
    int32_t nfeatures;      /* quadtree budget, Tracking.cc:1515-1520 (1000 @ 640x480); 1..4000 */
    int32_t nlevels;        /* FeatureExtractor.numOctaves (settings/orb32_settings.yaml:6); 1..8 */
    float scale_factor;     /* FeatureExtractor.scaleFactor (:7) */
    int32_t fast_threshold; /* int(FeatureExtractor.detectionTh) (:8, Feature_orb32.cpp:30) */
    int32_t max_width;      /* largest frame the context must accept (<= 4096) */
    int32_t max_height;
    int32_t max_batch;      /* frames per afv_orb_extract_batch* call */
} afv_orb_params;

void afv_default_orb_params(afv_orb_params *p); /* ORB32 defaults: 1000, 8, 1.2f, 20, 640x480, batch 1 */

int afv_create(int device_ordinal, const afv_orb_params *params, afv_ctx **out);
void afv_destroy(afv_ctx *ctx);
const char *afv_strerror(int code);
const char *afv_last_error(const afv_ctx *ctx); /* text of the last failing HIP call, "" if none */
int afv_max_keypoints_per_frame(const afv_ctx *ctx); /* sum over levels of max(quota_l + 2, 4 * nIni): safe `cap` */
void *afv_stream(afv_ctx *ctx); /* the context's hipStream_t (for callers that enqueue their own copies) */

/* ---- extraction: host-buffer plugin path (one frame; synchronous) ---- */
int afv_orb_extract(afv_ctx *ctx, const uint8_t *gray, int width, int height, int stride_bytes,
                    afv_keypoint *kps, uint8_t *desc32, int cap, int *n_out);

/* ---- the two halves of the plugin call on their own (FeatureExtractor::detectKeypoints / computeDescriptors, include/FeatureExtractor.h:123-124,
 * src/Feature_orb32.cpp:26-53): a host that calls the virtuals separately - a vocabulary builder that keeps keypoints and recomputes
 * descriptors at them - binds to these.  afv_orb_detect followed by afv_orb_compute on its keypoints gives afv_orb_extract's outputs bit for bit.
 *   afv_orb_detect   detectKeypoints + filterKeypoints: cv::ORB::detect (FAST + NMS, retainBest x 2, Harris response, IC angle, pt scaled to
 *                    level 0; Feature_orb32.cpp:26-40) and DistributeOctTree per level (:63-65, FeatureExtractor.cpp:276-284), merged in
 *                    ascending level order: keypoints with angle and response, no descriptors.
 *   afv_orb_compute  computeDescriptors: cv::ORB::compute (:42-53) for n caller-given keypoints - each described in its own octave at
 *                    cvRound(pt / scale) with its own angle, on the pyramid rebuilt from `gray` (cv::ORB::compute rebuilds levels 0 .. max
 *                    octave of its keypoints).  desc32[n][32] in the order of kps.  A keypoint is accepted when its octave is a level of
 *                    the context and its rounded centre (cx, cy) = cvRound(pt / scale) lies in 0 <= cx <= w, 0 <= cy <= h of that level: one
 *                    column / row past the last pixel is still described, as by the CPU baseline.  Any
 *                    other keypoint (NaN coordinates included): AFV_EINVAL, nothing is written. */
int afv_orb_detect(afv_ctx *ctx, const uint8_t *gray, int width, int height, int stride_bytes, afv_keypoint *kps, int cap, int *n_out);
int afv_orb_compute(afv_ctx *ctx, const uint8_t *gray, int width, int height, int stride_bytes, const afv_keypoint *kps, int n,
                    uint8_t *desc32);

/* ---- extraction: host-buffer batch (vocabulary builder shape, createVocabulary.cpp:161-174).  frames[f] = row-major gray image
 * with stride_bytes between rows; outputs kps[nframes][cap_per_frame], desc32[nframes][cap_per_frame][32], n_out[nframes].
 * Batches of at least two pipeline chunks are software-pipelined (upload of the next chunks / compute / download of the
 * finished chunk overlap).  Page-locked caller buffers (hipHostMalloc, hipHostRegister) are DMA'd in place: the whole rows
 * kps[f][0..cap) / desc32[f][0..cap) are then overwritten and entries beyond n_out[f] are unspecified.  All or nothing: the frames
 * count as page-locked only if the first and last frame of every chunk are (mixing pinned and pageable frames inside a chunk is not
 * supported), the outputs only if both arrays are page-locked end to end.  Pageable buffers are staged through the context's pinned
 * arena — correct, but about 3x slower over PCIe.  On any error no transfer is left in flight. ---- */
int afv_orb_extract_batch(afv_ctx *ctx, const uint8_t *const *frames, int nframes, int width, int height,
                          int stride_bytes, afv_keypoint *kps, uint8_t *desc32, int cap_per_frame, int *n_out);

/* ---- extraction: device-resident batch (benchmark / pipelines).  All pointers are DEVICE pointers;
 * frames are [nframes][height][stride_bytes] with frame_stride_bytes between frames (4-byte aligned base and
 * strides); outputs kps[nframes][cap_per_frame], desc32[nframes][cap_per_frame][32], n_out[nframes].
 * Enqueued on `stream` (hipStream_t); asynchronous — the caller synchronises.  STREAM RULE (all *_device entry points):
 * NULL selects the context's own non-blocking stream (afv_stream), which is NOT ordered with any stream of the caller —
 * not even HIP's null stream: either pass one of your own (non-null) streams, or order afv_stream(ctx) with events
 * (hipEventRecord + hipStreamWaitEvent both ways) or synchronise it.  The Python mirror does the event bridging when torch's
 * current stream is the default stream (_lib.launch_ordered).
 * status_out (device int32, may be NULL) receives 0 or AFV_ECAPACITY. ---- */
int afv_orb_extract_batch_device(afv_ctx *ctx, const uint8_t *d_frames, int nframes, int width, int height,
                                 int stride_bytes, size_t frame_stride_bytes, afv_keypoint *d_kps,
                                 uint8_t *d_desc32, int cap_per_frame, int32_t *d_n_out, int32_t *d_status_out,
                                 void *stream);

/* E12: size_i = normalised powf(scale, octave); sigma2_i = size^2; inf_i = 1/size^2 (host arithmetic) */
int afv_orb_size_sigma(const afv_ctx *ctx, const afv_keypoint *kps, int n, float *size, float *sigma2, float *inf);

/* ---- matching ---- */
enum { AFV_MATCH_KF_KF = 0, AFV_MATCH_KF_FRAME = 1,
       /* OR-ed into afv_match_job.mode (round 6): the descriptors are FLOAT rows - desc1 / desc2 point to n x (desc_bytes / 4) floats,
          desc_bytes = 4 * dim (a multiple of 16, <= 4096) - and the distance is cv::norm(a, b, NORM_L2SQR) narrowed to float, what
          FeatureMatcher::DescriptorDistance returns for SIFT128 / SURF64 / KAZE64 / R2D2 (FeatureMatcher.cc:1508-1531,
          Feature_sift128.cpp:132-134), evaluated like afv_match_l2.  afv_match_bow and afv_match_triangulation (bow.mode) take it;
          th_low / nnratio apply to the float distances as they stand. */
       AFV_MATCH_FLOAT32 = 0x100 };

typedef struct {
    const uint8_t *desc1; int32_t n1;   /* side 1 (KF1 / KF), n1 x desc_bytes, row-major */
    const uint8_t *desc2; int32_t n2;   /* side 2 (KF2 / Frame) */
    int32_t desc_bytes;                 /* 32 for ORB; any multiple of 4 up to 64 (AKAZE61 rows padded to 64 with zeros) */
    /* DBoW2::FeatureVector of each side as CSR over ascending node ids; nnodes == 0 on either side => brute
       force: a single node holding 0..n-1 on both sides */
    const int32_t *node_id1; const int32_t *seg_ptr1; const int32_t *seg_idx1; int32_t nnodes1;
    const int32_t *node_id2; const int32_t *seg_ptr2; const int32_t *seg_idx2; int32_t nnodes2;
    const uint8_t *valid1; const uint8_t *valid2; /* map point exists && !isBad(); NULL => all valid.
                                                     KF_FRAME ignores valid2 (FeatureMatcher.cc:216-232) */
    const float *angle1; const float *angle2;     /* keypoint angles in degrees; required iff check_orientation */
    float th_low;                       /* FeatureMatcher::TH_LOW (matchingTh, 75 for ORB) */
    float nnratio;                      /* mfNNratio */
    int32_t check_orientation;          /* mbCheckOrientation */
    int32_t mode;                       /* AFV_MATCH_KF_KF: out[n1] = idx2|-1, accept best < th_low;
                                           AFV_MATCH_KF_FRAME: out[n2] = idx1|-1, accept best <= th_low */
} afv_match_job;

/* host pointers; jobs are staged, matched on the GPU and copied back.  out = concatenation over jobs of
   int32[n1] (KF_KF) or int32[n2] (KF_FRAME); nmatches[njobs]. */
int afv_match_bow(afv_ctx *ctx, const afv_match_job *jobs, int njobs, int32_t *out, int32_t *nmatches);

/* JOB RECORDS THAT CARRY struct_size (afv_tri_job, afv_proj_job, afv_table_tri_job): set the FIRST field to sizeof(the struct you were
 * compiled against) in every job of the array.  The runtime uses it as the array stride and reads only the fields it covers; fields
 * beyond it are taken as zero (= the monocular call).  A value below the record's first published layout, above 4 x the current one,
 * or different between the jobs of one call is AFV_EINVAL - so a caller that forgot to fill it (0, stack garbage) is rejected instead of
 * having uninitialised tail pointers dereferenced.  Records grow only at the end. */
typedef struct {
    uint32_t struct_size;            /* sizeof(afv_tri_job) */
    afv_match_job bow;               /* valid1/valid2 mean "already HAS a map point" => skipped; nnratio / check_orientation and
                                        mode (but for its AFV_MATCH_FLOAT32 bit) ignored */
    const float *x1, *y1, *x2, *y2; /* mvKeysUn */
    const float *sigma2_2;           /* KeyFrame::GetKeyPt1DSigma2 of side 2 */
    float F12[9];                    /* row-major fundamental matrix */
    float ex, ey;                    /* epipole of camera 1 in image 2 */
    /* stereo keyframes (FeatureMatcher.cc:705-709, :727-731, :741): KeyFrame::mvuRight of either side (>= 0: the keypoint has a
       right-image match); NULL = monocular.  only_stereo = bOnlyStereo: features without a right match are skipped on both sides;
       the epipole-distance test (:741-748) only applies when NEITHER feature is stereo.  A zero-initialised tail = the mono call. */
    const float *u_right1, *u_right2;
    int32_t only_stereo;
} afv_tri_job;
int afv_match_triangulation(afv_ctx *ctx, const afv_tri_job *jobs, int njobs, int32_t *match12, int32_t *nmatches);

/* device-resident brute-force batch: pair p matches descriptor set a[p] (side 1) against set b[p] (side 2) of a
   table d_desc[nsets][cap][32] with per-set counts d_n[nsets] and angles d_kps (afv_keypoint, may be NULL when
   !check_orientation).  d_match[npairs][cap] (idx2 | -1), d_nmatches[npairs].  SearchByBoW(KF,KF) semantics. */
/* (d_nmatches[p] == -0x7fffffff marks a pair whose ordered phase gave up at its pass guard - never observed; the host-result entry
   points turn it into AFV_EHIP.  At most ONE call that uses the column-sliced phase 1 (calls of at most afv_set_small_batch_path's
   max_frames pairs) may be in flight per context: its tickets and slice records are per context, not per stream.) */
int afv_match_bruteforce_pairs_device(afv_ctx *ctx, const uint8_t *d_desc, const afv_keypoint *d_kps,
                                      const int32_t *d_n, int nsets, int cap, const int32_t *d_pair_a,
                                      const int32_t *d_pair_b, int npairs, float th_low, float nnratio,
                                      int check_orientation, int32_t *d_match, int32_t *d_nmatches, void *stream);

/* ---- keyframe descriptor table resident in HBM + multi-GPU replication (BASELINE.json configs[3]) ----
 * The reference matches a query keyframe against every loop / relocalisation candidate, one SearchByBoW call per
 * candidate (LoopClosing::ComputeSim3 src/LoopClosing.cc:255-281 over the candidates of KeyFrameDatabase::
 * DetectLoopCandidates src/KeyFrameDatabase.cc:76-197; Tracking::Relocalization src/Tracking.cc:1162-1182).  Here the
 * keyframes' descriptors (KeyFrame::mDescriptors, const after construction, include/KeyFrame.h:190), keypoint angles
 * (mvKeysUn[i].angle) and optionally their DBoW2::FeatureVector (mFeatVec, KeyFrame.h:194) live in ONE device table
 * of `nsets` slots x `cap` features; batches of (slot a, slot b) pair jobs are matched without any descriptor leaving
 * HBM.  With several GPUs (one process per GPU) the table is built on one rank and replicated with ONE RCCL broadcast
 * per array over xGMI (afv_table_broadcast); every rank then matches its own share of the jobs against its replica.
 * A table belongs to the context it was created on and is destroyed before it. */
typedef struct afv_table afv_table;
/* a table of 32-byte binary rows (ORB32) */
int afv_table_create(afv_ctx *ctx, int nsets, int cap /* <= 4096 */, afv_table **out);
/* a table of binary rows of desc_bytes = 1 .. 64 bytes (61 AKAZE, 48 BRISK, 64 FREAK ...), stored zero-padded to a pitch of 32 bytes
 * (desc_bytes <= 32) or 64 bytes (33 .. 64), the rule of resident frames.  Every afv_table_* entry point works at that width with the
 * reference's rules unchanged; a frame meets the table only when it is binary with the same desc_bytes (else AFV_EUNSUPPORTED).
 * afv_table_create(ctx, nsets, cap, out) is afv_table_create_bytes(ctx, nsets, cap, 32, out). */
int afv_table_create_bytes(afv_ctx *ctx, int nsets, int cap /* <= 4096 */, int desc_bytes, afv_table **out);
/* a table of FLOAT rows (SIFT128, SURF64, KAZE64, R2D2-128 ...): float_dim floats per row, a multiple of 4 from 4 to 1024 (the rule of
 * afv_frame_params.float_dim; anything else is AFV_EINVAL), pitch 4 * float_dim bytes, no padding.  Every afv_table_* entry point works on
 * it with the conventions of a float frame: afv_table_set takes n x float_dim floats behind its uint8_t pointer, afv_frame_view.desc32 of
 * afv_table_match_bow_frame points to n x float_dim floats, afv_table_device_ptrs gives d_desc[nsets][cap][float_dim] floats.  The
 * distance is L2^2 as cv::norm(a, b, NORM_L2SQR) evaluates it (Feature_sift128.cpp:132-134); th_low / nnratio apply to it as it stands.
 * A frame meets the table only when it is a float frame of the same float_dim; a binary frame against a float table, a float frame
 * against a binary table or a float table of another float_dim, and afv_table_clone / afv_table_broadcast between tables of different
 * kind or float_dim answer AFV_EUNSUPPORTED before any data moves. */
int afv_table_create_f32(afv_ctx *ctx, int nsets, int cap /* <= 4096 */, int float_dim, afv_table **out);
void afv_table_destroy(afv_table *t);
/* upload keyframe `set`: n x desc_bytes descriptors (packed; 32 for afv_table_create; a float table: n x float_dim floats), angles[n] in
 * degrees (NULL = zeros).
 * The library writes the rows' padding (zero).  Host pointers; synchronous. */
int afv_table_set(afv_table *t, int set, const uint8_t *desc32, const float *angles, int n);
/* the keyframe's FeatureVector as CSR over ascending node ids (as in afv_match_job); needed by afv_table_match_bow only.
 * The node ids / segment sizes stay on the host too (the merge-join of two FeatureVectors, FeatureMatcher.cc:205-276,
 * is host work: <= a few hundred ints per pair), the feature indices go to the device. */
int afv_table_set_featvec(afv_table *t, int set, const int32_t *node_id, const int32_t *seg_ptr, const int32_t *seg_idx,
                          int nnodes);
/* per-feature validity of keyframe `set` for afv_table_match_bow: valid[i] = map point exists && !isBad() (FeatureMatcher.cc:593-597,
 * :609-613; it changes as the map evolves, so the host re-uploads the n bytes when it does).  NULL = every feature valid (the
 * default).  The brute-force pair entry points take every feature as valid. */
int afv_table_set_valid(afv_table *t, int set, const uint8_t *valid);
/* device views for zero-copy callers: d_desc[nsets][cap][pitch] (pitch 32 or 64 bytes, see afv_table_create_bytes; a writer keeps the
 * padding zero; a float table: [nsets][cap][float_dim] floats), d_angle[nsets][cap] (float), d_n[nsets] (int32) */
int afv_table_device_ptrs(afv_table *t, uint8_t **d_desc, float **d_angle, int32_t **d_n);
/* brute-force SearchByBoW(KF,KF) (FeatureMatcher.cc:561-660 with one node holding everything) of npairs (a, b) slot
 * pairs.  pair arrays are HOST int32; outputs are HOST arrays: match12[npairs][cap] (may be NULL: counts only) and
 * nmatches[npairs].  The descriptors never leave the device; only the pair list goes in and the results come out. */
int afv_table_match_pairs(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, int npairs, float th_low, float nnratio,
                          int check_orientation, int32_t *match12, int32_t *nmatches);
/* same, fully device-resident and asynchronous on `stream` (see afv_orb_extract_batch_device for the stream rule):
 * d_pair_a / d_pair_b / d_match12[npairs][cap] / d_nmatches[npairs] are DEVICE pointers */
int afv_table_match_pairs_device(afv_table *t, const int32_t *d_pair_a, const int32_t *d_pair_b, int npairs, float th_low,
                                 float nnratio, int check_orientation, int32_t *d_match12, int32_t *d_nmatches, void *stream);
/* BoW-guided SearchByBoW(KF,KF) (FeatureMatcher.cc:561-660: merge-join of the two FeatureVectors, per shared node the
 * ordered greedy scan) of npairs slot pairs whose FeatureVectors were stored with afv_table_set_featvec.  Host pair
 * arrays in, host results out (match12 may be NULL); descriptors and feature indices stay in HBM. */
int afv_table_match_bow(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, int npairs, float th_low, float nnratio,
                        int check_orientation, int32_t *match12, int32_t *nmatches);
/* Relocalisation batch: SearchByBoW(KF, Frame) (FeatureMatcher.cc:186-283) of ONE frame against `nslots` candidate keyframes of the
 * table - what Tracking::Relocalization does in a loop over the candidates of DetectRelocalizationCandidates (src/Tracking.cc:1162,
 * 1182).  The frame is uploaded once (descriptors, angles, the feature indices of its FeatureVector); every candidate is one job of the
 * same launch pair.  Rules of the reference: validity (afv_table_set_valid) on the keyframe side only (:216-222), a frame feature that
 * already holds a match is skipped (:232), accept best <= th_low (:250), rotation histogram keyed by the frame feature (:259).
 * Host pointers.  match_f[nslots][frame->n] = index of the matched keyframe feature per FRAME feature or -1 (may be NULL: counts
 * only); nmatches[nslots]. */
typedef struct {
    const uint8_t *desc32; int32_t n;   /* the frame's n x desc_bytes descriptors (Frame::mDescriptors), packed at the table's width */
    const float *angle;                 /* mvKeysUn[i].angle in degrees; required iff check_orientation */
    /* Frame::mFeatVec as CSR over ascending node ids (as in afv_match_job); nnodes == 0: the frame shares no node with anybody */
    const int32_t *node_id; const int32_t *seg_ptr; const int32_t *seg_idx; int32_t nnodes;
} afv_frame_view;
int afv_table_match_bow_frame(afv_table *t, const int32_t *slots, int nslots, const afv_frame_view *frame, float th_low, float nnratio,
                              int check_orientation, int32_t *match_f, int32_t *nmatches);
/* SearchForTriangulation (FeatureMatcher.cc:662-790, stereo branches included: afv_table_set_u_right) of npairs slot pairs
 * over the stored FeatureVectors and the per-keyframe geometry stored with afv_table_set_geometry (mvKeysUn[i].pt and KeyFrame::GetKeyPt1DSigma2(i)): what
 * LocalMapping::CreateNewMapPoints does against <= 20 neighbours (src/LocalMapping.cc:238-297).  Per pair only the
 * fundamental matrix, the epipole and the "already has a map point" masks travel. */
int afv_table_set_geometry(afv_table *t, int set, const float *x, const float *y, const float *sigma2);
/* KeyFrame::mvuRight of a stereo keyframe (>= 0: the keypoint has a right-image match; FeatureMatcher.cc:705, :727), after
 * afv_table_set_geometry of the same slot, which marks every feature monocular (-1). */
int afv_table_set_u_right(afv_table *t, int set, const float *u_right);
/* afv_table_set (a recycled slot) forgets the slot's FeatureVector, geometry and validity mask: afv_table_match_bow /
 * afv_table_match_triangulation return AFV_EINVAL for a slot that holds features but lacks what the call needs, instead of
 * answering "no matches". */
typedef struct {
    uint32_t struct_size;    /* sizeof(afv_table_tri_job) (see afv_tri_job) */
    float F12[9];            /* row-major fundamental matrix (as afv_tri_job) */
    float ex, ey;            /* epipole of camera a in image b */
    const uint8_t *has_mp1;  /* [n_a] feature already has a map point => skipped (NULL = none has) */
    const uint8_t *has_mp2;  /* [n_b] */
    float th_low;            /* FeatureMatcher::TH_LOW */
    int32_t only_stereo;     /* bOnlyStereo (FeatureMatcher.cc:707-709, :729-731); 0 for monocular maps */
} afv_table_tri_job;
int afv_table_match_triangulation(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, const afv_table_tri_job *geo, int npairs,
                                  int32_t *match12 /*[npairs][cap]: idx_b | -1*/, int32_t *nmatches);
/* refresh the host copy of the per-slot counts after the caller wrote d_n on the device itself */
int afv_table_sync_counts(afv_table *t);

/* RCCL communicator (one process per GPU).  No RCCL symbol is linked: the library is looked up at run time
 * (an RCCL already loaded into the process, e.g. by PyTorch, is reused; otherwise librccl.so.1 is opened). */
typedef struct afv_comm afv_comm;
#define AFV_COMM_ID_BYTES 128
/* rank 0 creates the id and hands it to the other ranks through any host channel (file, socket, MPI, torch store) */
int afv_comm_unique_id(uint8_t id[AFV_COMM_ID_BYTES]);
int afv_comm_create(afv_ctx *ctx, const uint8_t id[AFV_COMM_ID_BYTES], int nranks, int rank, afv_comm **out);
void afv_comm_destroy(afv_comm *comm);
int afv_comm_rank(const afv_comm *comm);
int afv_comm_size(const afv_comm *comm);
/* in-place broadcast of `bytes` at device pointer `d_buf` from rank `root` (ncclBroadcast, uint8), asynchronous on
 * `stream` (NULL = the context's stream) */
int afv_comm_broadcast(afv_comm *comm, void *d_buf, size_t bytes, int root, void *stream);
/* every rank contributes bytes_per_rank at d_send; d_recv receives nranks * bytes_per_rank in rank order */
int afv_comm_allgather(afv_comm *comm, const void *d_send, void *d_recv, size_t bytes_per_rank, void *stream);
/* replicate the WHOLE table from `root`: descriptors, angles, counts, and — when the root holds them — FeatureVectors (the
 * feature-index plane plus the host-side node structure), geometry and validity planes: one broadcast per array and one for the
 * "replica image" (node ids / CSR pointers / per-set flags), then a stream synchronisation.  After the call every rank answers
 * afv_table_match_pairs, afv_table_match_bow and afv_table_match_triangulation exactly as the root does; whatever a receiver held
 * before is replaced.  elapsed_ms (may be NULL) = device time of the broadcasts (hipEvents on the context's stream). */
int afv_table_broadcast(afv_comm *comm, afv_table *t, int root, float *elapsed_ms);
/* copy everything `src` holds into `dst` (same nsets / cap; may live on another context or device) through the same replica image
 * and rebuild step the receivers of afv_table_broadcast run — a replica without a communicator (e.g. one table per calling thread) */
int afv_table_clone(const afv_table *src, afv_table *dst);
/* block partition of n_units over the ranks: unit u belongs to the rank whose [lo, hi) holds it */
void afv_shard_range(long n_units, int rank, int nranks, long *lo, long *hi);

/* float descriptors, L2^2 distance (config #3): brute force with SearchByBoW(KF,KF) control flow */
int afv_match_l2(afv_ctx *ctx, const float *desc1, int n1, const float *desc2, int n2, int dim,
                 const uint8_t *valid1, const uint8_t *valid2, float th_low, float nnratio, int32_t *match12,
                 int32_t *nmatches);
/* the same matcher over a device-resident table of float descriptors, many (set a, set b) pair jobs per call (the float counterpart of
 * afv_match_bruteforce_pairs_device): d_desc[(set * cap + row) * dim], d_n[set] rows per set, dim 64 or 128; d_match[pair * cap + row] =
 * index into set b or -1 (rows past the set's count: -1), d_nmatches[pair].  Asynchronous on `stream` (NULL: the context's stream). */
int afv_match_l2_pairs_device(afv_ctx *ctx, const float *d_desc, const int32_t *d_n, int cap, int dim, const int32_t *d_pair_a,
                              const int32_t *d_pair_b, int npairs, float th_low, float nnratio, int32_t *d_match, int32_t *d_nmatches,
                              void *stream);

/* ---- projection-guided matching core (grid window + Hamming) ----
 * Matching loops of FeatureMatcher::SearchByProjection(F, localMapPoints) (src/FeatureMatcher.cc:73-154, mode
 * AFV_PROJ_LOCALMAP) and SearchByProjection(CurrentFrame, LastFrame) (:1291-1402, AFV_PROJ_LASTFRAME, mono) incl.
 * Frame::GetFeaturesInArea (src/Frame.cc:333-382) over the grid of AssignFeaturesToGrid (Frame.cc:225-240).  The caller
 * evaluates the projection as the reference does and passes, per query in the reference's iteration order:
 * (u, v) = projected position, r = window radius (:91 / :1343), [min_size, max_size] = admissible keyPtsSize band. */
enum { AFV_PROJ_LOCALMAP = 0, AFV_PROJ_LASTFRAME = 1 };
typedef struct {
    uint32_t struct_size;                               /* sizeof(afv_proj_job) (see afv_tri_job) */
    const uint8_t *desc; int32_t n; int32_t desc_bytes; /* frame features F.mDescriptors (n <= 8192) */
    const float *x; const float *y;                     /* F.mvKeysUn[i].pt */
    const float *size;                                  /* F.keyPtsSize[i] */
    const float *angle;                                 /* F.mvKeysUn[i].angle (LASTFRAME + check_orientation) */
    const uint8_t *occupied;                            /* F.pts[i] && F.pts[i]->NumberOfObservations() > 0; NULL = none */
    const float *inf;                                   /* KeyFrame::GetKeyPt1DInf(i): afv_match_fuse only */
    float min_x, min_y, grid_inv_w, grid_inv_h;         /* mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv */
    int32_t grid_cols, grid_rows;                       /* FRAME_GRID_COLS 64, FRAME_GRID_ROWS 48 (Frame.h:40-41); cols * rows <= 8192 */
    int32_t nq;                                         /* queries: map points / last-frame keypoints */
    const uint8_t *qdesc; const uint8_t *qvalid;        /* pMP->GetDescriptor(); pMP && in view && !isBad (NULL = all) */
    const float *qu; const float *qv; const float *qr; const float *qmin_size; const float *qmax_size;
    const float *qangle;                                /* LastFrame.mvKeysUn[i].angle (LASTFRAME + check_orientation) */
    const uint8_t *qoccupies;                           /* pMP->NumberOfObservations() > 0 (NULL = yes) */
    float th_high, nnratio, size_tol, inv_size_tol;     /* TH_HIGH, mfNNratio, F.sizeTolerance, F.invSizeTolerance */
    int32_t check_orientation, mode;
    /* stereo frames / keyframes (NULL u_right = monocular; a zero-initialised tail = the mono call):
       u_right[i] = mvuRight of feature i; q_ur[q] = the query's projected right-image coordinate (pMP->mTrackProjXR :116,
       u - mbf * invzc :1369, ur of Fuse :885); q_er_max[q] = the gate of afv_match_projection (r * pMP->trackSigma :117 in
       AFV_PROJ_LOCALMAP, the window radius :1371 in AFV_PROJ_LASTFRAME).
       afv_match_projection skips a feature with u_right > 0 whose |q_ur - u_right| exceeds q_er_max (:114-119, :1367-1372);
       afv_match_fuse replaces the 2-dof gate e2 * inf <= 5.99 by the 3-dof one (ex^2 + ey^2 + er^2) * inf <= 7.8 for features with
       u_right >= 0 (:880-894).  afv_match_sim3 / afv_match_initialization have no stereo branch and ignore the three fields. */
    const float *u_right; const float *q_ur; const float *q_er_max;
    /* (ABI 6, appended: struct_size tells) float descriptors.  FeatureMatcher::DescriptorDistance dispatches on DescriptorType (FeatureMatcher.cc:1508-1531) and returns
       Descriptor_Distance_Type = float (Types.h:127): for SIFT128 / SURF64 / KAZE64 / R2D2 / any non-binary feature it is
       cv::norm(a, b, NORM_L2SQR) (Feature_sift128.cpp:132-134).  float_dim > 0: desc and qdesc point to rows of float_dim floats
       (a multiple of 4, <= 1024; desc_bytes is ignored), distances are evaluated like afv_match_l2 (float differences, squares and 4-way
       partial sums in double, narrowed once), th_high / nnratio apply to them as they stand; 0 (what a caller compiled against an older
       header gets) = binary rows of desc_bytes.  All four searches below accept it; afv_match_projection runs float jobs on either engine of
       its ordered phase (afv_set_projection_resolve), afv_match_initialization always on the ordered walk (its fixed point packs
       distances in 16 bits). */
    int32_t float_dim;
} afv_proj_job;
/* Job batches (njobs > 1; afv_match_projection, afv_match_fuse and afv_match_initialization alike; tests/test_gpu_proj_scenes.py):
 *   - every job is answered as if it had been sent alone: the jobs share nothing but the call;
 *   - the outputs follow each other in job order without padding: job k's slice starts at the sum of the earlier jobs' lengths, where a
 *     job's length is n (feature-indexed) for afv_match_projection and nq (query-indexed) for afv_match_fuse / _initialization;
 *     nmatches / nfound has one entry per job.  A job with n == 0 or nq == 0 is legal anywhere in the array (an empty slice / a slice
 *     of -1, count 0);
 *   - the jobs of one call may differ in everything: n, nq, the grid, the mode, check_orientation, occupancy masks, stereo fields,
 *     the width of binary rows (1 .. 64 bytes) and binary next to float rows (float_dim).  The engine of the ordered phase is chosen
 *     per CALL: the fixed point runs when the tables of the call's largest job fit the LDS of one workgroup, else every job of the
 *     call takes the ordered walk; one float job in an afv_match_initialization call sends the whole call to the ordered walk.  The
 *     answers do not depend on the engine;
 *   - limits, per job: n <= 8192, nq <= 65535, grid_cols * grid_rows <= 8192, desc_bytes <= 64, float_dim a multiple of 4 <= 1024.
 *     One job outside them refuses the whole call with AFV_EINVAL before anything is launched or written.
 * assign = concatenation over jobs of int32[n]: index of the query assigned to feature i (F.pts[i] = pMP) or -1 */
int afv_match_projection(afv_ctx *ctx, const afv_proj_job *jobs, int njobs, int32_t *assign, int32_t *nmatches);
/* matching core of FeatureMatcher::Fuse(pKF, vpMapPoints, th) (src/FeatureMatcher.cc:794-940) over
 * KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:613-652): per map point the most similar keypoint of the window that lies in
 * the size band [qmin_size, qmax_size] (= predictedSize / sizeTolerance .. * sizeTolerance, :871-873) and passes the
 * reprojection gate e2 * inf <= 5.99 (:897); th_high carries TH_LOW (:915).  Map points are independent here; the map surgery
 * (:918-936) stays with the caller.  best = concatenation over jobs of int32[nq] (feature index or -1); nfound[njobs]. */
int afv_match_fuse(afv_ctx *ctx, const afv_proj_job *jobs, int njobs, int32_t *best, int32_t *nfound);
/* inf == NULL in a job drops the reprojection gate: that is the matching core of Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
 * (src/FeatureMatcher.cc:942-1064).  The remaining SearchByProjection flavours need no extra entry point:
 *   - SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:287-397): afv_match_projection, mode AFV_PROJ_LASTFRAME,
 *     check_orientation 0, occupied = vpMatched[i] != NULL, qmin/qmax = predictedSize / , * sizeTolerance, th_high = TH_LOW;
 *   - SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, useHigh) (:1404-1506, relocalisation): the same mode with
 *     check_orientation = mbCheckOrientation, qangle = pKF->mvKeysUn[i].angle, occupied = CurrentFrame.pts[i] != NULL,
 *     th_high = descDistTh_{low,high}_reloc. */

/* SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/FeatureMatcher.cc:1066-1287): j12 = map points of KF1
 * (query q = KF1 feature index; q_valid = has a good, not already matched map point that projects into KF2) searched among
 * KF2's features, j21 the reverse; both are gate-less best-only searches with th_high = TH_HIGH (:1171, :1254); the
 * agreement check (:1268-1284) runs here too.  Requires j12->nq == j21->n and j21->nq == j12->n.
 * match12[j12->nq] = KF2 feature index or -1. */
int afv_match_sim3(afv_ctx *ctx, const afv_proj_job *j12, const afv_proj_job *j21, int32_t *match12, int32_t *nfound);

/* SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/FeatureMatcher.cc:399-557; active code
 * :480-556): queries = F1's features (q_valid = octave 0, q_u/q_v = vbPrevMatched, q_radius = windowSize,
 * q_size_min = 0, q_size_max = F1.maxKeyPtSize, q_angle = F1 keypoint angle), features = F2 with its grid, th_high = TH_LOW,
 * nnratio, check_orientation.  Ordered: a feature already matched at a distance <= the current one is skipped (:513) and a
 * later query steals it otherwise (:531-535).  match12 = concatenation over jobs of int32[nq]; the caller refreshes
 * vbPrevMatched (:551-553). */
int afv_match_initialization(afv_ctx *ctx, const afv_proj_job *jobs, int njobs, int32_t *match12, int32_t *nmatches);

/* ---- BoW quantisation ----
 * DBoW2 TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) as called by Vocabulary::transform
 * (src/Vocabulary.cpp:156-206, levelsup = 4; Frame::ComputeBoW src/Frame.cc:397-401, KeyFrame::ComputeBoW
 * src/KeyFrame.cc:65-73).  The tree is uploaded once; per descriptor the kernel descends it (k-way Hamming argmin per level,
 * first minimum wins) and returns the leaf node and the node met at depth L - levelsup, from which the host builds the
 * FeatureVector (node -> ascending feature indices) that afv_match_bow consumes and the BowVector (word weights). */
typedef struct afv_vocab afv_vocab;
/* children of node i = child_idx[child_ptr[i] .. child_ptr[i+1]) in DBoW2 order; node 0 = root; desc = nnodes x desc_bytes */
int afv_vocab_create(afv_ctx *ctx, int k, int L, int nnodes, const int32_t *child_ptr, const int32_t *child_idx,
                     const uint8_t *desc, int desc_bytes, afv_vocab **out);
void afv_vocab_destroy(afv_ctx *ctx, afv_vocab *v);
int afv_bow_transform(afv_ctx *ctx, const afv_vocab *v, const uint8_t *desc, int n, int levelsup, int32_t *leaf_node,
                      int32_t *node_at_level);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:279-349) for a batch of map points - the one M1 (DescriptorDistance) call site
 * of the reference that had no device form (LocalMapping calls it per created / fused point).  Map point s observes the
 * descriptors desc[set_ptr[s] .. set_ptr[s + 1]) (rows of desc_bytes, host memory, <= 65535 per point); best_idx[s] = the row (index
 * INSIDE the set) with the least median distance to the others - the median as the reference takes it: the floor(0.5 (N - 1))-th entry
 * of the sorted row of the N x N matrix, the zero self-distance included; the first row wins ties - or -1 for an empty set;
 * best_median[s] (may be NULL) = that median.  Binary descriptors. */
int afv_distinctive_descriptors(afv_ctx *ctx, const uint8_t *desc, int desc_bytes, const int32_t *set_ptr, int nsets, int32_t *best_idx,
                                int32_t *best_median);

/* ... and for float descriptors (DescriptorDistance = cv::norm(a, b, NORM_L2SQR) as a float, like afv_match_l2): desc = rows of `dim` floats,
 * best_median (may be NULL) = the winning row's median distance. */
int afv_distinctive_descriptors_f32(afv_ctx *ctx, const float *desc, int dim, const int32_t *set_ptr, int nsets, int32_t *best_idx,
                                    float *best_median);

/* The float cases of Vocabulary::transform (src/Vocabulary.cpp:158-187: SIFT128, SURF64, KAZE64, R2D2, any non-binary feature): node
 * descriptors and features are `dim` floats (64, 128 or 256), the distance at a node is DBoW2's float-descriptor distance - squared
 * differences evaluated in float, accumulated in double in index order (upstream FSurf64::distance; the reference's fork with the classes
 * it instantiates is an empty submodule: parity unpinned) - first minimum wins.  Same tree arguments as afv_vocab_create; destroyed with
 * afv_vocab_destroy; afv_bow_transform refuses a float vocabulary and afv_bow_transform_f32 a binary one; afv_frame_bow_transform wants the
 * vocabulary of the frame's own descriptor kind and size (a float frame - afv_frame_params.float_dim - a float vocabulary of that dimension). */
int afv_vocab_create_f32(afv_ctx *ctx, int k, int L, int nnodes, const int32_t *child_ptr, const int32_t *child_idx, const float *desc, int dim,
                         afv_vocab **out);
int afv_bow_transform_f32(afv_ctx *ctx, const afv_vocab *v, const float *desc, int n, int levelsup, int32_t *leaf_node, int32_t *node_at_level);

/* words the vocabulary stops (DBoW2 transform: a word whose weight is not > 0 enters neither the BowVector nor the FeatureVector):
 * stopped[nnodes] != 0 marks them; NULL = none (the default).  Only the device-built FeatureVector of afv_frame_bow_transform reads it. */
int afv_vocab_set_stopped(afv_ctx *ctx, afv_vocab *v, const uint8_t *stopped);

/* ---- the device-resident Frame (round 5) ----
 * In the reference a Frame is built once (src/Frame.cc:171-223: ExtractFeatures :242-259 -> UndistortKeyPoints :403-433 ->
 * AssignFeaturesToGrid :225-240) and then consumed by every matcher of that tracking step: SearchByProjection(cur, last)
 * (src/Tracking.cc:747,753), SearchByProjection(F, local map points) (:1026), Frame::ComputeBoW (Frame.cc:397-401) -> SearchByBoW(KF, F)
 * (Tracking.cc:626-629), SearchForInitialization, and - if promoted - copied into a KeyFrame (src/KeyFrame.cc:36).  An afv_frame is that
 * object on the device: afv_frame_extract runs the extraction of afv_orb_extract and KEEPS keypoints and descriptors in HBM, derives
 * mvKeysUn / keyPtsSize / keyPtsSigma2 / keyPtsInf per feature and builds the 64 x 48 grid there (PosInGrid's expression, Frame.cc:384-394:
 * cell = round((x - mnMinX) * mfGridElementWidthInv), ascending feature index inside a cell); the consumers below read it in place.
 * After the image nothing of the frame is uploaded again: a projection search sends its queries, a BoW search nothing at all.
 * A frame belongs to the context it was created on (one calling thread at a time, like the context) and dies with it. */
typedef struct afv_frame afv_frame;
typedef struct {
    uint32_t struct_size;             /* sizeof(afv_frame_params) */
    float min_x, min_y, max_x, max_y; /* mnMinX, mnMinY, mnMaxX, mnMaxY (Frame::ComputeImageBounds, Frame.cc:435-466) */
    int32_t grid_cols, grid_rows;     /* FRAME_GRID_COLS 64, FRAME_GRID_ROWS 48 (Frame.h:40-41); cols * rows <= 8192 */
    int32_t distorted;                /* 0: mDistCoef[0] == 0, mvKeysUn = mvKeys (Frame.cc:405-409) and the grid is built inside
                                         afv_frame_extract; 1: the caller undistorts (cv::undistortPoints of N points is host work) and
                                         hands mvKeysUn over with afv_frame_set_undistorted, which builds the grid */
    int32_t cap;                      /* most features the frame can hold; 0 = afv_max_keypoints_per_frame(ctx); <= 8192 */
    int32_t desc_bytes;               /* (ABI 6) bytes of one binary descriptor, 1 .. 64: 32 ORB (0 = 32), 61 AKAZE, 48 BRISK ... - the reference's
                                         matchers dispatch on DescriptorType (FeatureMatcher.cc:1508-1531).  Rows live zero-padded to 8 or 16
                                         dwords in HBM.  A frame that is not 32-byte is filled with afv_frame_set_features (afv_frame_extract
                                         is the ORB32 extractor; a keyframe TABLE of the same desc_bytes (afv_table_create_bytes) takes it
                                         in afv_table_set_from_frame / afv_table_match_bow_frame_h, a table of another width answers
                                         AFV_EUNSUPPORTED) and serves afv_frame_bow_transform with a
                                         vocabulary of the same descriptor size, afv_frame_match_projection / _fuse / _initialization */
    int32_t float_dim;                /* (ABI 6, appended) > 0: the frame holds FLOAT descriptors of float_dim floats (a multiple of 4, <= 1024:
                                         SIFT128, SURF64, KAZE64, R2D2 ...; desc_bytes is ignored): afv_frame_set_features takes the rows as
                                         n x float_dim floats behind its uint8_t pointer, afv_frame_bow_transform wants a float vocabulary of
                                         that dimension (afv_vocab_create_f32), the projection searches and SearchForInitialization use
                                         L2^2 distances (afv_proj_job.float_dim; afv_proj_queries.qdesc = nq x float_dim floats,
                                         desc_bytes = 4 * float_dim).  It meets a keyframe table of float rows of the same float_dim
                                         (afv_table_create_f32) in afv_table_set_from_frame / afv_table_match_bow_frame_h / qref_table;
                                         a binary table or another float_dim answers AFV_EUNSUPPORTED */
    int32_t keep_pyramid;             /* (appended; callers of the earlier layouts read 0) 1: afv_frame_extract leaves the detector's unblurred
                                         pyramid levels of its image with the frame (device copies out of the context's pyramid buffer,
                                         behind the extraction on the context's stream) for afv_frame_stereo_match; 0: the frame of
                                         before, nothing is copied */
} afv_frame_params;
int afv_frame_create(afv_ctx *ctx, const afv_frame_params *params, afv_frame **out);
void afv_frame_destroy(afv_frame *f);
/* FeatureExtractor::operator() into the frame: host outputs exactly as afv_orb_extract (kps / desc32 / n_out; the three may all be NULL
 * when the caller wants the device copy only) and the device-resident frame described above.  Synchronous. */
int afv_frame_extract(afv_frame *f, const uint8_t *gray, int width, int height, int stride_bytes, afv_keypoint *kps, uint8_t *desc32,
                      int cap, int *n_out);
/* a frame whose features were produced elsewhere (a stereo rig, another extractor, a test): n keypoints (cv::KeyPoint layout; pt =
 * mvKeysUn unless `distorted`), n descriptor rows of the frame's kind (desc_bytes bytes each; float_dim floats each for a float frame), per-feature keyPtsSize (NULL = E12 from the octave as afv_orb_size_sigma) and
 * mvuRight (NULL = monocular: -1).  Host pointers; asynchronous on the context's stream (the arrays are copied before the call returns). */
int afv_frame_set_features(afv_frame *f, const afv_keypoint *kps, const uint8_t *desc32, int n, const float *size, const float *u_right);
/* mvKeysUn of a `distorted` frame: x[n], y[n] (host); builds the grid.  Asynchronous on the context's stream. */
int afv_frame_set_undistorted(afv_frame *f, const float *x, const float *y);
int afv_frame_count(const afv_frame *f); /* N of the last afv_frame_extract / afv_frame_set_features */
/* device views (valid until the frame is destroyed; contents change with the next extract): any may be NULL.
 * d_kps[cap] afv_keypoint (mvKeys), d_desc[cap][row] (row = 32 bytes; 64 for binary rows above 32 bytes, zero-padded; 4 * float_dim for a float frame), d_xy = {x[cap], y[cap]} of mvKeysUn, d_size[cap] keyPtsSize, d_angle[cap],
 * d_n = the count */
int afv_frame_device_ptrs(afv_frame *f, afv_keypoint **d_kps, uint8_t **d_desc, float **d_x, float **d_y, float **d_size, float **d_angle,
                          int32_t **d_n);
/* parity / debugging: the grid as CSR over cells (cell = ix * grid_rows + iy): cell_ptr[cols * rows + 1], cell_idx[n] */
int afv_frame_get_grid(afv_frame *f, int32_t *cell_ptr, int32_t *cell_idx);
/* Frame::ComputeBoW (Frame.cc:397-401): the tree descent of afv_bow_transform over the frame's own descriptors.  leaf_node[n] /
 * node_at_level[n] (host, may be NULL) feed the caller's BowVector; the FeatureVector (node -> ascending feature indices, stopped words
 * left out) is built ON THE DEVICE and stays with the frame for afv_table_match_bow_frame_h / afv_table_set_from_frame; its node
 * structure (what the merge-join of two FeatureVectors walks, FeatureMatcher.cc:205-276) is kept on the host side of the handle.
 * nnodes_out (may be NULL) = number of distinct nodes.  Synchronous. */
int afv_frame_bow_transform(afv_frame *f, const afv_vocab *v, int levelsup, int32_t *leaf_node, int32_t *node_at_level, int32_t *nnodes_out);
/* the FeatureVector of the last afv_frame_bow_transform as CSR (host copies; any may be NULL): node_id[nnodes], seg_ptr[nnodes + 1],
 * seg_idx[seg_ptr[nnodes]] */
int afv_frame_get_featvec(afv_frame *f, int32_t *node_id, int32_t *seg_ptr, int32_t *seg_idx);
/* the queries of a projection search (everything afv_proj_job carries on the query side), host pointers */
typedef struct {
    uint32_t struct_size;                               /* sizeof(afv_proj_queries) */
    int32_t nq;
    const uint8_t *qdesc; int32_t desc_bytes;           /* pMP->GetDescriptor(), nq x desc_bytes (32) */
    const uint8_t *qvalid;                              /* NULL = all */
    const float *qu; const float *qv; const float *qr; const float *qmin_size; const float *qmax_size;
    const float *qangle;                                /* AFV_PROJ_LASTFRAME / initialization with check_orientation */
    const uint8_t *qoccupies;                           /* NULL = yes */
    const float *q_ur; const float *q_er_max;           /* stereo frames only (see afv_proj_job) */
    const uint8_t *occupied;                            /* F.pts[i] && F.pts[i]->NumberOfObservations() > 0 per FRAME feature; NULL = none:
                                                           the one piece of map state the searches read from the frame side */
    float th_high, nnratio;                             /* TH_HIGH (or the threshold of the flavour), mfNNratio */
    int32_t check_orientation, mode;                    /* mode: AFV_PROJ_LOCALMAP / AFV_PROJ_LASTFRAME */
    /* the queries' descriptors by reference instead of by value: a map point's descriptor is a row of the keyframe that observed it
     * (MapPoint::ComputeDistinctDescriptors copies pKF->mDescriptors.row(idx)), so when that keyframe sits in an afv_table the row is
     * gathered on the device: qref_table + qref_slot[nq] + qref_idx[nq] (qdesc NULL).  8 bytes per query instead of desc_bytes.  The table's
     * kind and desc_bytes / float_dim must be the frame's (else AFV_EUNSUPPORTED). */
    afv_table *qref_table; const int32_t *qref_slot; const int32_t *qref_idx;
} afv_proj_queries;
/* SearchByProjection(F, vpMapPoints, th) (FeatureMatcher.cc:73-154) / SearchByProjection(CurrentFrame, LastFrame, th, mono) (:1291-1402)
 * and the flavours listed under afv_match_projection, against the frame's resident features and grid; size_tol = the frame's
 * sizeTolerance (the context's scale_factor, Frame.cc:73-74).  assign[n] (query index now in F.pts[i] | -1), *nmatches.  Synchronous. */
int afv_frame_match_projection(afv_frame *f, const afv_proj_queries *q, int32_t *assign, int32_t *nmatches);
/* matching core of Fuse(pKF, vpMapPoints, th) with the frame in the role of the keyframe (KeyFrame::GetFeaturesInArea reads the grid the
 * KeyFrame copied from its Frame, KeyFrame.cc:36,613-652): best[nq] (feature index | -1), *nfound.  use_inf_gate 0 = the Sim3 flavour. */
int afv_frame_match_fuse(afv_frame *f, const afv_proj_queries *q, int use_inf_gate, int32_t *best, int32_t *nfound);
/* SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (FeatureMatcher.cc:399-557) between two resident frames: the
 * queries are F1's own features (descriptor, angle, octave-0 filter: all on the device), prev_x / prev_y = vbPrevMatched (host, n1
 * floats each).  match12[n1], *nmatches.  Nothing but the 8 n1 bytes of vbPrevMatched is uploaded. */
int afv_frame_match_initialization(afv_frame *f1, afv_frame *f2, const float *prev_x, const float *prev_y, float window_size, float th_low,
                                   float nnratio, int check_orientation, int32_t *match12, int32_t *nmatches);
/* KeyFrame::KeyFrame(Frame &F, ...) (src/KeyFrame.cc:36-60): the frame's descriptors, angles, mvKeysUn, sigma2, mvuRight and - when
 * afv_frame_bow_transform ran - its FeatureVector become keyframe `slot` of the table, device to device (the node structure host to
 * host).  The slot's validity mask is reset to "all valid" like afv_table_set does.  Asynchronous on the context's stream. */
int afv_table_set_from_frame(afv_table *t, int slot, afv_frame *f);
/* afv_table_match_bow_frame with the frame side taken from a resident frame (afv_frame_bow_transform must have run): SearchByBoW(KF, F)
 * of TrackReferenceKeyFrame (Tracking.cc:626-629, one slot) and of Relocalization (:1162-1182, the candidates). */
int afv_table_match_bow_frame_h(afv_table *t, const int32_t *slots, int nslots, afv_frame *f, float th_low, float nnratio,
                                int check_orientation, int32_t *match_f, int32_t *nmatches);
/* ---- stereo and RGB-D frames: mvuRight / mvDepth made on the device ----
 * Frame::ComputeStereoMatches (src/Frame.cc:465-645) and Frame::ComputeStereoFromRGBD (:648-669).  The semantics are those of the plain
 * restatement tests/_stereo_ref.py, which the device is held to bit for bit; it follows the reference's routine (ORB-SLAM2's, which the
 * reference marks "has not been modified yet to work with AnyFeature-VSLAM") with three deviations: (A) the row band of a right keypoint is
 * 2 x ITS OWN keyPtsSize (the reference reads the left frame's size at the right index, :491); (B) rows outside [0, nRows) are dropped
 * (:496-497 index unchecked); (C) a keypoint whose 11 x 11 window or 11 x 21 search strip leaves its pyramid level, or whose octave is no
 * level, is skipped (the reference would assert inside OpenCV).  Caller data cannot take the search outside its arrays: a scaled
 * coordinate round(u / size), round(v / size), round(uR0 / size) that is not finite or beyond +-2^20 (a zero, denormal or NaN keyPtsSize,
 * a huge coordinate) skips the keypoint like (C); a left keypoint whose y is NaN or outside (-1, nRows) has no row; the ends of a right
 * keypoint's row band are clamped to +-2^30 and a NaN end makes the band empty.  Parity with a real build is unpinned: none exists.
 * New symbols and appended fields only: AFV_ABI_VERSION stays 6. */
/* host-only: the level sizes of the context's pyramid for a width x height image (width / height within the context's maxima, levels of
 * at least 32 px; else AFV_EINVAL): *nlevels, lw[AFV_MAX_LEVELS], lh[AFV_MAX_LEVELS] */
int afv_pyramid_level_sizes(afv_ctx *ctx, int width, int height, int32_t *nlevels, int32_t *lw, int32_t *lh);
/* the pyramid of a frame filled with afv_frame_set_features (any extractor's frames; tests): nlevels host images, level l tightly packed
 * lw[l] x lh[l] bytes, where nlevels / lw / lh are the context's geometry for a width x height image (afv_pyramid_level_sizes; another
 * level count or a NULL level: AFV_EINVAL).  Synchronous. */
int afv_frame_set_pyramid(afv_frame *f, int width, int height, const uint8_t *const *levels, int nlevels);
/* a kept pyramid level back on the host (tightly packed lw x lh; AFV_EINVAL without a pyramid) */
int afv_frame_get_pyramid_level(afv_frame *f, int level, uint8_t *out);
typedef struct {
    uint32_t struct_size;   /* sizeof(afv_stereo_params) */
    float mbf, fx;          /* Frame::mbf, fx: mb = mbf / fx, maxD = mbf / mb, minD = 0 (:501-503) */
    float th_high, th_low;  /* FeatureMatcher::TH_HIGH / TH_LOW: the search starts at th_high, thOrbDist = (th_high + th_low) / 2 */
} afv_stereo_params;
/* ComputeStereoMatches of `left` against `right`: both on one context (else AFV_EINVAL), with features and a pyramid each (else
 * AFV_EINVAL), of the same descriptor kind and size and pyramids of the same geometry (else AFV_EUNSUPPORTED).  The keypoints are the
 * frames' mvKeys (the distorted points), sizes their keyPtsSize.  Fills left's mvuRight / mvDepth planes (-1 where no match), which
 * afv_frame_match_projection / _fuse / afv_table_set_from_frame then read with no further call; *n_stereo (may be NULL) = features with
 * mvuRight >= 0.  Two launches (k_stereo_match, k_stereo_median) and a 4-byte copy of the count on the context's stream, one wait. */
int afv_frame_stereo_match(afv_frame *left, afv_frame *right, const afv_stereo_params *params, int32_t *n_stereo);
/* ComputeStereoFromRGBD: depth = a width x height image of floats (host, stride_bytes per row), read at the truncated distorted keypoint;
 * d > 0: mvDepth = d, mvuRight = mvKeysUn.x - mbf / d; else (and for a keypoint outside the image) both -1. */
int afv_frame_set_depth(afv_frame *f, const float *depth, int width, int height, int stride_bytes, float mbf);
/* mvuRight[n], mvDepth[n] and, after afv_frame_stereo_match, for tests: sad[n] = the SAD of an accepted pair before the median filter,
 * best_r[n] = the right index the descriptor search chose; -1 where none.  Any pointer may be NULL. */
int afv_frame_get_stereo(afv_frame *f, float *u_right, float *depth, int32_t *sad, int32_t *best_r);
/* ---- resident map points: Frame::isInFrustum and the projections in front of the projection searches, on the device ----
 * The geometry every projection search starts with - transform the map point into the camera, project it, test the image bounds, the
 * scale-invariance band and the viewing angle, predict size and window radius - runs in ONE kernel (k_points_project) over a
 * device-resident store of map points and the pose of the resident frame; a search then sends the ids of its points, 4 bytes per query.
 * The semantics are those of the plain restatement tests/_points_ref.py, which the device is held to bit for bit: float arithmetic, one
 * rounding per operator, three-term sums as a0 + (a1 + a2).  Parity with a build of the reference is unpinned (its last bit depends on its
 * toolchain).  Four rule sets, each as the reference writes it:
 *   AFV_PT_FRUSTUM    Frame::isInFrustum (Frame.cc:276-331) + the radius of SearchByProjection(F, vpMapPoints) (FeatureMatcher.cc:90-95,
 *                     :116-117): PcZ < 0.0f rejects; u < min || u > max rejects (inclusive bounds); dist < 0.8f * min_distance ||
 *                     dist > 1.2f * max_distance rejects; viewCos = dot / dist, viewCos < limit rejects; size = (ref_size * ref_distance) /
 *                     dist; r = ((radius_scale * radius_th) * RadiusByViewingCos(viewCos)) * size with (double)viewCos > 0.998 ? 2.5f : 4.0f;
 *                     the stereo gate is r * ((ref_sigma * ref_distance) / dist)
 *   AFV_PT_LASTFRAME  SearchByProjection(CurrentFrame, LastFrame) (FeatureMatcher.cc:1312-1351, :1369-1371): invzc < 0 rejects (z = -0.0f
 *                     rejects, z = +0.0f does not); inclusive bounds; no distance band, no viewing angle; size = keyPtsSize of feature q of
 *                     the LAST resident frame (qframe), whose angle plane gives the query angles; r = (radius_scale * radius_th) * size,
 *                     which is the stereo gate too
 *   AFV_PT_RELOC      SearchByProjection(CurrentFrame, pKF, sAlreadyFound) (:1425-1465): NO depth test; inclusive bounds; the distance
 *                     band; no viewing angle; predicted size; r = (radius_scale * radius_th) * size; no stereo gate
 *   AFV_PT_FUSE       Fuse (:811-858, :309-357, :968-1015): z < 0.0f rejects; KeyFrame::IsInImage: x >= min && x < max (half-open,
 *                     KeyFrame.cc:654-657); the distance band; dot < 0.5 * dist rejects; predicted size; r = (radius_scale * radius_th) * size
 * FRUSTUM, LASTFRAME and RELOC project u = ((fx * PcX) * invz) + cx, FUSE x = PcX * invz; u = (fx * x) + cx (they differ in the last bit).
 * q_ur = u - mbf * invz.  The size band of a query is size / sizeTolerance .. size * sizeTolerance (the frame's).
 * D1, the one deliberate deviation: a query whose u, v, r or size band is not finite (z = +0, dist = 0, NaN coordinates) is not in view;
 * the reference would hand such values to GetFeaturesInArea, whose float-to-int conversion is undefined.
 * Queries: ids[q] == -1, an id that was never set and a bad point are invalid queries (not in view; the slot stays in the list, so q stays
 * the last frame's feature index for LASTFRAME and the keyframe's for RELOC); the order of ids is the query order of the ordered phase;
 * a query occupies its feature (afv_proj_queries.qoccupies) when its point's `observed` flag is set.  What a plane holds for a query that is
 * not in view is 0.
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
typedef struct afv_points afv_points;
#define AFV_POINTS_MAX_CAPACITY (1 << 22)
/* a store of `capacity` map points (1 .. AFV_POINTS_MAX_CAPACITY, else AFV_EINVAL) whose descriptor rows are binary of desc_bytes 1 .. 64
 * (0 = 32), or, with float_dim > 0, float rows (a multiple of 4 up to 1024): the kinds and the row padding of frames.  It belongs to the
 * context and dies with it.  Per point id: pos[3] (MapPoint::XYZ), normal[3] (normalVector), min_distance / max_distance (the raw members:
 * the device applies 0.8f * and 1.2f * as the getters do, MapPoint.cc:420-430), ref_size, ref_distance, ref_sigma, the flags `bad` and
 * `observed` (NumberOfObservations() > 0), one descriptor row, and whether afv_points_set ever named it. */
int afv_points_create(afv_ctx *ctx, int capacity, int desc_bytes, int float_dim, afv_points **out);
void afv_points_destroy(afv_points *p);
/* The setters take HOST arrays over n ids (pos / normal: n x 3 floats; the others n floats / bytes / rows), copy them before they return and
 * work asynchronously on the context's stream.  An array that is NULL leaves that field as it is.  An id outside [0, capacity) refuses the
 * whole call with AFV_EINVAL before anything is written; the ids of one call are distinct (a repeated id keeps one of its values).
 * afv_points_set marks its ids as set. */
int afv_points_set(afv_points *p, const int32_t *ids, int n, const float *pos, const float *normal, const float *min_d, const float *max_d,
                   const float *ref_size, const float *ref_dist, const float *ref_sigma);
int afv_points_set_flags(afv_points *p, const int32_t *ids, int n, const uint8_t *bad, const uint8_t *observed);
/* rows: n x desc_bytes bytes (n x float_dim floats for a float store), packed */
int afv_points_set_descriptors(afv_points *p, const int32_t *ids, int n, const uint8_t *rows);
/* the row of feature idx[i] of keyframe slot[i] of a table, COPIED device to device now (MapPoint::ComputeDistinctiveDescriptors clones the
 * keyframe's row).  A table of another kind or width: AFV_EUNSUPPORTED; a slot or an index out of range: AFV_EINVAL, before anything moves. */
int afv_points_set_descriptors_from_table(afv_points *p, const int32_t *ids, int n, afv_table *table, const int32_t *slot, const int32_t *idx);
/* for tests: what the store holds for n ids, any pointer may be NULL; flags[i] = 1 (set) | 2 (bad) | 4 (observed).  Synchronous. */
int afv_points_get(afv_points *p, const int32_t *ids, int n, float *pos, float *normal, float *min_d, float *max_d, float *ref_size,
                   float *ref_dist, float *ref_sigma, uint8_t *flags, uint8_t *rows);
/* the pose of a resident frame and its intrinsics: Rcw row-major, tcw, Ow = twc as the host computes it with the reference's own
 * expression (Frame.cc:270-273, FeatureMatcher.cc:1416).  The image bounds are the frame's (afv_frame_params).  The searches below answer
 * AFV_EINVAL on a frame without a pose. */
int afv_frame_set_pose(afv_frame *f, const float *Rcw, const float *tcw, const float *Ow, float fx, float fy, float cx, float cy, float mbf);
enum { AFV_PT_FRUSTUM = 0, AFV_PT_LASTFRAME = 1, AFV_PT_RELOC = 2, AFV_PT_FUSE = 3 };
typedef struct {
    uint32_t struct_size;         /* sizeof(afv_point_search) */
    int32_t flavour;              /* AFV_PT_* */
    afv_points *points;
    const int32_t *ids;           /* [nq] host: point id | -1 */
    int32_t nq;                   /* <= 65535 */
    float radius_th, radius_scale, viewing_cos_limit; /* radiusTh; radiusScale (1.15f in the reference); FRUSTUM's viewingCosLimit */
    afv_frame *qframe;            /* LASTFRAME: the last frame (nq <= its count); RELOC without qangle: optional source of the query
                                     angles; ignored (never read) by the other flavours */
    const float *qangle;          /* RELOC: host alternative, [nq] degrees */
    const uint8_t *occupied;      /* per FRAME feature, as in afv_proj_queries; NULL = none */
    float th_high, nnratio;
    int32_t check_orientation;
} afv_point_search;
typedef struct {
    uint32_t struct_size;         /* sizeof(afv_point_projection) */
    int32_t n_in_view;            /* out */
    uint8_t *in_view;             /* host outputs over nq queries, any may be NULL */
    float *u, *v, *ur, *size, *sigma, *view_cos, *r, *qmin, *qmax; /* sigma: every flavour but LASTFRAME; view_cos: FRUSTUM */
    float *er;                    /* the stereo gate the search applies to |ur - mvuRight|: r * sigma (FRUSTUM), r (the others) */
} afv_point_projection;
/* FRUSTUM (searched in AFV_PROJ_LOCALMAP mode: Tracking::SearchLocalPoints, Tracking.cc:988-1028), LASTFRAME and RELOC (AFV_PROJ_LASTFRAME
 * mode): assign[n] (the QUERY INDEX now in F.pts[i] | -1), *nmatches; in_view[nq] (may be NULL) is what IncreaseVisible needs
 * (Tracking.cc:1010-1013), *n_in_view (may be NULL) their number.  One launch (k_points_project: geometry and descriptor gather) ahead of
 * the search kernels of afv_frame_match_projection.  AFV_EINVAL / AFV_EUNSUPPORTED before any launch: store and frame on different
 * contexts (EINVAL), a store of another descriptor kind or width than the frame (EUNSUPPORTED), no pose, qframe missing for LASTFRAME, an
 * id at or beyond the capacity, nq > 65535, an unknown struct_size, the wrong flavour for the entry point.  nq == 0 is legal. */
int afv_frame_search_points(afv_frame *f, const afv_point_search *s, int32_t *assign, int32_t *nmatches, uint8_t *in_view, int32_t *n_in_view);
/* AFV_PT_FUSE: best[nq] (feature index | -1), *nfound, as afv_frame_match_fuse */
int afv_frame_fuse_points(afv_frame *f, const afv_point_search *s, int use_inf_gate, int32_t *best, int32_t *nfound);
/* the projection alone, any flavour (tests; hosts that want mTrackProjX and the like) */
int afv_frame_project_points(afv_frame *f, const afv_point_search *s, afv_point_projection *host_out);

/* ---- pose optimisation: Optimizer::PoseOptimization (src/Optimizer.cc:245-448) for a resident frame.  It is what Tracking calls between
 * the searches (Tracking.cc:637, :760, :802 and, per candidate keyframe, :1247, :1263, :1278).  Everything it reads is on the device: mvKeysUn,
 * mvuRight and keyPtsInf with the frame, XYZ per point id in the store, the intrinsics and mbf with the frame's pose (afv_frame_set_pose).
 * A call uploads pts[N] (4 bytes per feature) and the initial pose of each job and runs ONE launch, one 1024-thread workgroup per job: the
 * four rounds, the Levenberg iterations and trials, the 6 x 6 solve and the classification all happen in the kernel (csrc/k_poseopt.hip).
 *
 * g2o is an empty directory in the reference: the arithmetic is restated after upstream g2o as bundled with ORB-SLAM2 - parity unpinned.
 * The normative semantics are tests/_poseopt_ref.py; the device is held to it bit for bit.  Feature i is an edge when pts[i] >= 0 and that
 * id was set in the store (isBad is not consulted, :282; a never-set id is no point); mvuRight[i] < 0 makes it a mono edge, else stereo.
 * Fewer than 3 edges: n_good = 0, rounds = 0, the pose comes back as it went in and no flag is set (:362).
 * Deliberate deviations from upstream:
 *   P1  every edge is classified at the round's final ACCEPTED pose (upstream leaves an inlier edge with the error of the last trial,
 *       rejected or not, when the call ends on a rejection).
 *   P2  a chi2 that is not finite is an outlier (upstream: NaN > th is false).
 *   P3  the state is R (3 x 3) and t in double; a step is R <- dR R, t <- dR t + V upsilon, no quaternion in between.
 *   P4  the coefficients of the exponential map are fixed 16-term Horner polynomials in theta^2, no library sin / cos; a step with
 *       theta^2 > pi^2 is a failed trial.  Their accuracy: (1 - cos)/theta^2 and (theta - sin)/theta^3 within 4 ulp of their values over
 *       [0, pi] (measured 2.9 and 1.6); sin/theta within 4 ulp of its value up to theta = 2 (2.3) and within 2^-52 ABSOLUTE (1.9e-16)
 *       beyond - 5.8 ulp of its value at 2.5, 29 at 3.0, 88 at 3.1, no relative accuracy at pi, where it crosses zero.
 *   P5  every sum over the edges is a perfect binary tree over the feature index (leaves: the smallest power of two >= max(N, 1); no active
 *       edge = +0.0); the 6 x 6 solve is an unpivoted L L^T in a fixed loop order, a pivot that is not positive and finite is a failed
 *       trial; a round with no active edge leaves the pose as it is.
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
typedef struct {
    uint32_t struct_size;         /* sizeof(afv_pose_job) */
    const int32_t *pts;           /* [N] host: point id | -1, N = the frame's feature count */
    const float *Rcw, *tcw;       /* the initial pose (9 floats row-major, 3 floats); both NULL = the frame's pose */
} afv_pose_job;
typedef struct {
    uint32_t struct_size;         /* sizeof(afv_pose_result), set by the caller */
    float Rcw[9], tcw[3];         /* out: the pose of the last round run (Converter::toMatrix4f) */
    int32_t n_good, n_edges, rounds; /* out: nInitialCorrespondences - nBad; nInitialCorrespondences; rounds run (0, 1 or 4) */
    uint8_t *outlier;             /* [N] host, may be NULL: mvbOutlier */
    int32_t iterations[4], trials[4]; /* out, per round: calls of OptimizationAlgorithmLevenberg::solve; trials in them */
    double chi2[4], lambda[4];    /* out, per round: the robust chi2 at its final pose; the final lambda (the trace the tests compare) */
} afv_pose_result;
/* njobs 1 .. 64 jobs on one frame (the relocalisation loop: one per candidate keyframe); synchronous; the frame's stored pose does not
 * change.  The intrinsics and mbf are the frame's, so the frame must have been given a pose once (afv_frame_set_pose) even when every job
 * brings its own.  AFV_EINVAL before any launch: NULL arguments, a frame without features (or whose mvKeysUn are missing), without a pose,
 * a job with only one of Rcw / tcw, more than AFV_POSE_MAX_FEATURES features, store and frame on different contexts, an id at or beyond the capacity, njobs out of range, an
 * unknown struct_size in either array.  The descriptor kind of the store does not matter here. */
int afv_frame_pose_optimize(afv_frame *f, afv_points *points, const afv_pose_job *jobs, int njobs, afv_pose_result *results);
#define AFV_POSE_MAX_JOBS 64
#define AFV_POSE_MAX_FEATURES 8192 /* features of the frame a call takes (eight per thread of the workgroup); more: AFV_EINVAL */

/* ---- new map points: the match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:315-461) over slots of the keyframe table.
 * It is what LocalMapping does with the answer of afv_table_match_triangulation: per match the parallax test, the linear triangulation
 * through a 4 x 4 SVD or a stereo unprojection, the two depth tests, the two reprojection gates, the scale-consistency test and the creation
 * of the map point.  One lane per (pair, feature i of keyframe a); TWO launches per call whatever the number of pairs, ONE wait
 * (csrc/k_triangulate.hip).  The normative semantics are tests/_tri_ref.py; the device is held to it bit for bit.  Float arithmetic, one
 * rounding per operator, three-term sums as a0 + (a1 + a2); `> 5.991 * sigmaSquare`, `> 7.8 * sigmaSquare` and `cosParallaxRays < 0.9998`
 * are evaluated in double as the reference does.  The SVD restates OpenCV 4.x's JacobiSVDImpl_<float> (one-sided Jacobi on the transposed
 * matrix, double accumulators, at most 30 sweeps, |p| <= eps * sqrt(a * b), descending sort) - parity unpinned, as is the whole routine.
 * Quirks restated as written: the stereo gate of the second keyframe uses the current keyframe's mbf (:438); KeyFrame::UnprojectStereo
 * reads the distorted keypoint (KeyFrame.cc:664-665).
 * Deliberate deviations:
 *   T1  cos(2 * atan2(mb / 2, depth)) is (d * d - h * h) / (d * d + h * h) in float, h = mb / 2; no library cos / atan2 is called
 *   T2  the Jacobi rotation's hypot(p, beta) is sqrt(p * p + beta * beta) in double, correctly rounded
 *   T3  a match whose x3D has a component that is not finite is rejected (the reference: every comparison against a NaN is false, the
 *       point would pass all gates and enter the map)
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
/* The planes the routine reads per feature next to afv_table_set_geometry's: KeyFrame::GetKeyPtSize(i), mvDepth[i] and the distorted
 * mvKeys[i].pt.  Called after afv_table_set_geometry of the same slot (else AFV_EINVAL), which it does not replace.  depth NULL: -1
 * everywhere; x_dist and y_dist NULL (both or neither): the undistorted points.  afv_table_set forgets them as it forgets the geometry;
 * afv_table_set_from_frame brings the frame's along (depth -1 for a frame without stereo / RGB-D data); afv_table_clone /
 * afv_table_broadcast ship them. */
int afv_table_set_scale(afv_table *t, int set, const float *size, const float *depth, const float *x_dist, const float *y_dist);
typedef struct {
    uint32_t struct_size;                                            /* sizeof(afv_tri_points_job) */
    float Rcw1[9], tcw1[3], Ow1[3], Rcw2[9], tcw2[3], Ow2[3];        /* row-major; Ow as the host computes GetCameraCenter */
    float fx1, fy1, cx1, cy1, invfx1, invfy1, fx2, fy2, cx2, cy2, invfx2, invfy2;
    float mb1, mb2, mbf1;                                            /* KeyFrame::mb of a and b, mbf of a (:412, :438) */
    float ratio_factor;                                              /* 1.5f * sizeTolerance (:260) */
    float max_size1;                                                 /* KeyFrame::maxKeyPtSize of a */
} afv_tri_points_job;
#define AFV_TRI_MAX_PAIRS 64
enum { AFV_TRI_NO_MATCH = 0, AFV_TRI_ACCEPTED = 1, AFV_TRI_LOW_PARALLAX = 2 /* the `else continue` at :381 */, AFV_TRI_W_ZERO = 3,
       AFV_TRI_Z1 = 4, AFV_TRI_Z2 = 5, AFV_TRI_REPROJ1 = 6, AFV_TRI_REPROJ2 = 7, AFV_TRI_ZERO_DIST = 8, AFV_TRI_SCALE_RATIO = 9,
       AFV_TRI_NOT_FINITE = 10 /* T3 */ };
enum { AFV_TRI_ROUTE_TRIANGULATED = 0, AFV_TRI_ROUTE_UNPROJECT_A = 1, AFV_TRI_ROUTE_UNPROJECT_B = 2 };
/* npairs 1 .. AFV_TRI_MAX_PAIRS pairs (a = the current keyframe, b = a neighbour), independent of each other; match12[npairs][cap] as
 * afv_table_match_triangulation returns it (feature of b per feature of a, -1 = none).  Host outputs, any may be NULL: status / route
 * [npairs][cap] (AFV_TRI_*), x3d [npairs][cap][3] (zeros where none was made: no match, low parallax, w == 0), new_id [npairs][cap] (-1 =
 * not accepted), n_new[npairs].  Accepted matches get the dense ids first_id + rank, the rank counted in pair order and within a pair by
 * ascending feature of a: the order in which the reference creates them.  With a store (`points`, may be NULL) each new id receives what
 * MapPoint::MapPoint + UpdateNormalAndDepth (MapPoint.cc:372-418) hold for a point with exactly these two observations and a as reference:
 * pos = x3D, normal = (n1 / |n1| + n2 / |n2|) / 2, ref_distance = |x3D - Ow1|, ref_size = size1[i], ref_sigma = sqrtf(sigma2_1[i]),
 * max_distance = ref_distance * ref_size, min_distance = max_distance / max_size1, flags set | observed (not bad), and row i of keyframe a
 * as descriptor, copied device to device (the semantics of afv_points_set_descriptors_from_table; afv_distinctive_descriptors recomputes
 * it later).  first_id + the number of new points beyond the store's capacity: AFV_ECAPACITY, the store and the output arrays untouched.
 * Before anything runs: a store of another kind or width than the table AFV_EUNSUPPORTED; AFV_EINVAL for NULL t / pair_a / pair_b / jobs /
 * match12, npairs out of range, first_id < 0, a slot out of range, a slot that holds features but lacks its geometry or its scale planes,
 * an unknown struct_size, a store of another context, a match12 entry outside [-1, n_b) or a match at a feature i >= n_a. */
int afv_table_triangulate(afv_table *t, const int32_t *pair_a, const int32_t *pair_b, const afv_tri_points_job *jobs, int npairs,
                          const int32_t *match12, afv_points *points, int32_t first_id, uint8_t *status, uint8_t *route, float *x3d,
                          int32_t *new_id, int32_t *n_new);
/* The neighbour loop of LocalMapping::CreateNewMapPoints (:265-472) in ONE call, with the reference's answer: what a caller gets from
 * afv_table_match_triangulation + afv_table_triangulate per neighbour with the masks "already has a map point" updated in between, bit for
 * bit, without going back to the host between the neighbours.  One upload (the FeatureVector joins, the pair records, the masks, the first
 * id), two launches per neighbour on the context's stream (csrc/k_newpoints.hip: the row search and the judgement of its match in one lane;
 * the ids, the store and the masks), one wait.  Only the mask of the current keyframe and the next free id pass from a neighbour to the
 * next; they stay on the device and the order of the stream carries them.
 *   cur, neighbours[nn]   the slot of the current keyframe and 1 .. AFV_TRI_MAX_PAIRS distinct neighbour slots other than cur, in the
 *                         order in which the reference visits them
 *   search[nn]            F12, ex, ey, th_low, only_stereo of neighbour k; has_mp1 / has_mp2 must be NULL (the masks travel below)
 *   jobs[nn]              a = cur, b = neighbours[k]
 *   has_mp_cur[cap]       in / out: the mask of cur; has_mp_nb[nn][cap] in / out: row k is the mask of neighbours[k]
 *   points, first_id      as afv_table_triangulate (points may be NULL: ids are counted, nothing is stored, no capacity rule)
 *   match12, status, route, x3d, new_id   [nn][cap] each (x3d [nn][cap][3]), any may be NULL; n_new[nn]; *n_done: neighbours completed
 * Neighbour k searches under the masks as neighbour k - 1 left them (row k of match12 is that search's answer), every match is judged as
 * afv_table_triangulate judges it, the accepted ones get the ids first_id + (accepted over neighbours 0 .. k - 1) + rank in feature order
 * and are stored as afv_table_triangulate stores them; then has_mp_cur[i] = 1 and has_mp_nb[k][j] = 1 for every accepted match (i, j).
 * CAPACITY.  The host cannot know the total in advance.  If the points of neighbour k would go beyond the store's capacity, neighbour k and
 * every later one do nothing: the call answers AFV_ECAPACITY with *n_done = k; neighbours 0 .. k - 1 stand in the store, the masks and the
 * outputs - the state the neighbour-by-neighbour loop leaves when its k-th afv_table_triangulate answers AFV_ECAPACITY.  UNLIKE
 * afv_table_triangulate THE OUTPUT ARRAYS ARE WRITTEN ON AFV_ECAPACITY: rows k .. nn - 1 read match12 -1, status 0, route 0, x3d 0, new_id
 * -1, n_new 0.  On AFV_OK *n_done = nn.
 * Refused before any launch, the masks and the store untouched: a store of another kind or width than the table AFV_EUNSUPPORTED;
 * AFV_EINVAL for NULL t / neighbours / search / jobs / has_mp_cur / has_mp_nb / n_new / n_done, nn out of range, first_id < 0, a slot out of
 * range, a neighbour equal to cur or listed twice, a search record whose has_mp1 / has_mp2 is not NULL or whose only_stereo is not 0 / 1,
 * an unknown struct_size, a store of another context, a slot that holds features but lacks its FeatureVector, its geometry or its scale
 * planes.  Nothing persists between calls.
 * Measured (README, "New map points on the device"; 20 neighbours of 1000 features, 986 new points, host to host, one run): 1.65 ms through
 * the Python wrapper against 3.26 ms for the neighbour-by-neighbour loop, 1.09 ms for this call alone, 0.99 ms of it in its 40 kernels.
 * New symbol only: AFV_ABI_VERSION stays 6. */
int afv_table_create_new_points(afv_table *t, int32_t cur, const int32_t *neighbours, int nn, const afv_table_tri_job *search,
                                const afv_tri_points_job *jobs, uint8_t *has_mp_cur, uint8_t *has_mp_nb, afv_points *points, int32_t first_id,
                                int32_t *match12, uint8_t *status, uint8_t *route, float *x3d, int32_t *new_id, int32_t *n_new,
                                int32_t *n_done);

/* ---- Sim3Solver: all RANSAC hypotheses of a loop check at once (src/Sim3Solver.cc:38-411, as LoopClosing::ComputeSim3 uses it,
 * src/LoopClosing.cc:247-416).  Per candidate keyframe the constructor (the filter over vpMatched12, X3Dc1 / X3Dc2, their images, the two
 * error bounds) and EVERY hypothesis h < nhyp (three draws, Horn's closed form on them, T12 and T21, CheckInliers over all N
 * correspondences) run on the device: two launches and ONE wait per call whatever the number of candidates (csrc/k_sim3.hip:
 * k_sim3_gather, one workgroup per candidate; k_sim3_hypotheses, one wavefront per (candidate, hypothesis)).  Hypothesis h depends on
 * (seed, h) alone, so the sequential rule of Sim3Solver::iterate (running best, return on > minInliers) is a scan over count[h] that the
 * host does exactly (afv::Sim3Solver of the adapter, Sim3Solver of the Python package).
 * The normative semantics are tests/_sim3_ref.py; the device is held to it bit for bit - parity with a build of the reference is
 * unpinned.  Float arithmetic, one rounding per operator, a three-term sum (a row of a 3 x 3 product, a dot product) as a0 + (a1 + a2),
 * scalar expressions left to right as written; double where the reference accumulates in double: cv::Mat::dot (nom, err1, err2), den.
 * Quirks restated as written:
 *   Q1  mvnMaxError1/2 are vector<size_t>: the bound is (size_t)(9.210 * sigmaSquare), truncated, and err < bound compares in float
 *   Q2  the best hypothesis is updated on mnInliersi >= mnBestInliers, iterate returns on mnInliersi > mRansacMinInliers (strict)
 *   Q3  SetRansacParameters: epsilon in float, ceil(log(1 - p) / log(1 - pow(epsilon, 3))) in double, max(1, min(nIterations,
 *       maxIterations)); host mathematics only
 * Deliberate deviations:
 *   S1  the reference assigns N(0..2,3) from row 3, which was never written (:254-256); here N is Horn's symmetric matrix:
 *       N(3,0..2) = N(0..2,3) as computed at :242, :247, :252
 *   S2  the eigenvector of the largest eigenvalue comes from a cyclic Jacobi on the symmetric 4 x 4 in double: pairs (0,1) (0,2) (0,3)
 *       (1,2) (1,3) (2,3); only + - * / and sqrt; at most 12 sweeps, a pair is skipped when a_pq == 0 or |a_pp| + |a_pq| == |a_pp| and
 *       |a_qq| + |a_pq| == |a_qq|, a sweep that rotates nothing ends it; ties on the maximum go to the lowest index.  It replaces
 *       Eigen::EigenSolver
 *   S3  R12 is built directly from the normalised quaternion, in double, then rounded to float; it replaces atan2 + cv::Rodrigues
 *   S4  draws come from the counter-based generator of the vocabulary trainer: sm = splitmix64, key_h = sm(sm(seed) ^ (h + 1)), draw
 *       d in {0, 1, 2} = sm(key_h + (d + 1) * 0xD1342543DE82EF95) % (N - d), applied to vAvailableIndices with the reference's
 *       swap-with-back removal (:166-173)
 *   S5  a hypothesis is degenerate if den (when the scale is estimated), s12i, R12 or t12 is not finite, or den == 0: it counts 0
 *       inliers, is flagged, and its sim3 record and inlier words read 0.  A correspondence whose error is not finite is not an inlier
 *       (the comparisons as written).  A sigma2 that is negative or not finite gives bound 0
 *   S6  N < 3 evaluates no hypothesis: all counts 0, no flag (callers reach bNoMore first: min_inliers >= 3 is required)
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_sim3_job) */
    int32_t fix_scale;                       /* mbFixScale: 0 / 1 */
    uint32_t seed_lo, seed_hi;               /* the 64-bit seed of S4 */
    float Rcw1[9], tcw1[3], Rcw2[9], tcw2[3]; /* row-major; 1 = the current keyframe, 2 = the candidate */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
} afv_sim3_job;
#define AFV_SIM3_MAX_CANDIDATES 64
#define AFV_SIM3_MAX_HYPOTHESES 1024
#define AFV_SIM3_MAX_MASK_WORDS 256 /* mask_words 0 .. 256: twice what the largest table (cap 4096) needs */
/* nc 1 .. AFV_SIM3_MAX_CANDIDATES candidates: slot_a[c] holds keyframe 1 (mN1 = its feature count n1), slot_b[c] keyframe 2.  Host rows
 * of `cap` (the table's) ints per candidate, of which entries i1 < n1 are read: mp1 = the map-point id of feature i1 of keyframe 1
 * (vpKeyFrameMP1), mp2 = vpMatched12[i1], -1 = none; idx1 / idx2 = GetIndexInKeyFrame of the two points in their keyframes (idx1 NULL:
 * i1 itself).  A correspondence survives when mp2 >= 0, mp1 >= 0, neither point is bad in the store (an id that was never set counts as
 * bad), idx1 >= 0 and idx2 >= 0; the survivors keep the order of i1.  Outputs (host): n[nc] = N; index1[nc][cap] = mvnIndices1 (-1 from
 * N on); count / degenerate [nc][nhyp]; sim3[nc][nhyp][13] = R12 row-major, t12, s12 (T12 = [s12 * R12 | t12]); inliers
 * [nc][nhyp][mask_words], bit k of the row = correspondence k, unused bits 0; optional x3dc1 / x3dc2 [nc][cap][3] (mvX3Dc1/2) and
 * max_err[nc][cap][2] (the two Q1 bounds as floats), 0 from N on.
 * Refused before any launch, nothing written: AFV_EINVAL for NULL t / points / slot_a / slot_b / jobs / mp1 / mp2 / idx2 / n / index1 /
 * count / degenerate / sim3 / inliers, nc, nhyp or mask_words out of range, an unknown struct_size, a fix_scale other than 0 / 1, a slot out of
 * range or one holding features without geometry, a store of another context, an id outside [-1, capacity), an idx outside [-1, n_slot),
 * mask_words * 32 below the largest number of entries with mp1, mp2, idx1, idx2 >= 0 of a candidate.  The store's descriptor kind and
 * width do not matter: descriptors are not read. */
int afv_table_sim3_hypotheses(afv_table *t, afv_points *points, const int32_t *slot_a, const int32_t *slot_b, const afv_sim3_job *jobs, int nc,
                              const int32_t *mp1, const int32_t *mp2, const int32_t *idx1, const int32_t *idx2, int nhyp, int mask_words,
                              int32_t *n, int32_t *index1, int32_t *count, uint8_t *degenerate, float *sim3, uint32_t *inliers, float *x3dc1,
                              float *x3dc2, float *max_err);

/* ---- OptimizeSim3: the Sim3 of every loop candidate refined in one call (Optimizer::OptimizeSim3, src/Optimizer.cc:1033-1226, as
 * LoopClosing::ComputeSim3 calls it at src/LoopClosing.cc:342).  Everything the routine reads is resident: mvKeysUn of the two keyframes
 * (the table's geometry planes), GetKeyPt2DInf (the table's information plane, afv_table_set_inf), XYZ and isBad of the points (the
 * store).  One upload, two launches, one wait per call whatever the number of candidates (csrc/k_sim3opt.hip: k_sim3opt_gather, one
 * workgroup per job: the edge set; k_sim3opt_solve, ONE WAVEFRONT per job: both optimize() calls and both classifications, the estimate,
 * H, b and lambda lane-uniform in registers, the lanes striding over the correspondences, no barrier, no LDS).
 * The normative semantics are tests/_sim3opt_ref.py (double, one rounding per operator, every operator order fixed there); the device
 * is held to it bit for bit.  g2o is not shipped by the reference, so what it runs is restated after upstream g2o as bundled with
 * ORB-SLAM2 - parity with a real g2o is UNPINNED.
 * The edge set (:1084-1163): feature i of keyframe 1 is a correspondence when mp2[i] >= 0, mp1[i] >= 0, both ids are set in the store
 * and not bad, and idx2[i] >= 0.  A match that fails the filter stays in vpMatches1: it is no edge, and it is not removed.
 * Deliberate deviations from upstream (the numbering of tests/_sim3opt_ref.py):
 *   O1  both classifications are made at the accepted estimate (P1 of PoseOptimization)
 *   O2  a chi2 that is not finite is an outlier (P2)
 *   O3  the state is R (3 x 3), t and s in double; a step is R <- dR R, t <- ds (dR t) + dt, s <- ds s; no quaternion, the caller's R12
 *       is taken as given (P3)
 *   O4  no library sin / cos / exp: sin(th)/th, (1 - cos th)/th^2, (th - sin th)/th^3 are PoseOptimization's 16-term Horner polynomials in
 *       th^2 (sin th = th * A, cos th = 1 - th^2 * B); exp(sigma) = 2^k * P(r), k = floor(sigma * log2(e) + 0.5), r = (sigma - k * ln2_hi)
 *       - k * ln2_lo, P the Taylor polynomial of degree 13 by Horner; measured against math.exp over |sigma| <= 64: at most 1 ulp.  A step
 *       with th^2 > pi^2, or a sigma that is not finite or beyond 64 in magnitude, is a failed trial
 *   O5  every sum over the correspondences (28 + 7 + 1 per linearisation, 1 per trial): 64 partial sums, partial l adds the terms of
 *       the correspondences l, l + 64, ... (positions in the edge list) in ascending order, a correspondence contributing e12's term +
 *       e21's term, a removed one nothing; then p[l] += p[l + s], s = 32 .. 1
 *   O6  the 7 x 7 solve is an unpivoted L L^T in a fixed order; a pivot that is not positive and finite is a failed trial.  With
 *       fix_scale the numeric Jacobian's scale column is exactly zero, so row 6 holds lambda alone and the scale's bits never change
 *   O7  a problem without (remaining) edges evaluates nothing: optimize() leaves the estimate and reports 0 iterations
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_sim3opt_job) */
    int32_t fix_scale;                       /* bFixScale: 0 / 1 */
    float th2;                               /* th2; the Huber delta is sqrtf(th2) */
    float Rcw1[9], tcw1[3], Rcw2[9], tcw2[3]; /* row-major; 1 = the current keyframe, 2 = the candidate */
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
    float R12[9], t12[3], s12;               /* g2oS12 as Sim3Solver::GetEstimatedRotation / Translation / Scale return it */
} afv_sim3opt_job;
typedef struct {
    int32_t n_in;                            /* what OptimizeSim3 returns */
    int32_t n_corr, n_bad, more_iterations;  /* nCorrespondences, nBad of the first check, nMoreIterations (10 / 5) */
    int32_t early;                           /* 1: nCorrespondences - nBad < 10, the call answered 0 and R12 / t12 / s12 are the job's */
    int32_t iterations[2], trials[2];        /* per optimize() call */
    int32_t reserved;
    double R12[9], t12[3], s12;              /* g2oS12 after the call */
    double chi2[2], lambda[2];               /* the robust chi2 and lambda each optimize() call ended with */
} afv_sim3opt_result;
/* state[nc][cap], one byte per feature of keyframe 1 (0 from n1 on) */
#define AFV_SIM3OPT_NO_MATCH 0       /* mp2 < 0 */
#define AFV_SIM3OPT_NOT_EDGE 1       /* a match that fails the filter: kept in vpMatches1 */
#define AFV_SIM3OPT_KEPT 2           /* an edge whose match stays (an inlier unless the call answered 0 early) */
#define AFV_SIM3OPT_REMOVED_FIRST 3  /* removed by the check after optimize(5) */
#define AFV_SIM3OPT_REMOVED_SECOND 4 /* removed by the check after optimize(nMoreIterations) */
/* nc 1 .. AFV_SIM3_MAX_CANDIDATES jobs; slots, mp1 / mp2 / idx2 rows of `cap` ints as afv_table_sim3_hypotheses takes them (no idx1:
 * the observation of keyframe 1 is feature i itself, :1127).  Outputs (host): results[nc], state[nc][cap].
 * Refused before any launch, nothing written: AFV_EINVAL for a NULL argument, nc out of range, an unknown struct_size, a fix_scale other
 * than 0 / 1, a slot out of range, one holding features without geometry or without the information plane (afv_table_set_inf), a store
 * of another context, an id outside [-1, capacity), an idx2 outside [-1, n_slot_b).  Descriptors are not read. */
int afv_table_optimize_sim3(afv_table *t, afv_points *points, const int32_t *slot_a, const int32_t *slot_b, const afv_sim3opt_job *jobs, int nc,
                            const int32_t *mp1, const int32_t *mp2, const int32_t *idx2, afv_sim3opt_result *results, uint8_t *state);
/* GetKeyPt2DInf of a slot's features (inf[n]: the information of feature i is inf[i] * I), after afv_table_set_geometry of the same slot.
 * afv_table_set_from_frame brings the frame's keyPtsInf, afv_table_clone and afv_table_broadcast carry the plane, afv_table_set forgets
 * it.  Only afv_table_optimize_sim3 reads it. */
int afv_table_set_inf(afv_table *t, int set, const float *inf);

/* ---- Bundle adjustment: Optimizer::LocalBundleAdjustment (src/Optimizer.cc:450-768, as LocalMapping calls it after every keyframe) and
 * Optimizer::BundleAdjustment (:61-243: the two-keyframe BA of the monocular start-up, global BA) over slots of the keyframe table and
 * ids of the map-point store.  Everything the routines read is resident: mvKeysUn, mvuRight and GetKeyPt2DInf of every keyframe (the
 * table's geometry, u_right and information planes), GetWorldPos and isBad of every point (the store).
 * The normative semantics are tests/_lba_ref.py (double, one rounding per operator, every operator order fixed there); the device is held
 * to it bit for bit.  g2o is not shipped by the reference, so what it runs (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ with both
 * Jacobians, BaseBinaryEdge::constructQuadraticForm, BlockSolver_6_3 with the points marginalised, OptimizationAlgorithmLevenberg) is
 * restated after upstream g2o as bundled with ORB-SLAM2 - parity with a real g2o is UNPINNED.
 * The first n_free keyframes are optimised, the others are fixed (the host puts keyId == 0 and lFixedCameras there).  Edge e joins point
 * obs_point[e] (a position in point_ids) with feature obs_idx[e] of keyframe obs_kf[e] (a position in slots), in the order in which the
 * reference adds edges (per point, per observation): obs_point is ascending.  A feature is a stereo edge when its u_right >= 0; its
 * information is diag(inf, inf, 0.5f * (inf + inf)) (GetKeyPt3DInf), a mono edge's inf * I2.  A point id that is unset or bad in the
 * store drops the point and its edges (:475-476).
 * params.checks = 1: LocalBundleAdjustment - optimize(iterations[0]) under the kernel if robust[0], the first check (level 1 on chi2 >
 * 5.991 / 7.815 || !isDepthPositive), optimize(iterations[1]) with robust[1], the final check that fills vToErase; the reference's values
 * are iterations {5, 10}, robust {1, 0}.  checks = 0: BundleAdjustment - one optimize(iterations[0]) with robust[0], no check.
 * Quirk kept (L-Q1): the final check visits the edges removed by the first check too, with the chi2 of the first check (upstream caches
 * _error) and the depth test at the final estimate - an edge removed for depth alone can survive (AFV_LBA_EDGE_REMOVED_KEPT).
 * The launches (csrc/k_lba.hip): one gather per call; per iteration k_lba_linearise (a lane per edge), k_lba_build (a wavefront per free
 * keyframe, a lane per point), k_lba_begin; per trial k_lba_invert (a lane per point), k_lba_schur (a wavefront per block of the reduced
 * system), k_lba_solve (one workgroup: dense L L^T of at most 384 x 384), k_lba_step, k_lba_trial, k_lba_judge, then ONE wait in which
 * the host reads the status record (a few dozen bytes) and the stop flag - exactly where g2o's terminate() stands.  The accept / reject
 * decision, lambda and ni are the device's; the host only follows them.  No spinning flag, no cooperative launch, no captured graph.
 * Deliberate deviations from upstream (the numbering of tests/_lba_ref.py, where the full text is):
 *   L1  both checks are made at the accepted estimate (P1 / O1)      L2  a chi2 that is not finite is an outlier
 *   L3  the state is R, t in double, no quaternion                   L4  no libm (P4's Horner tables); a step beyond pi is a failed trial
 *   L5  every sum has one fixed shape: per keyframe (Hpp, bp, the Schur sums of block row i) 64 strided partial sums over that keyframe's
 *       edges in list order, then p[l] += p[l + s], s = 32 .. 1; per point (Hll, bl, the back substitution) its edges one after the
 *       other; the chi2 and scale sums the same 64-partial tree over the edge list and over the unknowns (poses, then points)
 *   L6  Hll^-1 by cofactors in a fixed order; a determinant that is 0 or not finite is a failed trial
 *   L7  the reduced system is solved by a dense, unpivoted L L^T in the order of the free-keyframe list, element (i, j) subtracting its
 *       products in ascending k (forward substitution ascending, back substitution descending); a pivot that is not positive and
 *       finite is a failed trial.  A vertex without active edges stays in the system: its block holds lambda alone, its step is 0
 *   L8  a problem without free keyframes, without points or without (active) edges evaluates nothing
 *   L9  what is not written reads 0: xyz_out of a dropped point, the trace of a round that did not run
 * The stop flag: stop_flag (a host variable, or NULL) is read before the call, before every iteration, after every trial and before the
 * first check; params.trial_budget > 0 raises it deterministically from the moment that many trials have run.  Raised before the call
 * with checks = 1: the return at :645-647 - results holds stopped = 1 and zeros, nothing else is written, the store is unchanged.
 * Raised during the first optimize(): bDoMore = false - the first check and the second optimize() are skipped, the final check and
 * the write-back run.
 * What the host still does: EraseMapPointMatch / EraseObservation for every edge in state AFV_LBA_EDGE_ERASE and SetPose from kf_out stay
 * with the host's map.  UpdateNormalAndDepth of the moved points no longer does: afv_table_refresh_points (below) takes the same
 * observation arrays and refreshes the store on the device.
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
#define AFV_LBA_MAX_FREE 64
#define AFV_LBA_MAX_KF 256
#define AFV_LBA_MAX_POINTS 32768
#define AFV_LBA_MAX_EDGES 262144
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_lba_cam) */
    float Rcw[9], tcw[3];                    /* GetPose(), row-major */
    float fx, fy, cx, cy, bf;                /* bf = mbf (read by stereo edges only) */
} afv_lba_cam;
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_lba_params) */
    int32_t iterations[2], robust[2];        /* per optimize() call */
    int32_t checks;                          /* 1: LocalBundleAdjustment's two checks; 0: BundleAdjustment, one round */
    int32_t write_points;                    /* 1: the store receives (float)xyz_out (SetWorldPos); 0: it stays (the nLoopKF != 0 path) */
    int32_t trial_budget;                    /* 0: none; k: the stop flag reads raised once k trials have run */
} afv_lba_params;
typedef struct {
    int32_t iterations[2], trials[2];        /* per optimize() call */
    int32_t n_edges, n_removed_first, n_erase;
    int32_t stopped;                         /* 0 no; 1 before the call; 2 in the first optimize(); 3 in the second */
    double chi2[2], lambda[2];               /* the robust chi2 and lambda each optimize() call ended with */
} afv_lba_result;
#define AFV_LBA_EDGE_DROPPED 0       /* its point is unset or bad in the store */
#define AFV_LBA_EDGE_KEPT 1
#define AFV_LBA_EDGE_REMOVED_KEPT 2  /* removed by the first check, not in vToErase (L-Q1) */
#define AFV_LBA_EDGE_ERASE 3         /* in vToErase */
/* slots[nk], cams[nk], point_ids[np], obs_point / obs_kf / obs_idx[ne] (host).  Outputs (host): results[1], kf_out[n_free][12] (R
 * row-major, t; double), xyz_out[np][3] (double; the store receives the float cast when write_points), edge_state[ne].
 * Refused before any launch, outputs untouched: AFV_EINVAL for a NULL argument, an unknown struct_size, nk > AFV_LBA_MAX_KF, n_free >
 * min(nk, AFV_LBA_MAX_FREE), np > AFV_LBA_MAX_POINTS, ne > AFV_LBA_MAX_EDGES or a negative count, iterations below 0, robust / checks /
 * write_points other than 0 / 1, a negative trial_budget, a slot out of range or one holding features without geometry or without the
 * information plane, a store of another context, a point id outside [0, capacity) or named twice, obs_point / obs_kf / obs_idx out of
 * range, edges not grouped by point (obs_point descending somewhere), a point observed twice by one keyframe.  Descriptors are not read. */
int afv_table_bundle_adjust(afv_table *t, afv_points *points, const int32_t *slots, int nk, int n_free, const afv_lba_cam *cams,
                            const int32_t *point_ids, int np, const int32_t *obs_point, const int32_t *obs_kf, const int32_t *obs_idx, int ne,
                            const afv_lba_params *params, const volatile int32_t *stop_flag, afv_lba_result *results, double *kf_out,
                            double *xyz_out, uint8_t *edge_state);

/* ---- Global bundle adjustment: Optimizer::GlobalBundleAdjustemnt (src/Optimizer.cc:53-58) as LoopClosing::RunGlobalBundleAdjustment
 * calls it after every loop closure (LoopClosing.cc:664: every keyframe of the map free except keyId == 0), and any bundle adjustment
 * with more than AFV_LBA_MAX_FREE free keyframes.  The arguments, the records (afv_lba_cam, afv_lba_params, afv_lba_result), the outputs,
 * the edge states, the stop-flag rule and the refusals are those of afv_table_bundle_adjust; both values of params.checks are accepted.
 * The normative semantics are tests/_gba_ref.py: tests/_lba_ref.py (L-Q1, L1 - L6, L8, L9, the order of every sum) with one amendment:
 *   L7' the reduced system is block-sparse in 6 x 6 blocks over the free keyframes, in the order of the caller's list.  Block (i, j) is
 *       structural when some listed point has an edge to both keyframes - taken from the edge list as given, before points are dropped
 *       and before a check removes edges, so a block that became empty holds exact zeros.  The factorisation is the unpivoted L L^T of L7
 *       restricted to the symbolic fill of that order: every scalar element subtracts its products one after the other in ascending k,
 *       the products with a factor in a block outside the fill are skipped; the forward substitution ascends, the back substitution
 *       descends, each product by product; a pivot that is not positive and finite is a failed trial; a free keyframe without active
 *       edges stays in the system with lambda on its diagonal.  On finite data this gives the doubles of L7 (skipping s - (+-0) changes
 *       nothing unless s is -0.0); where a zero sign ever differs, L7' is normative for this entry point.
 * On an input that both entry points accept they answer the same bytes.
 * The launches: those of afv_table_bundle_adjust, with k_lba_schur and k_lba_solve replaced per trial by k_gba_schur (a wavefront per
 * block of L from the plan's list: a structural block is evaluated and stored where it loads to, a fill block is zeroed) and
 * k_gba_factor (ONE workgroup walks the block columns: diagonal 6 x 6 factorisation, sub-diagonal blocks a lane per row, updates a lane
 * per entry, both substitutions in the same launch); csrc/k_gba.hip.  The dense n x n matrix is not allocated.  The host derives the plan
 * (the structural blocks, the column structure of L by symbolic elimination in list order) while it checks the arguments and uploads
 * it with the inputs in the call's one copy; one wait per trial, as before.
 * The capacities.  AFV_GBA_MAX_KF is the essential graph's (the same map goes through both).  A block of L costs 288 bytes + 9 bytes of
 * plan: 297 MiB at AFV_GBA_MAX_L_BLOCKS.  No update triples are stored (the kernel finds an update's target by a binary search in the
 * target column), so there is no cap on them.  An edge costs about 0.5 KB of device scratch (its 55 terms, observation, chi2 and
 * lists): 1.0 GiB at AFV_GBA_MAX_EDGES; a point 0.3 KB: 0.15 GiB at AFV_GBA_MAX_POINTS.  The context's arena has no limit of its own
 * below that (it is one device allocation that grows by half again: 2.2 GiB at all caps together).  A keyframe order whose fill exceeds
 * AFV_GBA_MAX_L_BLOCKS answers AFV_ECAPACITY before any launch, outputs and store untouched.
 * New symbols only: AFV_ABI_VERSION stays 6. */
#define AFV_GBA_MAX_KF 4096
#define AFV_GBA_MAX_POINTS 524288
#define AFV_GBA_MAX_EDGES 2097152
#define AFV_GBA_MAX_L_BLOCKS 1048576
/* Refused before any launch, outputs and store untouched: everything afv_table_bundle_adjust refuses, with nk > AFV_GBA_MAX_KF, n_free >
 * nk, np > AFV_GBA_MAX_POINTS, ne > AFV_GBA_MAX_EDGES in the place of its caps (AFV_EINVAL); AFV_ECAPACITY for a fill beyond
 * AFV_GBA_MAX_L_BLOCKS. */
int afv_table_global_bundle_adjust(afv_table *t, afv_points *points, const int32_t *slots, int nk, int n_free, const afv_lba_cam *cams,
                                   const int32_t *point_ids, int np, const int32_t *obs_point, const int32_t *obs_kf, const int32_t *obs_idx, int ne,
                                   const afv_lba_params *params, const volatile int32_t *stop_flag, afv_lba_result *results, double *kf_out,
                                   double *xyz_out, uint8_t *edge_state);
/* Internal, for the tests of the capacity answer: the plan of an edge list (obs_point ascending; obs_kf < n_free: a free keyframe)
 * against a block cap of the caller's choice - the entry point above always uses AFV_GBA_MAX_L_BLOCKS.  AFV_OK with counts[3] = the
 * blocks of L, the structural blocks among them, n_free; AFV_ECAPACITY (counts untouched) when the fill exceeds max_blocks.  No device is
 * touched. */
int afv_gba_plan_probe(int n_free, int np, const int32_t *obs_point, const int32_t *obs_kf, int ne, long long max_blocks, int32_t *counts);
/* The point correction of RunGlobalBundleAdjustment for the points the BA did not optimise (LoopClosing.cc:731-750): point ids[i] moves
 * to Rwc * (Rcw_bef * X + tcw_bef) + twc with q = pair_of_point[i], IN FLOAT, in the store, in place: T_before[q] = (Rcw, tcw) of the
 * reference keyframe before the BA (mTcwBefGBA), T_after[q] = (Rwc, twc) as the host's GetPoseInverse() holds it after SetPose(TcwGBA)
 * - nothing is inverted here; each record is 12 floats, R row-major, then t.  Each row is ((R[r][0] * x + R[r][1] * y) + R[r][2] * z) +
 * t[r], one rounding per operator (tests/_gba_ref.py, correct_se3; parity with the reference's cv::Mat product is UNPINNED).
 * afv_points_correct_sim3 works in double and is another arithmetic.  status[i] is AFV_POINT_MOVED, AFV_POINT_BAD_OR_UNSET or
 * AFV_POINT_NO_PAIR (q == -1).  One upload, one launch, one wait.  Refused before any launch, the store untouched: AFV_EINVAL for a NULL
 * argument, n < 0, n beyond the store's capacity, m outside 0 .. AFV_GBA_MAX_KF, an id outside [0, capacity) or named twice, a pair
 * outside [-1, m), a transform that is not finite.  The spanning-tree walk over the poses (:690-714) and SetPose stay with the host. */
int afv_points_correct_se3(afv_points *points, const int32_t *ids, int n, const int32_t *pair_of_point, const float *T_before, const float *T_after,
                           int m, uint8_t *status);

/* ---- Refresh of resident map points from their observations: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:279-349) and
 * MapPoint::UpdateNormalAndDepth (:372-418) for a batch of points, every row and every plane read where it is resident (the keyframe
 * table, the store).  The reference calls the two after BundleAdjustment (Optimizer.cc:234), LocalBundleAdjustment (:766) and
 * OptimizeEssentialGraph (:1029), at the end of SearchInNeighbors (LocalMapping.cc:547-548), in CorrectLoop (LoopClosing.cc:515) and
 * when an observation is added, erased or replaced (MapPoint.cc:120 / :172 / :249).
 * The observation arrays have the format and order of afv_table_bundle_adjust: grouped by point, obs_point ascending (a position in
 * point_ids), obs_kf a position in slots, and inside a point the order of the reference's map<KeyframeId, Obs>.  centres[k] is
 * GetCameraCenter() of keyframe k as the host computes it (the rule of afv_frame_set_pose for Ow), max_size[k] its maxKeyPtSize,
 * kf_bad[k] (NULL: none) its isBad(), ref_kf[p] the position of mpRefKF of point p in slots.
 * The normative semantics are tests/_refresh_ref.py (float, one rounding per operator); the device is held to it bit for bit.
 * A point that is unset or bad in the store is skipped by both parts, and so is a point without observations.
 * params.descriptors = 1: the observations of keyframes that are not kf_bad, in list order, are the N rows; per row the median =
 *   the floor(0.5 (N - 1))-th smallest of its N distances (its own 0 included); the least median wins, the first row on a tie; the
 *   distance is Hamming over desc_bytes (pad bytes are not counted) or, for float tables, cv::norm(NORM_L2SQR) as a float.  The winning
 *   row is copied into the store device to device (the semantics of afv_points_set_descriptors_from_table); N = 0 leaves the row as it is.
 * params.normals = 1: EVERY observation contributes, bad keyframes too (the routine does not test isBad):
 *   normal = (0.0f + n_0 / |n_0| + ...) / n summed in list order; ref_distance = |XYZ - centre(ref)|; ref_size = the table's keyPtsSize
 *   of the ref keyframe's observation; ref_sigma = sqrtf(its sigma2); max_distance = ref_distance * ref_size; min_distance =
 *   max_distance / max_size[ref].  It reads mpRefKF (ref_kf), NOT the refKeyframe the descriptor part has just chosen: the reference
 *   keeps two reference keyframes, and so does this.
 * Deliberate deviations:
 *   R1  a point whose ref_kf is -1, or which ref_kf does not observe, answers AFV_REFRESH_NO_REF and its normal part is not written (the
 *       reference would dereference a null Obs)
 *   R2  a point with an observation at distance 0 or at a distance that is not finite answers AFV_REFRESH_BAD_DISTANCE and its normal
 *       part is not written (R1 is tested first)
 *   R3  what is not written reads 0 in the host outputs (best_obs: -1)
 * The planes and the row of a skipped point are untouched, and so is every point the call does not name.
 * One upload, one launch per part (csrc/k_refresh.hip: a wavefront per point) on the context's stream, one wait.  No atomics.
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_refresh_params) */
    int32_t descriptors;                     /* 1: ComputeDistinctiveDescriptors */
    int32_t normals;                         /* 1: UpdateNormalAndDepth */
} afv_refresh_params;
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_refresh_out) */
    int32_t reserved;
    int32_t *status;                         /* [np] AFV_REFRESH_*; host arrays, any of which may be NULL */
    int32_t *best_obs;                       /* [np] the position in the observation arrays of the winning row: the host sets refKeyframe /
                                              * refIndex from it; -1: nothing was chosen */
    int32_t *best_median;                    /* [np] its median: an int32 for binary tables, the bits of the float for float tables */
} afv_refresh_out;
#define AFV_REFRESH_DONE 0           /* every part that was asked for was written (the descriptor part: unless N = 0) */
#define AFV_REFRESH_SKIPPED 1        /* the point is unset or bad in the store */
#define AFV_REFRESH_NO_OBSERVATIONS 2
#define AFV_REFRESH_NO_REF 3         /* R1: the descriptor part ran, the normal part did not */
#define AFV_REFRESH_BAD_DISTANCE 4   /* R2: likewise */
/* slots[nk], centres[nk][3], max_size[nk], kf_bad[nk] | NULL, point_ids[np], ref_kf[np], obs_point / obs_kf / obs_idx[ne] (host).
 * Refused before any launch, the store and the outputs untouched: AFV_EINVAL for a NULL argument (kf_bad and the members of out
 * excepted), an unknown struct_size, descriptors / normals other than 0 / 1, nk > AFV_LBA_MAX_KF, np > AFV_LBA_MAX_POINTS, ne >
 * AFV_LBA_MAX_EDGES or a negative count, a store of another context, a slot out of range or one holding features without geometry or
 * (normals) without the scale plane, a point id outside [0, capacity) or named twice, ref_kf outside [-1, nk), obs_point / obs_kf /
 * obs_idx out of range, observations not grouped by point, a point observed twice by one keyframe, more than 65535 observations of one
 * point; AFV_EUNSUPPORTED for a store whose row kind or width is not the table's. */
int afv_table_refresh_points(afv_table *t, afv_points *points, const int32_t *slots, int nk, const float *centres, const float *max_size,
                             const uint8_t *kf_bad, const int32_t *point_ids, int np, const int32_t *ref_kf, const int32_t *obs_point,
                             const int32_t *obs_kf, const int32_t *obs_idx, int ne, const afv_refresh_params *params, afv_refresh_out *out);

/* ---- Essential graph: Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:771-1031, as LoopClosing::CorrectLoop calls it at
 * LoopClosing.cc:581) over plain arrays and the map-point store, and the point correction of CorrectLoop (LoopClosing.cc:487-516) as a
 * call of its own.  It was the one step of a loop closure that left the device; it ends by moving every map point of the map, which
 * lives in the store.
 * The normative semantics are tests/_essgraph_ref.py (double, one rounding per operator, every operator order fixed there); the device is
 * held to it bit for bit, and so is the scalar host program tools/essgraph_host.cpp, which compiles the same text
 * (csrc/afv_essgraph_math.h).  g2o is not shipped by the reference, so what it runs (VertexSim3Expmap, EdgeSim3 with Sim3::log,
 * BaseBinaryEdge's numeric Jacobians, BlockSolver_7_3, OptimizationAlgorithmLevenberg with userLambdaInit) is restated after upstream g2o
 * as bundled with ORB-SLAM2 - parity with a real g2o is UNPINNED.
 * The problem: nk vertices in the order of the caller's keyframe list, S_init[k] = CorrectedSim3 of keyframe k or (Rcw, tcw, 1); vertex
 * `fixed` (pLoopKF) is fixed.  Edge e has the error log(edge_meas[e] * S(edge_v0[e]) * S(edge_v1[e])^-1), information I7, no robust
 * kernel, edge_v0 the vertex of setVertex(0, ...); the edges come in the order in which the reference adds them (the Python package's
 * essential_graph_edges builds that list from :835-971).  Several edges may join one pair.  One optimize(params.iterations) call (20 in the
 * reference) with lambda = params.lambda_init at iteration 0 (userLambdaInit: 1e-16), at most 10 trials per iteration.
 * Then (:979-998) S_out[k] = the estimate, Tiw_out[k] = [R | t * (1 / s)] (12 doubles, R row-major; SetPose takes the float cast), and
 * (:1000-1030) every point point_ids[i] that is set and not bad in the store and has point_ref[i] >= 0 (the position in the keyframe
 * list of mnCorrectedReference or mpRefKF) moves to float(S(ref)^-1.map(S_init(ref).map(double(P)))), map(P) = s (R P) + t; xyz_out has the
 * doubles (0 where nothing moved), the store receives the float cast when params.write_points.  Every other point and plane of the
 * store is untouched; UpdateNormalAndDepth of the moved points is afv_table_refresh_points.
 * The launches (csrc/k_essgraph.hip): per iteration k_ess_perturb (a lane per vertex and perturbation), k_ess_linearise (a lane per edge
 * and perturbed error), k_ess_terms (a lane per edge and term), k_ess_build (a wavefront per free vertex / per off-diagonal block),
 * k_ess_begin; per trial k_ess_load, k_ess_factor (ONE workgroup walks the block columns of L and runs both substitutions), k_ess_step,
 * k_ess_trial, k_ess_judge, then ONE wait in which the host reads the status record.  The accept / reject decision, lambda and ni are
 * the device's.  After the last iteration k_ess_recover and k_ess_correct_points.  One upload: the host builds the by-vertex order of
 * the edges, the symbolic factorisation and the update triples while it checks the arguments.  No spinning flag, no cooperative
 * launch, no captured graph, no atomics.
 * Deliberate deviations from upstream (the numbering of tests/_essgraph_ref.py, where the full text is):
 *   G1  the system is block-sparse in 7 x 7 blocks over the free vertices in the order of the caller's keyframe list, factorised by an
 *       unpivoted block L L^T on the symbolic fill of that order, block column by block column, every entry subtracting its products in
 *       ascending order; forward substitution ascending, back substitution descending; a pivot that is not positive and finite is a
 *       failed trial; a vertex without edges stays in the system (the reference: Eigen's sparse Cholesky with a fill-reducing order)
 *   G2  the state is R, t, s in double, no quaternion
 *   G3  no libm: the Horner tables of PoseOptimization for sin / cos, (1 - cos) / th^2 and (th - sin) / th^3; log by exponent split and
 *       a fixed polynomial (at most 3 ulp from math.log), acos by fdlibm's rational approximation (at most 1 ulp)
 *   G4  W^-1 t by cofactors in a fixed order, not by LU
 *   G5  an error that is not finite (theta at pi, a zero determinant) makes the trial fail; not finite at the initial estimate: nothing
 *       is evaluated, status AFV_ESS_NOT_FINITE, the outputs hold the initial estimate
 *   G6  every sum has one fixed shape: per free vertex 64 strided partial sums over its edges in list order, then p[l] += p[l + s], s =
 *       32 .. 1; per off-diagonal block its edges one after the other; chi2 and computeScale the same tree over the edge list / the unknowns
 *   G7  under fix_scale the scale column of every Jacobian is exactly zero, row 6 of every block holds lambda alone
 *   G8  no free vertex, no edge or no iteration: nothing is evaluated, status AFV_ESS_EMPTY
 *   G9  the caller lists only keyframes that are not bad; an edge from a vertex to itself is refused
 *   G10 near the identity with |sigma| >= eps, Sim3::log's B carries the "- 1" that upstream's text lacks (without it W degenerates and
 *       Levenberg stalls short of the optimum of every monocular loop)
 *   G11 the edge list of essential_graph_edges walks a keyframe's loop edges in ascending keyId (the reference's set<Keyframe> is ordered
 *       by pointer); the order of the edge list fixes the bits of the sums of G6
 * Quirk kept (G-Q1): on a graph whose chi2 is exactly 0 the zero step has rho == 0, is rejected and ends optimize().
 * The capacities: AFV_ESS_MAX_L_BLOCKS blocks of L (49 doubles each: 49 MiB at the cap) and AFV_ESS_MAX_UPDATES update triples (three
 * ints each: 24 MiB); beside them an edge costs 2.6 KB of device scratch (its 29 errors and 120 terms: 166 MiB at AFV_ESS_MAX_EDGES).
 * A keyframe order whose fill exceeds one of them answers AFV_ECAPACITY before any launch, outputs and store untouched.
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
#define AFV_ESS_MAX_KF 4096
#define AFV_ESS_MAX_EDGES 65536
#define AFV_ESS_MAX_L_BLOCKS 131072
#define AFV_ESS_MAX_UPDATES 2097152
typedef struct {
    double R[9], t[3], s;                    /* a Sim3: R row-major; map(P) = s (R P) + t */
} afv_sim3d;
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_ess_params) */
    int32_t iterations;                      /* numItEssGraphOpt: 20 */
    double lambda_init;                      /* userLambdaInit: 1e-16; > 0 */
    int32_t fix_scale;                       /* bFixScale: 0 / 1 */
    int32_t write_points;                    /* 1: the store receives (float)xyz_out (SetWorldPos); 0: it stays */
} afv_ess_params;
typedef struct {
    int32_t iterations, trials;
    double chi2_first, chi2_last, lambda;    /* the chi2 at the initial estimate and at the accepted one, the last lambda */
    int32_t l_blocks;                        /* 7 x 7 blocks of L in the given order, the diagonal ones included */
    int32_t status;                          /* AFV_ESS_* */
} afv_ess_result;
#define AFV_ESS_OK 0
#define AFV_ESS_NOT_FINITE 1         /* G5 */
#define AFV_ESS_EMPTY 2              /* G8 */
#define AFV_POINT_MOVED 0            /* point_status / status, one byte per point */
#define AFV_POINT_BAD_OR_UNSET 1
#define AFV_POINT_NO_PAIR 2          /* point_ref / pair_of_point is -1 */
/* points may be NULL when np == 0.  S_init[nk], edge_v0 / edge_v1 / edge_meas[ne], point_ids / point_ref[np] (host).  Outputs (host):
 * result[1], S_out[nk], Tiw_out[nk][12], xyz_out[np][3], point_status[np].
 * Refused before any launch, outputs and store untouched: AFV_EINVAL for a NULL argument, an unknown struct_size, nk outside 1 ..
 * AFV_ESS_MAX_KF, ne > AFV_ESS_MAX_EDGES, a negative count, iterations below 0, fix_scale / write_points other than 0 / 1, a lambda_init
 * that is not positive and finite, fixed or an edge end out of range, an edge from a vertex to itself, a measurement or an initial Sim3
 * that is not finite or has s <= 0, a store of another context, a point id outside [0, capacity) or named twice, a point_ref outside
 * [-1, nk); AFV_ECAPACITY for a fill beyond AFV_ESS_MAX_L_BLOCKS or AFV_ESS_MAX_UPDATES. */
int afv_essential_graph(afv_ctx *ctx, afv_points *points, const afv_sim3d *S_init, int nk, int fixed, const int32_t *edge_v0, const int32_t *edge_v1,
                        const afv_sim3d *edge_meas, int ne, const afv_ess_params *params, const int32_t *point_ids, const int32_t *point_ref, int np,
                        afv_ess_result *result, afv_sim3d *S_out, double *Tiw_out, double *xyz_out, uint8_t *point_status);
/* The point correction alone (LoopClosing.cc:487-516: CorrectedSwi.map(Siw.map(P)) over the points of the current keyframe's
 * neighbours): point ids[i] moves to float(S_to[q].map(S_from[q].map(double(P)))) with q = pair_of_point[i], in the store, in place;
 * status[i] is AFV_POINT_MOVED, AFV_POINT_BAD_OR_UNSET or AFV_POINT_NO_PAIR (q == -1).  The same kernel as afv_essential_graph's last
 * launch.  One upload, one launch, one wait.  Refused before any launch, the store untouched: AFV_EINVAL for a NULL argument, n < 0, m
 * outside 0 .. AFV_ESS_MAX_KF, an id outside [0, capacity) or named twice, a pair outside [-1, m), a Sim3 that is not finite or has s <= 0. */
int afv_points_correct_sim3(afv_points *points, const int32_t *ids, int n, const int32_t *pair_of_point, const afv_sim3d *S_from, const afv_sim3d *S_to,
                            int m, uint8_t *status);

/* ---- Initializer: monocular start-up between two resident frames (src/Initializer.cc:41-908, as Tracking::MonocularInitialization calls
 * it, src/Tracking.cc:487).  One synchronous call does what Initializer::Initialize does, from matches12 (what
 * afv_frame_match_initialization answers) to (R21, t21, vP3D, vbTriangulated): one upload, three launches on the context's stream, one
 * wait (csrc/k_init.hip: k_init_prepare - ordered compaction of the matches, Normalize of both frames over ALL their keypoints, the
 * 8-sets of every iteration; k_init_hypotheses - one wavefront per (model, iteration): ComputeH21 / ComputeF21, de-normalisation,
 * CheckHomography / CheckFundamental over all N matches; k_init_reconstruct - selection, RH, the 8 motion hypotheses of ReconstructH or
 * the 4 of ReconstructF, CheckRT with one or two wavefronts per motion hypothesis, the accept / reject rules).  Only the mvKeysUn planes of the
 * two frames are read: frames of every descriptor kind and width are accepted.
 * The normative semantics are tests/_init_ref.py; the device is held to it bit for bit - parity with a build of the reference is
 * unpinned (it uses Eigen::JacobiSVD<float> and its own random generator).  Float arithmetic, one rounding per operator, a three-term
 * sum as a0 + (a1 + a2), other scalar expressions left to right as written, A * B * C = (A * B) * C, det3 / inv3 by cofactors.
 * Quirks restated as written: CheckFundamental gates on 3.841 and scores with 5.991; CheckRT counts in nGood (and writes p3d for) points
 * that fail cosParallax < minCos while isGood stays false; ReconstructF's else-if chain tests only the first hypothesis equal to
 * maxGood; RH is NaN when both scores are 0 and goes to ReconstructF; ReconstructF counts inliers in a float, ReconstructH in an int.
 * Deliberate deviations:
 *   I1  the DLT null vector: M = A^T A in double (running sums over the rows), a cyclic Jacobi on the symmetric 9 x 9 in double, pairs
 *       (0,1) (0,2) .. (7,8), + - * / sqrt only, at most 30 sweeps, the skip and stop rules and the rotation of S2; the column of V of the
 *       smallest diagonal entry (ties: lowest index), rounded to float.  It replaces Eigen::JacobiSVD
 *   I2  svd3 (the rank-2 step, DecomposeE, ReconstructH): V from the same Jacobi on the 3 x 3 A^T A, columns ordered by descending
 *       eigenvalue (for i in 0, 1: for k in i + 1 .. 2: swap when d_i < d_k); b_k = A v_k, w_k = |b_k|, u_0 = b_0 / w_0, u_1 = b_1 / w_1,
 *       u_2 = u_0 x u_1, v_2 negated when b_2 . u_2 < 0; all in double, then rounded to float
 *   I3  ReconstructH negates A = K^-1 H21 K when det3(A) < 0: the sign of H21 reaches no output (that of F21 does not either: I2)
 *   I4  draws: key_h = sm(sm(seed) ^ (h + 1)), draw d in 0..7 = sm(key_h + (d + 1) * 0xD1342543DE82EF95) % (N - d), applied to
 *       availableIndices with the reference's swap-with-back (:83-89); H and F share the sets
 *   I5  fixed-shape sums.  Normalize: 256 partial sums (partial t adds elements t, t + 256, .. in ascending order), then p[t] += p[t + s]
 *       for s = 128 .. 1.  The scores: a match contributes e = c1 + c2 (c = th - chiSquare where the gate passes, else 0), 64 partial
 *       sums over the matches l, l + 64, .., the same halving tree from s = 32
 *   I6  no acosf: parallax > / >= minParallax is cos < / <= float(cos(1 degree)) on the min(50, n - 1)-th smallest cosine; nGood == 0
 *       reads cosine 1, ReconstructH's initial bestParallax = -1 reads cosine 2.  The trace carries cosines
 *   I7  N < 8: nothing is evaluated, ok = 0, reason AFV_INIT_TOO_FEW_MATCHES, every per-hypothesis output reads 0
 *   I8  a hypothesis is degenerate when the second-smallest diagonal entry of the converged 9 x 9 is <= 1e-12 times the largest (repeated
 *       or collinear points), or an entry of H21, H12 or F21 is not finite: it scores 0, is flagged, its model record and inlier words
 *       read 0.  A match whose chiSquare is not finite fails that gate and contributes 0
 *   I9  no hypothesis of a model scores above 0: the model is all zeros with no inliers, its winning index is -1
 *   I10 CheckRT skips a point with x3Dh(3) == 0 or a cosParallax that is not finite like a point that is not finite
 *   I11 on ok = 0, R21, t21, p3d and triangulated read 0; on ok = 1 the p3d rows CheckRT did not write read 0
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_init_job) */
    int32_t iterations;                      /* maxIterations, 1 .. AFV_INIT_MAX_ITERATIONS */
    uint32_t seed_lo, seed_hi;               /* the 64-bit seed of I4 */
    float fx, fy, cx, cy;                    /* K of the reference frame */
    float sigma;                             /* sigmaInitializer */
} afv_init_job;
#define AFV_INIT_MAX_ITERATIONS 1024
#define AFV_INIT_MAX_MOTIONS 8
#define AFV_INIT_MAX_MASK_WORDS 256 /* mask_words 0 .. 256: the largest frame (8192 features) needs 256 */
enum { AFV_INIT_ROUTE_H = 0, AFV_INIT_ROUTE_F = 1 };
enum { AFV_INIT_OK = 0, AFV_INIT_TOO_FEW_MATCHES, AFV_INIT_D_RATIO, AFV_INIT_AMBIGUOUS, AFV_INIT_PARALLAX, AFV_INIT_MIN_TRIANGULATED,
       AFV_INIT_MIN_GOOD };
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_init_trace), set by the caller */
    int32_t n;                               /* N, the number of matches */
    float sh, sf, rh;                        /* SH, SF, RH = SH / (SH + SF) */
    int32_t best_h, best_f;                  /* the winning iteration of each model, -1 = none (I9) */
    float h21[9], f21[9];                    /* the winning models, row-major */
    int32_t route;                           /* AFV_INIT_ROUTE_H / _F: which reconstruction ran */
    int32_t n_inliers;                       /* inliers of that model */
    int32_t n_motion;                        /* motion hypotheses built: 8, 4, or 0 (N < 8, dRatio) */
    int32_t best_motion;                     /* the accepted one, -1 = none */
    int32_t reason;                          /* AFV_INIT_OK or why the answer is false */
    int32_t n_good[AFV_INIT_MAX_MOTIONS];    /* CheckRT's nGood */
    float cos_parallax[AFV_INIT_MAX_MOTIONS]; /* the selected cosine (I6) */
    float R[AFV_INIT_MAX_MOTIONS][9], t[AFV_INIT_MAX_MOTIONS][3];
    float T1[9], T2[9];                      /* Normalize's T of both frames */
} afv_init_trace;
/* f1 = the reference frame (N1 = its feature count), f2 = the current frame (N2); matches12[N1] = feature of f2 | -1.  Outputs (host):
 * *ok, *route, R21[9] row-major, t21[3], p3d[N1][3], triangulated[N1]; optional: trace, hyp_score[2][iterations] (0 = H, 1 = F),
 * hyp_model[2][iterations][9], hyp_degenerate[2][iterations], hyp_inliers[2][iterations][mask_words] (bit k of a row = match k in
 * ascending i1, unused bits 0).
 * Refused before any launch, nothing written: AFV_EINVAL for NULL f1 / f2 / job / ok / route / R21 / t21, NULL matches12 / p3d /
 * triangulated when N1 > 0, frames of different contexts or without features (a distorted frame without afv_frame_set_undistorted),
 * iterations out of range, an unknown struct_size (job or trace), a matches12[i] outside [-1, N2), sigma, fx or fy not finite or
 * <= 0, cx or cy not finite, mask_words outside 0 .. AFV_INIT_MAX_MASK_WORDS, mask_words * 32 < N when hyp_inliers is given. */
int afv_frame_initializer(afv_frame *f1, afv_frame *f2, const afv_init_job *job, const int32_t *matches12, int32_t *ok, int32_t *route,
                          float *R21, float *t21, float *p3d, uint8_t *triangulated, afv_init_trace *trace, float *hyp_score,
                          float *hyp_model, uint8_t *hyp_degenerate, uint32_t *hyp_inliers, int mask_words);

/* ---- PnPsolver: all EPnP RANSAC hypotheses of a relocalisation at once (src/PnPsolver.cc:67-950, as Tracking::Relocalization uses it,
 * src/Tracking.cc:1190-1216).  Per candidate keyframe the constructor (the filter over vpMapPointMatches, mvP2D, mvP3Dw, mvMaxError,
 * mRansacMinInliers), EVERY hypothesis h < nhyp (four draws, EPnP on them, CheckInliers over all N correspondences) and the Refine of
 * every RECORD run on the device: one upload, three launches and ONE wait per call whatever the number of candidates (csrc/k_pnp.hip:
 * k_pnp_gather, one workgroup per candidate; k_pnp_hypotheses and k_pnp_refine, one wavefront per (candidate, hypothesis)).
 * Hypothesis h depends on (seed, h) alone.  Refine reads only mvbBestInliers, which changes only at a record: h is a record when
 * count[h] >= min_inliers and count[h] > count[g] for every g < h.  A Refine called at a later hypothesis that is no record repeats the
 * last record's computation, so the device evaluates it once per record and PnPsolver::iterate is a scan over count[] that the host does
 * exactly (afv::PnPsolver of the adapter, PnPsolver of the Python package): at a hypothesis with count >= min_inliers it answers the refined pose of the current record
 * when that record's refined count is > min_inliers.
 * It reads the frame's mvKeysUn and sigma2 planes, XYZ and the flags of the store and the intrinsics given with afv_frame_set_pose.
 * The normative semantics are tests/_pnp_ref.py; the device is held to it bit for bit - parity with a build of the reference is
 * unpinned (it links OpenCV's legacy cvSVD / cvSolve / cvInvert).  EPnP runs in double, one rounding per operator, scalar expressions
 * left to right as written.
 * Quirks restated as written:
 *   Q1  the `||` of iterate's loop condition: a call runs until mnIterations >= mRansacMaxIts AND its own count >= nIterations (host)
 *   Q2  pow(epsilon, 3) with a minimal set of 4 (host)
 *   Q3  the best is updated on >, the early answer is given on refined count > min_inliers, the final answer on best >= min_inliers: it
 *       is the UNREFINED best pose (host)
 *   Q4  Refine runs at every qualifying hypothesis, on the best set so far, not on the current one
 *   Q5  CheckInliers: Xc, Yc, invZc are floats of double expressions, ue / ve double, distX / distY / error2 float, error2 < mvMaxError[i]
 *   Q6  solve_for_sign looks at the first selected correspondence only
 * Deliberate deviations:
 *   E1  eigenvectors of M^T M: the cyclic Jacobi of S2 / I1 on the symmetric 12 x 12 in double, pairs (0,1) (0,2) .. (10,11), + - * /
 *       sqrt only, the same skip and stop rules, at most 30 sweeps (the scenes of tests/_pnp_scenes.py need at most 10); the columns
 *       ordered by descending diagonal entry, ties to the lowest index; ut row k = column k; signs as the Jacobi leaves them
 *   E2  PCA of the points: the same Jacobi on the 3 x 3, descending order
 *   E3  cvInvert(CC, CV_SVD): the inverse by cofactors in double (the layout of the Initializer's inv3)
 *   E4  the three cvSolve(CV_SVD) least-squares systems go through the file's own qr_solve (:860-950), restated as written
 *   E5  estimate_R_and_t's SVD of ABt: the I2 construction in double: V from the Jacobi on A^T A, u_k = A v_k / |A v_k| for k = 0, 1,
 *       u_2 = u_0 x u_1, v_2 negated when (A v_2) . u_2 < 0; R = U V^T, then the reference's det < 0 fix
 *   E6  draws: key_h = sm(sm(seed) ^ (h + 1)), draw d in 0..3 = sm(key_h + (d + 1) * 0xD1342543DE82EF95) % (N - d), applied to
 *       vAvailableIndices with the reference's swap-with-back (:188-201)
 *   E7  every sum over the selected correspondences (centroid, PW0^T PW0, M^T M, pc0 / pw0, ABt, the reprojection error) has a fixed
 *       shape: 64 partial sums (partial l starts at 0 and adds the selected elements l, l + 64, .. in ascending order), then
 *       p[l] += p[l + s] for s = 32 .. 1
 *   E8  a hypothesis or a refinement is degenerate when qr_solve meets eta == 0 (the reference returns with X unwritten), a betas[0] it
 *       divides by is 0, or an entry of R or t of the chosen approximation is not finite: it counts 0 inliers, is flagged, its pose and
 *       words read 0.  A reprojection error that is not finite loses the comparison of the three approximations; a correspondence whose
 *       error2 is not finite is not an inlier.  A coplanar or collinear 4-set has no rule of its own (the reference has no rank test):
 *       CC is singular or nearly so and the pose is what the arithmetic gives, or not finite and then degenerate by this clause
 *       (the first two clauses are tested at the functions that raise them only: no 4-set of finite points is known that reaches them
 *       through EPnP - control points that coincide exactly make the barycentric coordinates NaN first, which is the third clause)
 *   E9  N < 4 evaluates nothing: all counts 0, no flag
 *   E10 what is not written reads 0; the refined rows of a hypothesis that is not a record read 0 with refined = 0
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
typedef struct {
    uint32_t struct_size;                    /* sizeof(afv_pnp_job) */
    uint32_t seed_lo, seed_hi;               /* the 64-bit seed of E6 */
    int32_t min_inliers;                     /* minInliers of SetRansacParameters, >= 4 */
    float epsilon, th2;                      /* epsilon and th2 of SetRansacParameters */
} afv_pnp_job;
#define AFV_PNP_MAX_CANDIDATES 64
#define AFV_PNP_MAX_HYPOTHESES 1024
#define AFV_PNP_MAX_MASK_WORDS 256 /* mask_words 0 .. 256: the largest frame (8192 features) needs 256 */
/* nc 1 .. AFV_PNP_MAX_CANDIDATES candidates of the frame f (NF = its feature count): pts[nc][NF] = the map-point id matched to feature
 * i for candidate c (what afv_table_match_bow_frame answers, mapped to point ids), -1 = none.  A feature is kept when its id is >= 0,
 * was set in the store and is not bad (an id that was never set counts as bad); the survivors keep the feature order.  Outputs (host):
 * n[nc] = N; min_inliers[nc] = mRansacMinInliers = max(int(N * epsilon), job.min_inliers, 4), the product in float; index[nc][NF] =
 * mvKeyPointIndices (-1 from N on); count / degenerate [nc][nhyp]; pose[nc][nhyp][12] = Rcw row-major, tcw, converted to float; inliers
 * [nc][nhyp][mask_words], bit k of the row = correspondence k, unused bits 0; refined[nc][nhyp]: 0 = h is no record, 1 = refined, 2 =
 * a record whose refinement is degenerate; refined_count / refined_pose / refined_inliers as count / pose / inliers; optional max_err
 * [nc][NF] (mvMaxError = sigma2 * th2 in float) and p3dw[nc][NF][3] (mvP3Dw), 0 from N on.
 * Refused before any launch, nothing written: AFV_EINVAL for a NULL argument other than max_err / p3dw, a frame without features or
 * without a pose (afv_frame_set_pose: the intrinsics are the frame's), a store of another context, an id outside [-1, capacity), nc,
 * nhyp or mask_words out of range, mask_words * 32 below the largest number of ids >= 0 in a row, an unknown struct_size, min_inliers
 * < 4, epsilon or th2 not finite or <= 0.  The descriptor kind and width of frame and store do not matter: descriptors are not read. */
int afv_frame_pnp_hypotheses(afv_frame *f, afv_points *points, const afv_pnp_job *jobs, int nc, const int32_t *pts, int nhyp, int mask_words,
                             int32_t *n, int32_t *min_inliers, int32_t *index, int32_t *count, uint8_t *degenerate, float *pose,
                             uint32_t *inliers, uint8_t *refined, int32_t *refined_count, float *refined_pose, uint32_t *refined_inliers,
                             float *max_err, float *p3dw);

/* engine of the ordered phase of the projection searches / SearchForInitialization (identical results):
 *   1: one fixed point over all live queries of a job on a 1024-thread workgroup (round 5)   0: the ordered walk of rounds 1-4 on one
 *   wavefront   2 (default): 1 whenever the job's tables fit the workgroup's LDS, else 0   3: as 1, but ranking and ordered phase as two
 *   launches even for a single job on a resident frame (by default those run in ONE launch: the last ranking workgroup goes on as the
 *   fixed-point workgroup) */
int afv_set_projection_resolve(afv_ctx *ctx, int engine);

/* ---- place recognition: BowVectors and DBoW2 L1 scores (the arithmetic under KeyFrameDatabase::DetectLoopCandidates /
 * DetectRelocalizationCandidates, src/KeyFrameDatabase.cc:76-309, Vocabulary::score, src/Vocabulary.cpp:132-153, and the minScore loop of
 * LoopClosing.cc:137-157).  DBoW2 is an empty submodule in the reference: BowVector::addWeight / normalize(L1) and L1Scoring::score follow
 * upstream DBoW2 - parity unpinned.  New symbols and records only: AFV_ABI_VERSION stays 6. ----
 *
 * Word weights of a (binary or float) vocabulary, by DBoW2 node id: weight[nnodes] (TF-IDF node weights, read at the leaves) and
 * word_id[nnodes] (-1 for inner nodes).  With weights set, afv_frame_bow_transform also builds the frame's BowVector on the device and
 * afv_bow_vector works; weight == NULL removes them.  A vocabulary without weights behaves as before everywhere. */
int afv_vocab_set_weights(afv_ctx *ctx, afv_vocab *v, const double *weight, const int32_t *word_id);
/* DBoW2 transform's BowVector from the leaves afv_bow_transform[_f32] returned (n <= 8192): a feature whose leaf weight is not > 0 adds
 * nothing; value[w] grows by one addition of weight[w] per feature; norm = sum of fabs(value) in ascending word order; every value is
 * divided by it when norm > 0.  Entries ascending by word id; word / value hold up to n entries.  IEEE double throughout. */
int afv_bow_vector(afv_ctx *ctx, const afv_vocab *v, const int32_t *leaf_node, int n, int32_t *word, double *value, int32_t *n_out);
/* the BowVector afv_frame_bow_transform built (vocabulary with weights; AFV_EINVAL otherwise): up to the frame's cap entries */
int afv_frame_get_bowvec(afv_frame *f, int32_t *word, double *value, int32_t *n_out);
/* BowVector of keyframe `slot` from host arrays: ascending, unique word ids >= 0, n <= cap (else AFV_EINVAL).  afv_table_set on the slot
 * forgets it; afv_table_set_from_frame brings the frame's along; afv_table_clone / afv_table_broadcast ship it. */
int afv_table_set_bowvec(afv_table *t, int slot, const int32_t *word, const double *value, int n);

#define AFV_BOW_QUERY_SLOT 0  /* the BowVector of table slot `slot` (LoopClosing) */
#define AFV_BOW_QUERY_FRAME 1 /* the BowVector of resident frame `frame` (relocalisation: nothing is uploaded) */
#define AFV_BOW_QUERY_HOST 2  /* host arrays word[n] (ascending, unique) / value[n], n <= 8192 */
typedef struct afv_bow_query {
    uint32_t struct_size; /* sizeof(afv_bow_query) of the caller's build */
    int32_t kind;
    int32_t slot;
    int32_t n;
    afv_frame *frame;
    const int32_t *word;
    const double *value;
} afv_bow_query;
/* nq queries against the slots of the table in ONE launch.  slot_mask[nsets] != NULL: only slots with a non-zero byte (naming a slot that
 * holds features but no BowVector is AFV_EINVAL); NULL: every slot.  Per (query, slot), row-major [nq][nsets]:
 *   common        words present in both vectors (mnLoopWords / mnRelocWords); -1 for an empty, masked-out or BowVector-less slot
 *   first_common  the smallest shared word id, -1 when there is none (may be NULL)
 *   score         L1Scoring::score(query, slot): over the shared words in ascending order s += fabs(v - w) - fabs(v) - fabs(w) (v: query,
 *                 w: slot; left to right), result -s / 2.0; 0.0 when nothing is shared or the slot is absent
 * A query slot / frame without BowVector is AFV_EINVAL. */
int afv_table_score_bow(afv_table *t, const afv_bow_query *q, int nq, const uint8_t *slot_mask, int32_t *common, double *score,
                        int32_t *first_common);

/* ---- vocabulary training on the device: DBoW2 TemplatedVocabulary::create for binary descriptors (the trainer the reference ships as
 * createVocabulary.py -> src/createVocabulary.cpp: loadBinaryFeatures :122-179, voc.create(features) :292-301, k / L at :50-51, TF_IDF and
 * L1_NORM at :52-53).  DBoW2 is an empty submodule in the reference: HKmeansStep, initiateClustersKMpp, createWords, setNodeWeights and
 * FORB::meanValue / distance are restated from upstream DBoW2 - parity unpinned.  tests/_voctrain_ref.py is the normative restatement; every
 * quantity is an integer, the device is held to bit equality with it.  Two deliberate differences from upstream:
 *   - a cluster that ends an association round empty KEEPS its previous centre (upstream releases it and the next distance reads an empty
 *     matrix);
 *   - the seeding draws come from a counter-based generator instead of rand(): sm = splitmix64, key(root) = sm(seed), key(child at cluster
 *     position i) = sm(key(parent) ^ (i + 1)); first centre sm(key) % n, draw j: cut = 1 + sm(key + j * 0xD1342543DE82EF95) % dist_sum -
 *     a pure function of (seed, path, draw), so all nodes of a level train at once.
 * Weights: TF-IDF, log(nimages / Ni) in double on the host, Ni = images with a feature whose descent (afv_bow_transform's) ends in the word;
 * Ni == 0 leaves 0.0.  Float vocabularies, the other weighting / scoring enums and the C++ adapter are out of scope.
 * New symbols and records only: AFV_ABI_VERSION stays 6. ---- */
#define AFV_VOCAB_TRAIN_MAX_ROWS (1 << 26) /* the largest n afv_vocab_train[_device] takes */
typedef struct afv_vocab_train_params {
    uint32_t struct_size;        /* sizeof(afv_vocab_train_params) of the caller's build */
    int32_t k;                   /* branching factor, 2..32 */
    int32_t L;                   /* depth levels, 1..10 */
    int32_t desc_bytes;          /* 1..64 */
    uint64_t seed;
    int32_t max_iters;           /* cap on the associate / mean rounds of a node; 0 = unlimited (upstream) */
    int32_t n_init;              /* rows of init_centres, 1..k (0 with init_centres == NULL) */
    const uint8_t *init_centres; /* host rows [n_init][desc_bytes] replacing the seeding of the ROOT only (ignored when n <= k); NULL = seed */
} afv_vocab_train_params;
typedef struct afv_vocab_tree afv_vocab_tree;
/* desc: host rows [n][desc_bytes] in image order then feature order; image_ptr[nimages + 1] (image_ptr[0] == 0, non-decreasing,
 * image_ptr[nimages] == n; empty images are legal).  AFV_EINVAL, before any launch and with *out == NULL, for k outside 2..32, L outside
 * 1..10, desc_bytes outside 1..64, n < 1 or n > AFV_VOCAB_TRAIN_MAX_ROWS, nimages < 1, an inconsistent image_ptr, n_init outside 1..k. */
int afv_vocab_train(afv_ctx *ctx, const afv_vocab_train_params *params, const uint8_t *desc, int64_t n, const int32_t *image_ptr, int nimages,
                    afv_vocab_tree **out);
/* the same over a device array: row i at d_desc + i * pitch_bytes (pitch_bytes >= desc_bytes), e.g. what afv_orb_extract_batch_device left
 * behind, compacted.  The work that produced the rows must have completed.  image_ptr stays on the host. */
int afv_vocab_train_device(afv_ctx *ctx, const afv_vocab_train_params *params, const uint8_t *d_desc, size_t pitch_bytes, int64_t n,
                           const int32_t *image_ptr, int nimages, afv_vocab_tree **out);
int afv_vocab_tree_nnodes(const afv_vocab_tree *t); /* nodes in DBoW2 id order, node 0 = the root */
/* per node, any pointer may be NULL: parent[nnodes] (0 for the root), desc[nnodes][desc_bytes] (zeros for the root), is_leaf[nnodes],
 * weight[nnodes] (0.0 for inner nodes), ni[nnodes] (-1 for inner nodes) */
int afv_vocab_tree_get(const afv_vocab_tree *t, int32_t *parent, uint8_t *desc, uint8_t *is_leaf, double *weight, int32_t *ni);
/* per level (L entries each, any pointer may be NULL): association rounds run (the most any node of the level took; 0: only trivial
 * nodes or none), rows of the level's non-trivial nodes, host seconds spent; *capped: some node stopped at max_iters unconverged */
int afv_vocab_tree_stats(const afv_vocab_tree *t, int32_t *rounds, int64_t *rows, double *seconds, int32_t *capped);
void afv_vocab_tree_destroy(afv_vocab_tree *t);

/* DescriptorDistance_orb32 on the host (utility for adapters / tests) */
int afv_hamming256(const uint8_t *a, const uint8_t *b);

/* ---- live stage timing: when enabled, every afv_orb_extract_batch_device / afv_match_bruteforce_pairs_device / afv_table_match_pairs* call
 * brackets each kernel stage with hipEvents recorded on the stream the kernels are launched on.
 * afv_profile_read waits for the recorded events and returns, per stage, the number of launches and the summed
 * duration in milliseconds since the last afv_profile_enable(ctx, 1).  Stages: ---- */
enum { AFV_STAGE_PYRAMID = 0, AFV_STAGE_FAST_NMS = 1 /* k_fast_nms */, AFV_STAGE_SELECT = 2, AFV_STAGE_DESCRIBE = 3,
       AFV_STAGE_MATCH = 4 /* k_match_topk: the xor + popcount phase */, AFV_STAGE_MATCH_RESOLVE = 5 /* ordered greedy resolve */,
       AFV_STAGE_HARRIS = 6 /* k_retain_score + k_harris: retainBest on the score, Harris response of the survivors */,
       AFV_NUM_STAGES = 7 };
/* The stage list grows between releases: size the arrays passed to afv_profile_read with afv_num_stages() (or with the AFV_NUM_STAGES
 * of the header the caller was compiled against, after checking that afv_num_stages() is not larger). */
int afv_num_stages(void);
int afv_profile_enable(afv_ctx *ctx, int enable); /* 0 = off; n >= 1 = time the stages of every n-th extraction / pair-match call
                                                     * (1 = every call; the event pairs cost ~3 % of a batch step, sampling keeps that
                                                     * out of a timed run); resets the accumulated figures */
int afv_profile_read(afv_ctx *ctx, int32_t *launches /*[afv_num_stages()]*/, float *total_ms /*[afv_num_stages()]*/,
                     int64_t *units /*[afv_num_stages()], frames (pairs for MATCH) covered by those launches; may be NULL*/);
/* batches of at least `min_frames` frames (pairs) are split over the context's two streams so that latency-bound kernels of
 * one half overlap the VALU-bound ones of the other (default 64; 0x7fffffff disables the split) */
int afv_set_split_threshold(afv_ctx *ctx, int min_frames);
int afv_set_split_chunks(afv_ctx *ctx, int chunks); /* ... into this many chunks alternating over the two streams (2..64; 0 = automatic,
                                                      * chunks of about 85 frames: the default) */
/* How the chunks of a split call meet on the two streams; identical results either way.
 *   1 (default): extraction - the first part of the batch on the caller's stream, the rest on the second; each stream builds the
 *      pyramid of its whole part first (one launch per level), then runs its share of the chunks; the caller's stream carries slightly
 *      more frames, so that it ends last and runs on into the caller's next call without waiting for a hand-off.  Pair matcher - a call
 *      of up to 4096 pairs stays on the caller's stream, one top-k and one resolve launch (larger calls are split as under 0).
 *   0: chunk k, pyramid included, on stream k % 2, the pair matcher split the same way (the schedule of earlier releases, kept for A/B runs) */
int afv_set_split_schedule(afv_ctx *ctx, int mode);
/* afv_match_l2_pairs_device processes its jobs in launches of at most `pairs` jobs (default 2048; the key scratch of a launch is
 * pairs x cap x 32 bytes and is reused by the next launch on the same stream) */
int afv_set_l2_chunk_pairs(afv_ctx *ctx, int pairs);
/* Phase 2 of the brute-force pair matchers (the ordered greedy assignment of SearchByBoW, FeatureMatcher.cc:587-641); identical results:
 *   1: one fixed point over all live rows of a pair, a thread per row, claims in rotating LDS arrays (one barrier per pass): half the
 *      latency of a pair, more total work
 *   0: the ordered walk of rounds 2-3: one wavefront, 64 rows per round: what a batch that fills the chip runs fastest with
 *   2 (default): 1 for calls of at most 256 pairs (every pair then has a CU to itself), else 0 */
int afv_set_match_resolve(afv_ctx *ctx, int engine);
/* The small-batch ("latency") path.  Tracking extracts ONE frame per call (src/Frame.cc:186 -> src/FeatureExtractor.cpp:111-121) and
 * matches it against ONE other frame: at that size the batch kernels are a chain of dependent launches, each a few microseconds of
 * ramp and cache boundary around a fraction of a microsecond of work.  Calls of at most `max_frames` frames / pairs (default 4) run
 * kernels shaped for that case instead - the whole pyramid in one launch, retainBest + Harris in one launch, a quadtree workgroup of
 * 1024 threads, the brute-force distance phase split over column slices - with bit-identical results.
 *   mode 0 = never, 1 = calls of at most max_frames frames (default), 2 = always (parity tests); max_frames 0 keeps the current value */
int afv_set_small_batch_path(afv_ctx *ctx, int mode, int max_frames);
/* Phase 1 of the brute-force pair matchers (afv_match_bruteforce_pairs_device, afv_table_match_pairs*, plain SearchByBoW jobs without
 * a FeatureVector): every row's four nearest columns.  Both engines produce identical keys, hence identical match vectors.
 *   AFV_MATCH_ENGINE_MFMA (default): Hamming distance as an exact i8 x i8 -> i32 contraction on the matrix cores
 *   AFV_MATCH_ENGINE_POPCOUNT:       8 xor + 8 v_bcnt per descriptor pair on the vector ALU */
enum { AFV_MATCH_ENGINE_POPCOUNT = 0, AFV_MATCH_ENGINE_MFMA = 1 };
int afv_set_match_engine(afv_ctx *ctx, int engine);
/* afv_orb_extract_batch pipelines H2D / compute / D2H over chunks of `frames` frames with the uploads `chunks_ahead` chunks ahead of
 * the compute (defaults 64 and 8; batches below two chunks run as one) */
int afv_set_pipeline_chunk(afv_ctx *ctx, int frames, int chunks_ahead);

/* ---- stage-level introspection of the LAST afv_orb_extract* call (parity tests / profiling) ---- */
typedef struct {
    int32_t nlevels, width, height;
    int32_t lw[AFV_MAX_LEVELS], lh[AFV_MAX_LEVELS];
    float lscale[AFV_MAX_LEVELS];
    int32_t quota[AFV_MAX_LEVELS];    /* mnFeaturesPerLevel */
    int32_t cv_quota[AFV_MAX_LEVELS]; /* cv::ORB nfeaturesPerLevel for nfeatures*10 */
    int32_t cand_cap[AFV_MAX_LEVELS];
} afv_geometry;
int afv_get_geometry(const afv_ctx *ctx, afv_geometry *g);
/* copy pyramid level `level` of frame `frame` to host (tightly packed lw x lh) */
int afv_debug_get_level(afv_ctx *ctx, int frame, int level, uint8_t *out);
/* FAST+NMS candidates of (frame, level), unordered: packed[i] = x | y<<12 | score<<24, response[i] = Harris */
int afv_debug_get_candidates(afv_ctx *ctx, int frame, int level, uint32_t *packed, float *response, int cap, int *n_out);
/* keypoints chosen by the quadtree for (frame, level) in list order: x,y level coordinates */
int afv_debug_get_selected(afv_ctx *ctx, int frame, int level, int32_t *x, int32_t *y, float *response, int cap, int *n_out);
/* standalone 7x7 Gaussian blur of a level (E9) — same arithmetic as the fused describe kernel */
int afv_debug_blur_level(afv_ctx *ctx, int frame, int level, uint8_t *out);
/* host-only (no device, no context): the work plan of the one-launch pyramid for a geometry - per level and per tile index of the top
 * level the (need.lo, need.hi, own.lo, own.hi) ranges in x (first [nlevels][ntx] quadruples) and y ([nlevels][nty]), the resize
 * coefficient tables (pairs (source offset, weight of the right tap) per level: x then y, levels 1..) and, in info[4 + 6 * 8]:
 * nlevels, ntx, nty, LDS bytes, then per level w, h, LDS pitch, log2 dword slots per row, x-table offset, y-table offset (in pairs).
 * tests/test_host_logic.py replays the kernel's data flow on the CPU from exactly these numbers. */
int afv_debug_pyramid_plan(const afv_orb_params *params, int width, int height, int tile_w, int tile_h, int16_t *regions,
                           int regions_cap, int32_t *info, int16_t *tables, int tables_cap);

/* host-only (no device, no context): what the FAST kernel decides per tile of a frame of the given geometry - per 64 x 32 tile, in the order
 * of the flat tile index, 12 ints: level, tile column, tile row, the rectangle of pixels FAST can report (3 <= x < w - 3, 3 <= y < h - 3) in tile
 * coordinates x0, y0, x1, y1 (exclusive ends), 1 if the tile holds none and its workgroup leaves at once, the last score row that matters, the
 * last pre-test row group, the wavefronts (bit mask) that skip the pre-test, the wavefronts that skip the NMS.  level_wh[2 * AFV_MAX_LEVELS]:
 * w, h per level.  tests/test_fast_ragged_cpu.py holds these decisions to rectangles it computes itself. */
int afv_debug_fast_tiles(const afv_orb_params *params, int width, int height, int32_t *tiles, int tiles_cap, int32_t *level_wh, int *n_out);

/* host-only (no device, no context): what the describe kernel stages and row-filters of a keypoint's 43 x 43 patch - the tables it was compiled
 * with.  R[37 * 37]: 1 where a rotated BRIEF test can land, [iy + 18][ix + 18].  Per patch alignment a = 0..3 (first patch column & 3):
 * items[a][192] = pair-row << 8 | group of four plane columns, in schedule order (wave step = index / 64, lane = index % 64);
 * dwords[a][448] = patch row << 8 | dword of the LDS row, likewise; both padded with copies of their last entry.  counts[8]: items per
 * alignment, then staged dwords per alignment.  layout[8]: row-pass steps, staging steps, byte offset of the patch in a wavefront's LDS slice,
 * pitch of a patch row, bytes of a plane pair-row, slice bytes, 1 if the built kernel trims the row pass, 1 if it trims the staging.
 * tests/test_describe_reach_cpu.py holds the tables to an angle sweep of the pattern. */
int afv_debug_describe_reach(uint8_t *R, uint16_t *items, uint16_t *dwords, int32_t *counts, int32_t *layout);

/* ---- test hooks for the per-call scratch of a context (tests/test_gpu_scratch.py).  Nothing in the product calls them. ----
 * Every entry point lays its inputs, outputs and device-only scratch into grow-only buffers of its context and must not depend on what
 * an earlier call left there.  These hooks make that a property a test can check: report the buffers' sizes, fill them with a byte,
 * read them back, and read the words every call has to leave zero.
 *
 * afv_debug_scratch_bytes: out[i] for i < min(n, AFV_SCRATCH_SLOTS), in this order (the AFV_SCRATCH_* indices):
 *   0 d_match       device staging of the matcher / solver entry points (Blob)
 *   1 h_stage       its pinned host image
 *   2 d_topk        key records of the brute-force pair matcher
 *   3 d_slice       per-slice key records of the column-sliced phase 1
 *   4 d_l2_scratch  key records of the float pair matcher
 *   5 sum over the context's map-point stores of afv_points::d_stage (device staging of the setters / afv_points_get)
 *   6 sum over them of afv_points::h_pin (its pinned image)
 *   7 sum over the context's keyframe tables of the pair buffers d_pairs + d_out + d_nm (afv_table_match_pairs)
 *   8 sum over them of the pinned image h_pin of those
 * afv_debug_paint_scratch: waits for the context's stream, then fills every byte of exactly those buffers with `byte` - the device ones
 * on the context's own stream (and waits), the host ones with memset.
 * LEFT OUT, because they carry state from one call to the next by design or are not per-call scratch:
 *   d_proj_ticket, d_points_count, d_tickets   zero at rest: afv_debug_rest_words reads them
 *   the extraction working set (d_pyr, d_cand_*, d_l1*, d_hq*, d_kept_*, d_sel*, d_frames, d_out_block, d_n, d_status; sized once at
 *     afv_create / afv_set_geometry)   the afv_debug_get_* getters read the last extraction out of it, and its counters are cleared by
 *     the extraction itself; tests/test_gpu_extract*.py compare it stage by stage
 *   d_geo, d_tab, d_pf_blob   the geometry's plan, written when the geometry is set and read by every extraction
 *   the planes of frames, map-point stores and tables, a frame's pyramid and grid, a table's d_mp / d_kf_cell_*   resident data
 *   the AKAZE context (akaze_api.hip)   a context type of its own
 * afv_debug_rest_words: waits for the context's stream, copies d_proj_ticket, both words of d_points_count (once a map-point store made
 * them) and d_tickets[0, tickets_n) to the host and stores in *nonzero how many of them are not zero.
 * afv_debug_scratch_read: bytes [offset, offset + bytes) of slot `which` (0 .. 8) after a wait for the stream; a slot that stands for
 * several buffers (5 .. 8) reads as one run of bytes: the stores, then the tables, in the order they were made, per table d_pairs, d_out,
 * d_nm.  AFV_EINVAL beyond the slot's size.  All four: AFV_OK | AFV_EINVAL | AFV_EHIP. */
enum { AFV_SCRATCH_D_MATCH = 0, AFV_SCRATCH_H_STAGE = 1, AFV_SCRATCH_D_TOPK = 2, AFV_SCRATCH_D_SLICE = 3, AFV_SCRATCH_D_L2 = 4,
       AFV_SCRATCH_POINTS_STAGE = 5, AFV_SCRATCH_POINTS_PIN = 6, AFV_SCRATCH_TABLE_PAIRS = 7, AFV_SCRATCH_TABLE_PIN = 8, AFV_SCRATCH_SLOTS = 9 };
int afv_debug_scratch_bytes(afv_ctx *ctx, size_t *out, int n);
int afv_debug_paint_scratch(afv_ctx *ctx, int byte);
int afv_debug_rest_words(afv_ctx *ctx, int32_t *nonzero);
int afv_debug_scratch_read(afv_ctx *ctx, int which, size_t offset, void *out, size_t bytes);

/* ---- fusing map points into keyframes of the table: FeatureMatcher::Fuse(pKF, vpMapPoints, th) (FeatureMatcher.cc:794-940) and
 * Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:942-1064) as LocalMapping::SearchInNeighbors (LocalMapping.cc:475-555) and
 * LoopClosing::SearchAndFuse (LoopClosing.cc:601-628) run them: the points of a resident store into up to 64 table slots in one call.
 * What a slot needs next to its rows, geometry (afv_table_set_geometry) and scale planes (afv_table_set_scale): the table's camera, a pose
 * (or a pose_override in the job) and the keyframe's mvpMapPoints as a plane of point ids; with use_inf_gate its information plane
 * (afv_table_set_inf).  All of it is allocated on first use and nothing existing changes its behaviour.
 *
 * The camera of the table: the image bounds mnMinX .. mnMaxY and the grid of KeyFrame::GetFeaturesInArea (KeyFrame.cc:613-652), the
 * fields afv_frame_params carries for a frame; sizeTolerance is the context's scale factor, as for frames.  grid_cols * grid_rows <= 8192
 * (else AFV_EINVAL); a grid whose one-workgroup build does not fit the LDS: AFV_EUNSUPPORTED.  The grid of a slot is built on the device
 * by the kernel that builds a frame's (cells in ix, iy order, ascending feature index inside a cell), on demand by the fuse call, and kept
 * until the slot's geometry, scale planes or the camera change.
 * The pose of a slot: the argument rule of afv_frame_set_pose (Ow computed by the host with the reference's own expression); kept on the
 * host side of the table.  The plane: ids[n] over the slot's features, -1 = no point.  afv_table_set forgets pose and plane of its slot;
 * afv_table_clone carries both along (and the camera).
 *
 * Per (job, query), packed in job order: best (feature index | -1), occupant (the id the plane holds at best | -1) and status:
 *   0  invalid query: id -1, never set, or bad in the store
 *   1  already in the keyframe: the id occurs in the slot's plane (IsInKeyFrame / spAlreadyFound: one rule for both overloads)
 *   2  not in view: any geometric test of the AFV_PT_FUSE rule set, deviation D1 included
 *   3  no feature won: empty window, every candidate gated, or bestDist > th_low
 *   4  the winning feature is free: the host adds the observation
 *   5  the winning feature holds a point that is bad in the store (the reference counts it and does nothing)
 *   6  the winning feature holds a good point: Replace / vpReplacePoint.  An occupant id outside [0, capacity) or never set counts as
 *      good; the store is not read for it.
 * nfused[job] counts statuses 4 to 6: what the reference returns.  The geometry is AFV_PT_FUSE's with the camera of the job, the search
 * that of afv_match_fuse (one kernel text for both); use_inf_gate = 1 is Fuse no. 1 with its 5.99 / 7.8 gates, 0 is Fuse no. 2.
 * SNAPSHOT RULE: every job is answered against the store and the planes as they stand when the call is made; the call writes neither.
 * Two queries of a job may win the same free feature (both status 4); AddObservation, Replace and ComputeDistinctiveDescriptors stay
 * with the caller.  One target per call with the caller's updates in between gives the reference's loop.
 * Limits: nt 0 .. 64, nq <= 65535 per job, the nq of a call sum to at most AFV_KFFUSE_MAX_QUERIES; jobs that pass the same ids pointer
 * and nq share one descriptor gather.  Refused before any launch, outputs untouched (AFV_EINVAL unless noted): nt out of range, a slot
 * out of range, a slot without geometry, scale planes, information plane (use_inf_gate), map-point plane or pose (a pose_override replaces
 * Rcw, tcw and Ow only: the intrinsics are always those given with afv_table_set_pose), no camera, store and table on different contexts, a store of another descriptor kind or width (AFV_EUNSUPPORTED), an id outside
 * [-1, capacity), a query total beyond the cap, an unknown struct_size.
 * New symbols and records only: AFV_ABI_VERSION stays 6. */
#define AFV_KFFUSE_MAX_TARGETS 64
#define AFV_KFFUSE_MAX_QUERIES (1 << 20)
typedef struct {
    uint32_t struct_size;         /* sizeof(afv_table_camera) */
    float min_x, max_x, min_y, max_y;   /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    int32_t grid_cols, grid_rows;
    float grid_inv_w, grid_inv_h;       /* mfGridElementWidthInv, mfGridElementHeightInv */
} afv_table_camera;
typedef struct {
    float R[9], t[3], Ow[3];      /* Fuse no. 2: the decomposed Scw (sRcw / scw, Scw's translation as it stands, -Rcw^T tcw) */
} afv_table_fuse_pose;
typedef struct {
    uint32_t struct_size;         /* sizeof(afv_table_fuse_job) */
    int32_t slot;
    const int32_t *ids;           /* [nq] host: point id | -1, in the reference's iteration order */
    int32_t nq;
    float radius_th, radius_scale, th_low;
    int32_t use_inf_gate;
    const afv_table_fuse_pose *pose_override;   /* NULL: the slot's pose */
} afv_table_fuse_job;
int afv_table_set_camera(afv_table *t, const afv_table_camera *cam);
int afv_table_set_pose(afv_table *t, int slot, const float *Rcw, const float *tcw, const float *Ow, float fx, float fy, float cx, float cy,
                       float mbf);
int afv_table_set_map_points(afv_table *t, int slot, const int32_t *ids);
/* for tests: the plane of a slot, n ints.  AFV_EINVAL for a slot without a plane.  Synchronous. */
int afv_table_get_map_points(afv_table *t, int slot, int32_t *ids);
int afv_table_fuse_points(afv_table *t, afv_points *points, const afv_table_fuse_job *jobs, int nt, int32_t *best, int32_t *occupant,
                          uint8_t *status, int32_t *nfused);

#ifdef __cplusplus
}
#endif
#endif
