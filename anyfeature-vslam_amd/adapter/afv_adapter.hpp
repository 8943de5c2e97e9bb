// afv_adapter.hpp — header-only C++17 host adapter over the C-ABI (include/afv_hip.h).
//
// It mirrors the reference's plugin classes so that a host which HAS OpenCV can drop the GPU path in by compiling
// this header with -DAFV_WITH_OPENCV (then afv::KeyPoint = cv::KeyPoint, afv::Mat8 = cv::Mat) — see INTEGRATION.md for
// the subclass that plugs into Tracking.cc:1523-1552.  Without OpenCV (this repository's build container) the same
// code works on two layout-compatible PODs, which is what adapter_selftest.cpp compiles and runs.
//
// Reference interfaces mirrored (file:line in the reference tree):
//   FeatureExtractorSettings        include/FeatureExtractor.h:23-66, src/FeatureExtractor.cpp:21-56
//   FeatureExtractor::operator()    include/FeatureExtractor.h:76-93, src/FeatureExtractor.cpp:111-129
//   FeatureExtractor_orb32          include/Feature_orb32.h:12-33, src/Feature_orb32.cpp:11-65
//   FeatureMatcher::SearchByBoW x2  include/FeatureMatcher.h:59-60, src/FeatureMatcher.cc:186-283, 561-660
//   FeatureMatcher::SearchForTriangulation  include/FeatureMatcher.h:66-67, src/FeatureMatcher.cc:662-790
//   Frame (the part the front end reads)  include/Frame.h, src/Frame.cc:171-240, 333-433 -> DeviceFrame (afv_frame_*)
//   FeatureMatcher::SearchByProjection x4 / Fuse x2 / SearchBySim3 / SearchForInitialization (matching cores)
//                                   include/FeatureMatcher.h:47-82, src/FeatureMatcher.cc:73-154, 287-397, 399-557, 794-1064,
//                                   1066-1287, 1291-1506 — the projection geometry stays with the caller, as in the reference
// The reference binary is vslamlab_anyfeature_mono; the stereo branches of the matchers (FeatureMatcher.cc:114-119, 705-747, 880-894,
// 1367-1372) are served through the optional mvuRight members below, mvImagePyramid through ImagePyramid().  Frame::ComputeStereoMatches
// (Frame.cc:465-645) and Frame::ComputeStereoFromRGBD (:648-669) run on the device between resident frames that kept their pyramids:
// DeviceFrame::ComputeStereoMatches / ComputeStereoFromRGBD below (semantics and the three deviations from the reference's routine:
// include/afv_hip.h, "stereo and RGB-D frames"; parity with a build of the reference is unpinned).
// Error behaviour follows the reference: no exceptions cross the boundary; an empty image leaves the outputs
// untouched (ORBextractor.cc:570-571); an unrecoverable device error terminates (cf. Feature_sift128.cpp:61).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <array>
#include <exception>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <utility>
#include <vector>

#include <cstring>

#include "afv_akaze.h"
#include "afv_covis.h"
#include "afv_hip.h"

#ifdef AFV_WITH_OPENCV
#include <opencv2/core.hpp>
#endif

namespace afv {

#ifdef AFV_WITH_OPENCV
using KeyPoint = cv::KeyPoint;
static_assert(sizeof(cv::KeyPoint) == sizeof(afv_keypoint), "cv::KeyPoint layout changed");
#else
struct KeyPoint {  // same member order and size as cv::KeyPoint
    struct { float x, y; } pt;
    float size, angle, response;
    int octave, class_id;
};
struct Mat8 {  // minimal stand-in for a continuous CV_8UC1 cv::Mat
    int rows = 0, cols = 0;
    std::vector<uint8_t> data;
    void create(int r, int c) { rows = r; cols = c; data.assign((size_t)r * c, 0); }
    uint8_t *ptr(int r = 0) { return data.data() + (size_t)r * cols; }
    const uint8_t *ptr(int r = 0) const { return data.data() + (size_t)r * cols; }
    bool empty() const { return rows == 0 || cols == 0; }
    size_t step() const { return (size_t)cols; }
};
struct Image {  // include/Image.h:13-29: the extractor reads grayImg only
    Mat8 grayImg;
};
#endif
static_assert(sizeof(KeyPoint) == sizeof(afv_keypoint), "KeyPoint must be bit-compatible with afv_keypoint");

struct Mat2f { float m[2][2]; };  // Eigen::Matrix<float,2,2> (Types.h:139), row/column symmetric here

struct FeatureExtractorSettings {  // FeatureExtractor.h:23-66
    static inline int numOctaves0 = 8;
    static inline float scaleFactor0 = 1.2f;
    static inline float th0 = 20.0f;
    float scaleFactor = scaleFactor0;
    int nOctaves = numOctaves0;
    float detectTh = th0;
    bool ON_automaticTuning = true;
    static float GetDetectorNominalScaleFactor() { return scaleFactor0; }
    static int GetDetectorNominalNumOctaves() { return numOctaves0; }
    static float GetDetectorNominalThreshold() { return th0; }
};

[[noreturn]] inline void fatal(const char *what, int rc, afv_ctx *ctx) {
    std::fprintf(stderr, "afv: %s failed: %s (%s)\n", what, afv_strerror(rc), ctx ? afv_last_error(ctx) : "");
    std::terminate();
}

// drop-in for FeatureExtractor_orb32: same call operators, GPU behind them
class FeatureExtractor_orb32_hip {
  public:
    std::shared_ptr<FeatureExtractorSettings> settings;

    FeatureExtractor_orb32_hip(const int &nfeatures_, std::shared_ptr<FeatureExtractorSettings> &settings_, int device = 0,
                               int max_width = 640, int max_height = 480)
        : settings(settings_), nfeatures(nfeatures_) {
        afv_orb_params p;
        afv_default_orb_params(&p);
        p.nfeatures = nfeatures_;
        p.nlevels = settings->nOctaves;
        p.scale_factor = settings->scaleFactor;
        p.fast_threshold = int(settings->detectTh);  // Feature_orb32.cpp:30 setFastThreshold(int(detectTh))
        p.max_width = max_width;
        p.max_height = max_height;
        const int rc = afv_create(device, &p, &ctx);
        if (rc != AFV_OK) fatal("afv_create", rc, nullptr);
        cap = afv_max_keypoints_per_frame(ctx);
        mvScaleFactor.resize(settings->nOctaves);  // FeatureExtractor.cpp:77-85
        mvScaleFactor[0] = 1.0f;
        for (int i = 1; i < settings->nOctaves; i++) mvScaleFactor[i] = mvScaleFactor[i - 1] * settings->scaleFactor;
    }
    ~FeatureExtractor_orb32_hip() { afv_destroy(ctx); }
    FeatureExtractor_orb32_hip(const FeatureExtractor_orb32_hip &) = delete;
    FeatureExtractor_orb32_hip &operator=(const FeatureExtractor_orb32_hip &) = delete;

    // 6-argument operator() (FeatureExtractor.cpp:111-121)
    template <class ImageT, class MatT>
    void operator()(const ImageT &img, std::vector<KeyPoint> &keypoints, MatT &descriptors, std::vector<Mat2f> &keyPtsSigma2,
                    std::vector<Mat2f> &keyPtsInf, std::vector<float> &keyPtsSize) {
        (*this)(img, keypoints, descriptors);
        const int n = (int)keypoints.size();
        keyPtsSize.assign(n, 0.f);
        std::vector<float> s2(n), inf(n);
        const int rc = afv_orb_size_sigma(ctx, reinterpret_cast<const afv_keypoint *>(keypoints.data()), n, keyPtsSize.data(),
                                          s2.data(), inf.data());
        if (rc != AFV_OK) fatal("afv_orb_size_sigma", rc, ctx);
        keyPtsSigma2.clear();
        keyPtsInf.clear();
        for (int i = 0; i < n; ++i) {  // computeSigma(SIZE): sigma^2 * I, 1/sigma^2 * I (FeatureExtractor.cpp:159-170)
            keyPtsSigma2.push_back(Mat2f{{{s2[i], 0.f}, {0.f, s2[i]}}});
            keyPtsInf.push_back(Mat2f{{{inf[i], 0.f}, {0.f, inf[i]}}});
        }
    }

    // 3-argument operator() (FeatureExtractor.cpp:123-129)
    template <class ImageT, class MatT>
    void operator()(const ImageT &img, std::vector<KeyPoint> &keypoints, MatT &descriptors) {
        if (settings->ON_automaticTuning) {  // automaticTuning (FeatureExtractor.cpp:195-274): detectTh = th0, once
            settings->detectTh = FeatureExtractorSettings::GetDetectorNominalThreshold();
            settings->ON_automaticTuning = false;
        }
        detectAndCompute(img, keypoints, descriptors);
    }

    // Feature_orb32.cpp:11-18: detect -> quadtree -> describe -> merge, all on the GPU
    template <class ImageT, class MatT>
    void detectAndCompute(const ImageT &img, std::vector<KeyPoint> &keypoints, MatT &descriptors) {
        const auto &g = img.grayImg;
        if (g.empty()) return;  // outputs untouched (ORBextractor.cc:570-571)
        std::vector<KeyPoint> kps((size_t)cap);
        std::vector<uint8_t> desc((size_t)cap * AFV_DESC_BYTES);
        int n = 0;
        const int rc = afv_orb_extract(ctx, g.ptr(0), g.cols, g.rows, (int)row_step(g), reinterpret_cast<afv_keypoint *>(kps.data()),
                                       desc.data(), cap, &n);
        if (rc != AFV_OK) fatal("afv_orb_extract", rc, ctx);
        kps.resize((size_t)n);
        keypoints.swap(kps);  // mergeKeypointLevels clears and refills (FeatureExtractor.cpp:300-307)
        fill_descriptors(descriptors, desc.data(), n);
    }

    // The three virtuals detectAndCompute is composed of (FeatureExtractor.h:123-128), for a host that calls them one by one - a vocabulary
    // builder that keeps keypoints and recomputes descriptors at them (cv::ORB::compute semantics).  detectKeypoints here already
    // includes the quadtree of filterKeypoints (the device never ships cv::ORB::detect's 10x candidate set to the host), so the
    // filterKeypoints override is the identity; detectKeypoints -> filterKeypoints -> computeDescriptors -> mergeKeypointLevels gives
    // detectAndCompute's outputs bit for bit (tests/test_gpu_extract.py::test_plugin_virtuals_one_by_one, adapter_selftest).
    template <class ImageT>
    void detectKeypoints(std::map<int, std::vector<KeyPoint>> &keypoints_level, const ImageT &img, const float & /*detectTh*/, const int & /*nOctaves*/) const {
        const auto &g = img.grayImg;
        if (g.empty()) return;
        std::vector<KeyPoint> kps((size_t)cap);
        int n = 0;
        const int rc = afv_orb_detect(ctx, g.ptr(0), g.cols, g.rows, (int)row_step(g), reinterpret_cast<afv_keypoint *>(kps.data()), cap, &n);
        if (rc != AFV_OK) fatal("afv_orb_detect", rc, ctx);
        for (int i = 0; i < n; ++i) keypoints_level[kps[(size_t)i].octave].push_back(kps[(size_t)i]);  // GetKeypointOctave (Feature_orb32.cpp:55-57)
    }
    template <class MatT>
    void filterKeypoints(std::map<int, std::vector<KeyPoint>> & /*keypoints_level*/, const MatT & /*image*/, const MatT & /*mask*/) const {}
    // descriptors_level[level]: n x 32 rows in the order of keypoints_level[level] (one cv::ORB::compute per level in the reference,
    // Feature_orb32.cpp:49-50; ONE device call here)
    template <class ImageT, class MatT>
    void computeDescriptors(std::map<int, MatT> &descriptors_level, std::map<int, std::vector<KeyPoint>> &keypoints_level, const ImageT &img) const {
        const auto &g = img.grayImg;
        std::vector<KeyPoint> all;
        for (auto &lk : keypoints_level) all.insert(all.end(), lk.second.begin(), lk.second.end());
        std::vector<uint8_t> desc(all.size() * AFV_DESC_BYTES);
        const int rc = afv_orb_compute(ctx, g.ptr(0), g.cols, g.rows, (int)row_step(g), reinterpret_cast<const afv_keypoint *>(all.data()), (int)all.size(),
                                       desc.data());
        if (rc != AFV_OK) fatal("afv_orb_compute", rc, ctx);
        size_t o = 0;
        for (auto &lk : keypoints_level) {
            fill_descriptors(descriptors_level[lk.first], desc.data() + o * AFV_DESC_BYTES, (int)lk.second.size());
            o += lk.second.size();
        }
    }

    // FeatureExtractor::mvImagePyramid (FeatureExtractor.h:142; read by Frame::ComputeStereoMatches, Frame.cc:475,568): the levels of
    // the LAST extracted frame, copied from the device on demand (the mono entry point never asks).  MatT: cv::Mat (CV_8UC1) or Mat8.
    template <class MatT>
    void ImagePyramid(std::vector<MatT> &pyramid) {
        afv_geometry g;
        int rc = afv_get_geometry(ctx, &g);
        if (rc != AFV_OK) fatal("afv_get_geometry", rc, ctx);
        pyramid.resize((size_t)g.nlevels);
        std::vector<uint8_t> tight;
        for (int l = 0; l < g.nlevels; ++l) {
            tight.resize((size_t)g.lw[l] * g.lh[l]);
            rc = afv_debug_get_level(ctx, 0, l, tight.data());
            if (rc != AFV_OK) fatal("afv_debug_get_level", rc, ctx);
#ifdef AFV_WITH_OPENCV
            pyramid[(size_t)l].create(g.lh[l], g.lw[l], CV_8U);
#else
            pyramid[(size_t)l].create(g.lh[l], g.lw[l]);
#endif
            for (int y = 0; y < g.lh[l]; ++y) std::copy(tight.begin() + (size_t)y * g.lw[l], tight.begin() + (size_t)(y + 1) * g.lw[l], pyramid[(size_t)l].ptr(y));
        }
    }

    int GetLevels() { return settings->nOctaves; }
    float GetScaleFactor() { return settings->scaleFactor; }
    std::vector<float> GetScaleFactors() { return mvScaleFactor; }
    int GetKeypointOctave(const KeyPoint &kp) const { return kp.octave; }                                  // Feature_orb32.cpp:55-57
    float GetKeypointSize(const KeyPoint &kp) const { return powf(settings->scaleFactor, float(kp.octave)); }  // :59-61
    afv_ctx *context() { return ctx; }

  private:
    template <class M> static size_t row_step(const M &m) {
#ifdef AFV_WITH_OPENCV
        return (size_t)m.step;
#else
        return m.step();
#endif
    }
    template <class M> static void fill_descriptors(M &m, const uint8_t *src, int n) {
#ifdef AFV_WITH_OPENCV
        m.create(n, AFV_DESC_BYTES, CV_8U);
#else
        m.create(n, AFV_DESC_BYTES);
#endif
        for (int i = 0; i < n; ++i) std::copy(src + (size_t)i * AFV_DESC_BYTES, src + (size_t)(i + 1) * AFV_DESC_BYTES, m.ptr(i));
    }
    int nfeatures;
    afv_ctx *ctx = nullptr;
    int cap = 0;
    std::vector<float> mvScaleFactor;
};

// ---- the device-resident map points (include/afv_hip.h afv_points_*; reference object: MapPoint, src/MapPoint.cc) ----
// One per Map.  LocalMapping writes a point where it calls SetWorldPos / UpdateNormalAndDepth / ComputeDistinctiveDescriptors / SetBadFlag
// ("Resident map points"); a DeviceFrame with a pose then searches the points by id.  Arrays are indexed like `ids`.
class DeviceMapPoints {
  public:
    DeviceMapPoints(afv_ctx *ctx_, int capacity, int desc_bytes = AFV_DESC_BYTES, int float_dim = 0) : ctx(ctx_) {
        const int rc = afv_points_create(ctx, capacity, desc_bytes, float_dim, &p);
        if (rc != AFV_OK) fatal("afv_points_create", rc, ctx);
    }
    ~DeviceMapPoints() { afv_points_destroy(p); }
    DeviceMapPoints(const DeviceMapPoints &) = delete;
    DeviceMapPoints &operator=(const DeviceMapPoints &) = delete;

    // MapPoint::SetWorldPos: xyz = ids.size() x 3 floats
    void SetWorldPos(const std::vector<int32_t> &ids, const float *xyz) { Set(ids, xyz, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); }
    // MapPoint::UpdateNormalAndDepth: normalVector (n x 3), minDistance / maxDistance (the raw members), refSize / refDistance / refSigma
    void UpdateNormalAndDepth(const std::vector<int32_t> &ids, const float *normal, const float *minDistance, const float *maxDistance,
                              const float *refSize, const float *refDistance, const float *refSigma) {
        Set(ids, nullptr, normal, minDistance, maxDistance, refSize, refDistance, refSigma);
    }
    // any subset of the fields at once (nullptr leaves a field as it is)
    void Set(const std::vector<int32_t> &ids, const float *xyz, const float *normal, const float *minDistance, const float *maxDistance,
             const float *refSize, const float *refDistance, const float *refSigma) {
        const int rc = afv_points_set(p, ids.data(), (int)ids.size(), xyz, normal, minDistance, maxDistance, refSize, refDistance, refSigma);
        if (rc != AFV_OK) fatal("afv_points_set", rc, ctx);
    }
    // isBad() / NumberOfObservations() > 0 (SetBadFlag, AddObservation, EraseObservation)
    void SetFlags(const std::vector<int32_t> &ids, const uint8_t *bad, const uint8_t *observed) {
        const int rc = afv_points_set_flags(p, ids.data(), (int)ids.size(), bad, observed);
        if (rc != AFV_OK) fatal("afv_points_set_flags", rc, ctx);
    }
    // MapPoint::ComputeDistinctiveDescriptors: the chosen rows by value ...
    void SetDescriptors(const std::vector<int32_t> &ids, const uint8_t *rows) {
        const int rc = afv_points_set_descriptors(p, ids.data(), (int)ids.size(), rows);
        if (rc != AFV_OK) fatal("afv_points_set_descriptors", rc, ctx);
    }
    // ... or as rows (keyframe slot, feature index) of the keyframe table, copied on the device
    void SetDescriptorsFromTable(const std::vector<int32_t> &ids, afv_table *table, const int32_t *slot, const int32_t *idx) {
        const int rc = afv_points_set_descriptors_from_table(p, ids.data(), (int)ids.size(), table, slot, idx);
        if (rc != AFV_OK) fatal("afv_points_set_descriptors_from_table", rc, ctx);
    }
    afv_points *handle() { return p; }

  private:
    afv_ctx *ctx;
    afv_points *p = nullptr;
};

// ---- the device-resident Frame (include/afv_hip.h afv_frame_*; reference object: Frame, src/Frame.cc:171-240) ----
// One per Frame the tracker keeps alive (currentFrame, lastFrame, the initial frame): Frame::Frame calls Extract() instead of the plain
// operator(), and from then on SearchByProjection / Fuse / SearchForInitialization / ComputeBoW / SearchByBoW(KF, F) and the promotion to
// a KeyFrame read the frame where the extraction left it ("Tracking through a resident frame").
class DeviceFrame {
  public:
    // mnMinX .. mnMaxY: Frame::ComputeImageBounds (Frame.cc:435-466); distorted: mDistCoef.at<float>(0) != 0 (Frame.cc:405)
    // keep_pyramid: the stereo constructor's frames (Frame.cc:76-80) - Extract() leaves the pyramid levels with the frame for ComputeStereoMatches
    DeviceFrame(afv_ctx *ctx_, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, bool distorted = false, int grid_cols = 64, int grid_rows = 48,
                bool keep_pyramid = false)
        : ctx(ctx_) {
        afv_frame_params p{};
        p.struct_size = sizeof(p);
        p.min_x = mnMinX; p.min_y = mnMinY; p.max_x = mnMaxX; p.max_y = mnMaxY;
        p.grid_cols = grid_cols; p.grid_rows = grid_rows;
        p.distorted = distorted ? 1 : 0;
        p.keep_pyramid = keep_pyramid ? 1 : 0;
        const int rc = afv_frame_create(ctx, &p, &f);
        if (rc != AFV_OK) fatal("afv_frame_create", rc, ctx);
    }
    ~DeviceFrame() { afv_frame_destroy(f); }
    DeviceFrame(const DeviceFrame &) = delete;
    DeviceFrame &operator=(const DeviceFrame &) = delete;

    // Frame::ExtractFeatures (Frame.cc:242-259): FeatureExtractor::operator() 3-argument form into the resident frame; the host vectors
    // are filled exactly as by FeatureExtractor_orb32_hip::detectAndCompute
    template <class ImageT, class MatT>
    void Extract(const ImageT &img, std::vector<KeyPoint> &keypoints, MatT &descriptors) {
        const auto &g = img.grayImg;
        if (g.empty()) return;
        const int cap = afv_max_keypoints_per_frame(ctx);
        std::vector<KeyPoint> kps((size_t)cap);
        std::vector<uint8_t> desc((size_t)cap * AFV_DESC_BYTES);
        int n = 0;
#ifdef AFV_WITH_OPENCV
        const size_t step = (size_t)g.step;
#else
        const size_t step = g.step();
#endif
        const int rc = afv_frame_extract(f, g.ptr(0), g.cols, g.rows, (int)step, reinterpret_cast<afv_keypoint *>(kps.data()), desc.data(), cap, &n);
        if (rc != AFV_OK) fatal("afv_frame_extract", rc, ctx);
        kps.resize((size_t)n);
        keypoints.swap(kps);
#ifdef AFV_WITH_OPENCV
        descriptors.create(n, AFV_DESC_BYTES, CV_8U);
#else
        descriptors.create(n, AFV_DESC_BYTES);
#endif
        for (int i = 0; i < n; ++i) std::copy(desc.data() + (size_t)i * AFV_DESC_BYTES, desc.data() + (size_t)(i + 1) * AFV_DESC_BYTES, descriptors.ptr(i));
    }
    // Frame::UndistortKeyPoints for a distorted camera: mvKeysUn after cv::undistortPoints (Frame.cc:411-432); builds the grid
    void SetUndistorted(const std::vector<KeyPoint> &mvKeysUn) {
        std::vector<float> x(mvKeysUn.size()), y(mvKeysUn.size());
        for (size_t i = 0; i < mvKeysUn.size(); ++i) {
            x[i] = mvKeysUn[i].pt.x;
            y[i] = mvKeysUn[i].pt.y;
        }
        const int rc = afv_frame_set_undistorted(f, x.data(), y.data());
        if (rc != AFV_OK) fatal("afv_frame_set_undistorted", rc, ctx);
    }
    // Frame::ComputeStereoMatches (Frame.cc:465-645): this frame is the left eye, `right` the right one (both keep_pyramid, one context).
    // mvuRight / mvDepth are filled as the reference's members and stay on the device for the projection searches and the keyframe table.
    // Returns the number of features with mvuRight >= 0.
    int ComputeStereoMatches(DeviceFrame &right, float mbf, float fx, float th_high, float th_low, std::vector<float> &mvuRight, std::vector<float> &mvDepth) {
        afv_stereo_params p{};
        p.struct_size = sizeof(p);
        p.mbf = mbf; p.fx = fx; p.th_high = th_high; p.th_low = th_low;
        int32_t n_stereo = 0;
        int rc = afv_frame_stereo_match(f, right.f, &p, &n_stereo);
        if (rc != AFV_OK) fatal("afv_frame_stereo_match", rc, ctx);
        GetStereo(mvuRight, mvDepth);
        return n_stereo;
    }
    // Frame::ComputeStereoFromRGBD (Frame.cc:648-669): imDepth as rows of floats (cv::Mat CV_32F: ptr<float>(0), cols, rows, step)
    void ComputeStereoFromRGBD(const float *imDepth, int cols, int rows, size_t step_bytes, float mbf, std::vector<float> &mvuRight, std::vector<float> &mvDepth) {
        const int rc = afv_frame_set_depth(f, imDepth, cols, rows, (int)step_bytes, mbf);
        if (rc != AFV_OK) fatal("afv_frame_set_depth", rc, ctx);
        GetStereo(mvuRight, mvDepth);
    }
    void GetStereo(std::vector<float> &mvuRight, std::vector<float> &mvDepth) {
        const size_t n = (size_t)std::max(N(), 0);
        mvuRight.assign(n, -1.0f);
        mvDepth.assign(n, -1.0f);
        const int rc = afv_frame_get_stereo(f, mvuRight.data(), mvDepth.data(), nullptr, nullptr);
        if (rc != AFV_OK) fatal("afv_frame_get_stereo", rc, ctx);
    }
    // ---- resident map points: the geometry in front of the projection searches runs on the device (afv_frame_search_points) ----
    // Frame::SetPose + the intrinsics: Rcw row-major, tcw, Ow = twc as UpdatePoseMatrices computes it (Frame.cc:270-273)
    void SetPose(const float Rcw[9], const float tcw[3], const float Ow[3], float fx, float fy, float cx, float cy, float mbf) {
        const int rc = afv_frame_set_pose(f, Rcw, tcw, Ow, fx, fy, cx, cy, mbf);
        if (rc != AFV_OK) fatal("afv_frame_set_pose", rc, ctx);
        for (int k = 0; k < 9; ++k) mRcw[k] = Rcw[k];
        for (int k = 0; k < 3; ++k) { mtcw[k] = tcw[k]; mOw[k] = Ow[k]; }
        mK[0] = fx; mK[1] = fy; mK[2] = cx; mK[3] = cy; mK[4] = mbf;
        mHasPose = true;
    }
    // the pose last handed to SetPose: Rcw[9], tcw[3], Ow[3] (PoseOptimization with setPose updates it)
    const float *Rcw() const { return mRcw; }
    const float *tcw() const { return mtcw; }
    const float *Ow() const { return mOw; }
    // Optimizer::PoseOptimization(this) (Optimizer.cc:245-448; Tracking.cc:637, :760, :802, :1247-1278) in one launch: pts[i] = the id of
    // the map point of feature i | -1.  Returns nInitialCorrespondences - nBad and fills mvbOutlier[N]; setPose: pFrame->SetPose (:445) -
    // the optimised pose goes back into the frame with Ow = -Rcw^T tcw in float (Frame.cc:270-273), so the next search runs on it.  The
    // host still walks mvbOutlier as Tracking.cc does (it clears pts[i] of the outliers and counts the inliers with observations)
    int PoseOptimization(DeviceMapPoints &points, const std::vector<int32_t> &pts, std::vector<uint8_t> &mvbOutlier, bool setPose = true) {
        afv_pose_job job{};
        job.struct_size = sizeof(job);
        job.pts = pts.data();
        afv_pose_result r{};
        r.struct_size = sizeof(r);
        mvbOutlier.assign((size_t)std::max(N(), 0) + 1, 0);
        r.outlier = mvbOutlier.data();
        const int rc = afv_frame_pose_optimize(f, points.handle(), &job, 1, &r);
        if (rc != AFV_OK) fatal("afv_frame_pose_optimize", rc, ctx);
        mvbOutlier.resize((size_t)std::max(N(), 0));
        if (setPose) {
            // the intrinsics handed back are those of this object's SetPose: a pose set on the raw handle alone is unknown here
            if (!mHasPose) fatal("DeviceFrame::PoseOptimization(setPose): the pose was not set through DeviceFrame::SetPose", AFV_EINVAL, ctx);
            float Ow[3];
            for (int k = 0; k < 3; ++k) Ow[k] = -r.Rcw[k] * r.tcw[0] + (-r.Rcw[3 + k] * r.tcw[1] + -r.Rcw[6 + k] * r.tcw[2]);
            SetPose(r.Rcw, r.tcw, Ow, mK[0], mK[1], mK[2], mK[3], mK[4]);
        }
        return r.n_good;
    }
    // Tracking::SearchLocalPoints (Tracking.cc:988-1028): isInFrustum of every point of `ids` and SearchByProjection(F, vpMapPoints, th)
    // in one call.  assign[N] = index INTO ids of the point now in F.pts[i] | -1; inView[ids.size()] = mbTrackInView (IncreaseVisible)
    int SearchLocalPoints(DeviceMapPoints &points, const std::vector<int32_t> &ids, float radiusTh, float viewingCosLimit, float thHigh, float nnratio,
                          std::vector<int32_t> &assign, std::vector<uint8_t> &inView, const uint8_t *occupied = nullptr) {
        afv_point_search s = PointSearch(points, ids, AFV_PT_FRUSTUM, radiusTh, thHigh, nnratio, false, occupied);
        s.viewing_cos_limit = viewingCosLimit;
        inView.assign(ids.size() + 1, 0);
        const int n = Search(s, assign, inView.data());
        inView.resize(ids.size());
        return n;
    }
    // SearchByProjection(CurrentFrame = this, LastFrame, th) (FeatureMatcher.cc:1291-1402): ids[i] = the map point of LastFrame's feature i,
    // -1 for none / an outlier
    int SearchByProjectionLast(DeviceMapPoints &points, DeviceFrame &last, const std::vector<int32_t> &ids, float radiusTh, float thHigh, float nnratio,
                               bool checkOrientation, std::vector<int32_t> &assign, const uint8_t *occupied = nullptr) {
        afv_point_search s = PointSearch(points, ids, AFV_PT_LASTFRAME, radiusTh, thHigh, nnratio, checkOrientation, occupied);
        s.qframe = last.f;
        return Search(s, assign, nullptr);
    }
    // SearchByProjection(CurrentFrame = this, pKF, sAlreadyFound, th, useHigh) (:1404-1506): ids[i] = the map point of the keyframe's feature
    // i (-1: none / already found), kfAngles[i] = pKF->mvKeysUn[i].angle
    int SearchByProjectionReloc(DeviceMapPoints &points, const std::vector<int32_t> &ids, const float *kfAngles, float radiusTh, float descDistTh,
                                float nnratio, bool checkOrientation, std::vector<int32_t> &assign, const uint8_t *occupied = nullptr) {
        afv_point_search s = PointSearch(points, ids, AFV_PT_RELOC, radiusTh, descDistTh, nnratio, checkOrientation, occupied);
        s.qangle = kfAngles;
        return Search(s, assign, nullptr);
    }
    // matching core of Fuse(pKF = this, vpMapPoints, th) (:794-940; useInfGate false: Fuse(pKF, Scw, ...)): best[ids.size()] = feature | -1
    int FusePoints(DeviceMapPoints &points, const std::vector<int32_t> &ids, float radiusTh, float thLow, bool useInfGate, std::vector<int32_t> &best) {
        afv_point_search s = PointSearch(points, ids, AFV_PT_FUSE, radiusTh, thLow, 0.0f, false, nullptr);
        best.assign(ids.size() + 1, -1);
        int32_t n = 0;
        const int rc = afv_frame_fuse_points(f, &s, useInfGate ? 1 : 0, best.data(), &n);
        if (rc != AFV_OK) fatal("afv_frame_fuse_points", rc, ctx);
        best.resize(ids.size());
        return n;
    }
    float radiusScale = 1.15f;  // FeatureMatcher's static radiusScale

    int N() const { return afv_frame_count(f); }
    afv_frame *handle() { return f; }
    afv_ctx *context() { return ctx; }

  private:
    float mRcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, mtcw[3] = {0, 0, 0}, mOw[3] = {0, 0, 0};  // the pose last handed to SetPose
    float mK[5] = {0, 0, 0, 0, 0};                                                          // ... and fx fy cx cy mbf
    bool mHasPose = false;
    afv_point_search PointSearch(DeviceMapPoints &points, const std::vector<int32_t> &ids, int flavour, float radiusTh, float th, float nnratio,
                                 bool checkOrientation, const uint8_t *occupied) const {
        afv_point_search s{};
        s.struct_size = sizeof(s);
        s.flavour = flavour;
        s.points = points.handle();
        s.ids = ids.data();
        s.nq = (int32_t)ids.size();
        s.radius_th = radiusTh;
        s.radius_scale = radiusScale;
        s.occupied = occupied;
        s.th_high = th;
        s.nnratio = nnratio;
        s.check_orientation = checkOrientation ? 1 : 0;
        return s;
    }
    int Search(const afv_point_search &s, std::vector<int32_t> &assign, uint8_t *inView) {
        assign.assign((size_t)std::max(N(), 0) + 1, -1);
        int32_t n = 0;
        const int rc = afv_frame_search_points(f, &s, assign.data(), &n, inView, nullptr);
        if (rc != AFV_OK) fatal("afv_frame_search_points", rc, ctx);
        assign.resize((size_t)std::max(N(), 0));
        return n;
    }
    afv_ctx *ctx;
    afv_frame *f = nullptr;
};

// ---- matcher side: flat view of what FeatureMatcher reads from KeyFrame / Frame ----
using FeatureVector = std::map<unsigned, std::vector<unsigned>>;  // DBoW2::FeatureVector (node id -> feature indices)

// The reference's matchers dispatch on the descriptor type (FeatureMatcher::DescriptorDistance, FeatureMatcher.cc:1508-1531): the views
// below carry it as `desc_bytes` (binary rows: 32 ORB, 61 AKAZE, 48 BRISK ..., Hamming) or `float_dim` > 0 (float rows - SIFT128, SURF64,
// KAZE64, R2D2 ...: `descriptors` then points to N x float_dim floats, mDescriptors.ptr<float>(), and the distance is
// cv::norm(a, b, NORM_L2SQR) as a float, Feature_sift128.cpp:132-134).  Both sides of a call must agree.
struct FeatureView {
    const uint8_t *descriptors = nullptr;  // N x desc_bytes (or N x float_dim floats), continuous (KeyFrame::mDescriptors)
    int N = 0;
    int desc_bytes = AFV_DESC_BYTES, float_dim = 0;
    const FeatureVector *featVec = nullptr;  // nullptr => brute force
    const uint8_t *valid = nullptr;          // map point exists && !isBad() (triangulation: has a map point)
    const float *angles = nullptr;           // mvKeysUn[i].angle
    const float *x = nullptr, *y = nullptr;  // mvKeysUn[i].pt       (triangulation)
    const float *sigma2 = nullptr;           // GetKeyPt1DSigma2(i)  (triangulation)
    const float *mvuRight = nullptr;         // KeyFrame::mvuRight (stereo keyframes; nullptr: monocular)  (triangulation)
};

// the queries' descriptors named as rows (slot, idx) of a keyframe table instead of carried by value (afv_proj_queries::qref_*)
struct TableRefs {
    afv_table *table = nullptr;
    const int32_t *slot = nullptr, *idx = nullptr;
};

class FeatureMatcherHip {
  public:
    static inline float TH_LOW = 0.0f, TH_HIGH = 0.0f;  // FeatureMatcher.cc:56-59
    static void setDescriptorDistanceThresholds(float matchingTh) { TH_LOW = TH_HIGH = matchingTh; }  // :1533-1545

    FeatureMatcherHip(afv_ctx *ctx_, float nnratio = 0.6f, bool checkOri = true) : ctx(ctx_), mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    // SearchByBoW(KF1, KF2, vpMatches12) (FeatureMatcher.cc:561-660): matches12[i] = index in KF2 or -1
    int SearchByBoW(const FeatureView &kf1, const FeatureView &kf2, std::vector<int> &matches12) {
        return run(kf1, kf2, AFV_MATCH_KF_KF, matches12);
    }
    // SearchByBoW(KF, Frame, vpMapPointMatches) (:186-283): matchesF[idxF] = index in KF or -1
    int SearchByBoW_Frame(const FeatureView &kf, const FeatureView &frame, std::vector<int> &matchesF) {
        return run(kf, frame, AFV_MATCH_KF_FRAME, matchesF);
    }
    // SearchForTriangulation (:662-790; stereo branches :705-709, :727-731, :741 through FeatureView::mvuRight): vMatchedPairs ascending idx1
    int SearchForTriangulation(const FeatureView &kf1, const FeatureView &kf2, const float F12[9], float ex, float ey,
                               std::vector<std::pair<size_t, size_t>> &vMatchedPairs, bool bOnlyStereo = false) {
        Csr c1(kf1), c2(kf2);
        afv_tri_job t{};
        t.struct_size = sizeof(t);
        fill(t.bow, kf1, kf2, c1, c2, AFV_MATCH_KF_KF);
        t.x1 = kf1.x; t.y1 = kf1.y; t.x2 = kf2.x; t.y2 = kf2.y; t.sigma2_2 = kf2.sigma2;
        for (int i = 0; i < 9; ++i) t.F12[i] = F12[i];
        t.ex = ex; t.ey = ey;
        t.u_right1 = kf1.mvuRight; t.u_right2 = kf2.mvuRight; t.only_stereo = bOnlyStereo ? 1 : 0;
        std::vector<int32_t> m((size_t)std::max(kf1.N, 1), -1);
        int32_t n = 0;
        const int rc = afv_match_triangulation(ctx, &t, 1, m.data(), &n);
        if (rc != AFV_OK) fatal("afv_match_triangulation", rc, ctx);
        vMatchedPairs.clear();
        for (int i = 0; i < kf1.N; ++i)
            if (m[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m[i]);
        return n;
    }

    // ---- projection-guided searches.  The caller evaluates the projections exactly as the reference does
    // and hands over, per query in the reference's iteration order, (u, v, r, size band); see include/afv_hip.h ----
    struct FrameGridView {  // what the matchers read from a Frame / KeyFrame (Frame.cc:100-101, Frame.h:40-41)
        const uint8_t *descriptors = nullptr; int N = 0;
        int desc_bytes = AFV_DESC_BYTES, float_dim = 0;  // descriptor kind (see FeatureView); the queries carry the same kind
        const float *x = nullptr, *y = nullptr;  // mvKeysUn[i].pt
        const float *size = nullptr;             // keyPtsSize[i]
        const float *angle = nullptr;            // mvKeysUn[i].angle
        const uint8_t *occupied = nullptr;       // pts[i] (&& observations > 0 where the reference asks) ; nullptr = none
        const float *inf = nullptr;              // GetKeyPt1DInf(i) (Fuse only)
        const float *mvuRight = nullptr;         // stereo frames / keyframes (nullptr: monocular): FeatureMatcher.cc:114, :880, :1367
        float mnMinX = 0.f, mnMinY = 0.f, mfGridElementWidthInv = 0.f, mfGridElementHeightInv = 0.f;
        int grid_cols = 64, grid_rows = 48;      // FRAME_GRID_COLS / ROWS
        float sizeTolerance = 1.2f, invSizeTolerance = 1.0f / 1.2f;  // Frame.cc:73-74
    };
    struct ProjectionQueries {
        const uint8_t *descriptors = nullptr; int n = 0;  // pMP->GetDescriptor() / LastFrame.mDescriptors
        const float *u = nullptr, *v = nullptr, *r = nullptr, *min_size = nullptr, *max_size = nullptr;
        const uint8_t *valid = nullptr;      // nullptr = all
        const float *angle = nullptr;        // last-frame style searches with orientation check
        const uint8_t *occupies = nullptr;   // pMP->NumberOfObservations() > 0 (nullptr = yes)
        // stereo: projected right-image coordinate (pMP->mTrackProjXR :116 / u - mbf * invzc :1369 / ur :885) and the gate on
        // |ur - mvuRight| of the two SearchByProjection flavours that have one (r * pMP->trackSigma :117 / the window radius :1371)
        const float *ur = nullptr, *er_max = nullptr;
    };
    // SearchByProjection(F, vpMapPoints, radiusTh) (FeatureMatcher.cc:73-154): assign[i] = query stored in F.pts[i] or -1
    int SearchByProjection(const FrameGridView &F, const ProjectionQueries &q, std::vector<int> &assign) {
        return projection(F, q, TH_HIGH, AFV_PROJ_LOCALMAP, false, assign);
    }
    // SearchByProjection(CurrentFrame, LastFrame, radiusTh) (:1291-1402)
    int SearchByProjection_LastFrame(const FrameGridView &F, const ProjectionQueries &q, std::vector<int> &assign) {
        return projection(F, q, TH_HIGH, AFV_PROJ_LASTFRAME, mbCheckOrientation, assign);
    }
    // SearchByProjection(CurrentFrame, pKF, sAlreadyFound, radiusTh, useHighMatchingThreshold) (:1404-1506, relocalisation)
    int SearchByProjection_Reloc(const FrameGridView &F, const ProjectionQueries &q, float th, std::vector<int> &assign) {
        return projection(F, q, th, AFV_PROJ_LASTFRAME, mbCheckOrientation, assign, false);
    }
    // SearchByProjection(pKF, Scw, vpPoints, vpMatched, radiusTh) (:287-397, loop closing)
    int SearchByProjection_Sim3(const FrameGridView &KF, const ProjectionQueries &q, std::vector<int> &assign) {
        return projection(KF, q, TH_LOW, AFV_PROJ_LASTFRAME, false, assign, false);
    }
    // Fuse(pKF, vpMapPoints, radiusTh) (:794-940): best[q] = keypoint index or -1; with KF.inf == nullptr it is
    // Fuse(pKF, Scw, vpPoints, radiusTh, vpReplacePoint) (:942-1064)
    int Fuse(const FrameGridView &KF, const ProjectionQueries &q, std::vector<int> &best) {
        afv_proj_job j = proj_job(KF, q);
        j.th_high = TH_LOW;
        best.assign((size_t)std::max(q.n, 1), -1);
        int32_t n = 0;
        const int rc = afv_match_fuse(ctx, &j, 1, best.data(), &n);
        if (rc != AFV_OK) fatal("afv_match_fuse", rc, ctx);
        best.resize((size_t)q.n);
        return n;
    }
    // SearchBySim3(pKF1, pKF2, vpMatches12, ...) (:1066-1287): q1 = KF1's map points projected into KF2, q2 the reverse
    int SearchBySim3(const FrameGridView &KF1, const ProjectionQueries &q1, const FrameGridView &KF2, const ProjectionQueries &q2,
                     std::vector<int> &matches12) {
        afv_proj_job j12 = proj_job(KF2, q1), j21 = proj_job(KF1, q2);
        j12.th_high = j21.th_high = TH_HIGH;
        matches12.assign((size_t)std::max(q1.n, 1), -1);
        int32_t n = 0;
        const int rc = afv_match_sim3(ctx, &j12, &j21, matches12.data(), &n);
        if (rc != AFV_OK) fatal("afv_match_sim3", rc, ctx);
        matches12.resize((size_t)q1.n);
        return n;
    }
    // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (:399-557): q = F1's features
    int SearchForInitialization(const FrameGridView &F2, const ProjectionQueries &q, std::vector<int> &vnMatches12) {
        afv_proj_job j = proj_job(F2, q);
        j.th_high = TH_LOW;
        j.check_orientation = mbCheckOrientation;
        vnMatches12.assign((size_t)std::max(q.n, 1), -1);
        int32_t n = 0;
        const int rc = afv_match_initialization(ctx, &j, 1, vnMatches12.data(), &n);
        if (rc != AFV_OK) fatal("afv_match_initialization", rc, ctx);
        vnMatches12.resize((size_t)q.n);
        return n;
    }

    // ---- the same searches against a resident frame: nothing of the frame is uploaded, only the queries travel (or, with q_table /
    // q_slot / q_idx, only 8 bytes per query: a map point's descriptor named as the keyframe row MapPoint::ComputeDistinctDescriptors
    // copied it from) ----
    int SearchByProjection(DeviceFrame &F, const ProjectionQueries &q, const uint8_t *occupied, std::vector<int> &assign, TableRefs refs = TableRefs()) {
        return frame_projection(F, q, occupied, TH_HIGH, AFV_PROJ_LOCALMAP, false, refs, assign);
    }
    int SearchByProjection_LastFrame(DeviceFrame &F, const ProjectionQueries &q, const uint8_t *occupied, std::vector<int> &assign,
                                     TableRefs refs = TableRefs()) {
        return frame_projection(F, q, occupied, TH_HIGH, AFV_PROJ_LASTFRAME, mbCheckOrientation, refs, assign);
    }
    int SearchByProjection_Reloc(DeviceFrame &F, const ProjectionQueries &q, const uint8_t *occupied, float th, std::vector<int> &assign) {
        ProjectionQueries mono = q;
        mono.ur = mono.er_max = nullptr;  // no mvuRight branch in :1404-1506
        return frame_projection(F, mono, occupied, th, AFV_PROJ_LASTFRAME, mbCheckOrientation, TableRefs(), assign);
    }
    int Fuse(DeviceFrame &KF, const ProjectionQueries &q, bool reprojection_gate, std::vector<int> &best) {
        afv_proj_queries Q = frame_queries(q, nullptr, TH_LOW, 0, false, TableRefs());
        best.assign((size_t)std::max(q.n, 1), -1);
        int32_t n = 0;
        const int rc = afv_frame_match_fuse(KF.handle(), &Q, reprojection_gate ? 1 : 0, best.data(), &n);
        if (rc != AFV_OK) fatal("afv_frame_match_fuse", rc, ctx);
        best.resize((size_t)q.n);
        return n;
    }
    // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (:399-557) between two resident frames; vbPrevMatched is
    // refreshed like :551-553 when F2's undistorted keypoints are given
    int SearchForInitialization(DeviceFrame &F1, DeviceFrame &F2, std::vector<float> &prev_x, std::vector<float> &prev_y, int windowSize,
                                std::vector<int> &vnMatches12, const std::vector<KeyPoint> *F2_mvKeysUn = nullptr) {
        const int n1 = F1.N();
        vnMatches12.assign((size_t)std::max(n1, 1), -1);
        int32_t n = 0;
        const int rc = afv_frame_match_initialization(F1.handle(), F2.handle(), prev_x.data(), prev_y.data(), (float)windowSize, TH_LOW, mfNNratio,
                                                      mbCheckOrientation ? 1 : 0, vnMatches12.data(), &n);
        if (rc != AFV_OK) fatal("afv_frame_match_initialization", rc, ctx);
        vnMatches12.resize((size_t)n1);
        if (F2_mvKeysUn)
            for (int i = 0; i < n1; ++i)
                if (vnMatches12[i] >= 0) {
                    prev_x[i] = (*F2_mvKeysUn)[(size_t)vnMatches12[i]].pt.x;
                    prev_y[i] = (*F2_mvKeysUn)[(size_t)vnMatches12[i]].pt.y;
                }
        return n;
    }

  private:
    afv_proj_queries frame_queries(const ProjectionQueries &q, const uint8_t *occupied, float th, int mode, bool ori, TableRefs refs) const {
        afv_proj_queries Q{};
        Q.struct_size = sizeof(Q);
        Q.nq = q.n; Q.qdesc = refs.table ? nullptr : q.descriptors; Q.desc_bytes = AFV_DESC_BYTES;
        Q.qvalid = q.valid; Q.qu = q.u; Q.qv = q.v; Q.qr = q.r; Q.qmin_size = q.min_size; Q.qmax_size = q.max_size;
        Q.qangle = q.angle; Q.qoccupies = q.occupies; Q.q_ur = q.ur; Q.q_er_max = q.er_max;
        Q.occupied = occupied;
        Q.th_high = th; Q.nnratio = mfNNratio; Q.check_orientation = ori ? 1 : 0; Q.mode = mode;
        Q.qref_table = refs.table; Q.qref_slot = refs.slot; Q.qref_idx = refs.idx;
        return Q;
    }
    int frame_projection(DeviceFrame &F, const ProjectionQueries &q, const uint8_t *occupied, float th, int mode, bool ori, TableRefs refs,
                         std::vector<int> &assign) {
        afv_proj_queries Q = frame_queries(q, occupied, th, mode, ori, refs);
        const int n = F.N();
        assign.assign((size_t)std::max(n, 1), -1);
        int32_t nm = 0;
        const int rc = afv_frame_match_projection(F.handle(), &Q, assign.data(), &nm);
        if (rc != AFV_OK) fatal("afv_frame_match_projection", rc, ctx);
        assign.resize((size_t)n);
        return nm;
    }
    afv_proj_job proj_job(const FrameGridView &F, const ProjectionQueries &q) const {
        afv_proj_job j{};
        j.struct_size = sizeof(j);
        j.desc = F.descriptors; j.n = F.N; j.desc_bytes = F.float_dim ? 4 * F.float_dim : F.desc_bytes; j.float_dim = F.float_dim;
        j.x = F.x; j.y = F.y; j.size = F.size; j.angle = F.angle; j.occupied = F.occupied; j.inf = F.inf;
        j.min_x = F.mnMinX; j.min_y = F.mnMinY; j.grid_inv_w = F.mfGridElementWidthInv; j.grid_inv_h = F.mfGridElementHeightInv;
        j.grid_cols = F.grid_cols; j.grid_rows = F.grid_rows;
        j.nq = q.n; j.qdesc = q.descriptors; j.qvalid = q.valid; j.qu = q.u; j.qv = q.v; j.qr = q.r;
        j.qmin_size = q.min_size; j.qmax_size = q.max_size; j.qangle = q.angle; j.qoccupies = q.occupies;
        j.nnratio = mfNNratio; j.size_tol = F.sizeTolerance; j.inv_size_tol = F.invSizeTolerance;
        j.u_right = F.mvuRight; j.q_ur = q.ur; j.q_er_max = q.er_max;
        return j;
    }
    // stereo = false: the relocalisation / Sim3 flavours share the entry point but have no mvuRight branch (:287-397, :1404-1506)
    int projection(const FrameGridView &F, const ProjectionQueries &q, float th, int mode, bool ori, std::vector<int> &assign, bool stereo = true) {
        afv_proj_job j = proj_job(F, q);
        if (!stereo) j.u_right = nullptr;
        j.th_high = th; j.mode = mode; j.check_orientation = ori;
        assign.assign((size_t)std::max(F.N, 1), -1);
        int32_t n = 0;
        const int rc = afv_match_projection(ctx, &j, 1, assign.data(), &n);
        if (rc != AFV_OK) fatal("afv_match_projection", rc, ctx);
        assign.resize((size_t)F.N);
        return n;
    }
    struct Csr {
        std::vector<int32_t> id, ptr, idx;
        explicit Csr(const FeatureView &v) {
            if (!v.featVec) return;
            ptr.push_back(0);
            for (const auto &kv : *v.featVec) {
                id.push_back((int32_t)kv.first);
                for (unsigned f : kv.second) idx.push_back((int32_t)f);
                ptr.push_back((int32_t)idx.size());
            }
        }
    };
    void fill(afv_match_job &j, const FeatureView &a, const FeatureView &b, const Csr &ca, const Csr &cb, int mode) const {
        j.desc1 = a.descriptors; j.n1 = a.N; j.desc2 = b.descriptors; j.n2 = b.N;
        if (a.float_dim != b.float_dim || a.desc_bytes != b.desc_bytes) fatal("FeatureMatcherHip: the two sides carry different descriptor kinds", AFV_EINVAL, ctx);
        j.desc_bytes = a.float_dim ? 4 * a.float_dim : a.desc_bytes;
        if (a.float_dim) mode |= AFV_MATCH_FLOAT32;
        j.node_id1 = ca.id.data(); j.seg_ptr1 = ca.ptr.data(); j.seg_idx1 = ca.idx.data(); j.nnodes1 = (int32_t)ca.id.size();
        j.node_id2 = cb.id.data(); j.seg_ptr2 = cb.ptr.data(); j.seg_idx2 = cb.idx.data(); j.nnodes2 = (int32_t)cb.id.size();
        j.valid1 = a.valid; j.valid2 = b.valid; j.angle1 = a.angles; j.angle2 = b.angles;
        j.th_low = TH_LOW; j.nnratio = mfNNratio; j.check_orientation = mbCheckOrientation && a.angles && b.angles; j.mode = mode;
    }
    int run(const FeatureView &a, const FeatureView &b, int mode, std::vector<int> &out) {
        Csr ca(a), cb(b);
        afv_match_job j{};
        fill(j, a, b, ca, cb, mode);
        const int nout = mode == AFV_MATCH_KF_FRAME ? b.N : a.N;
        out.assign((size_t)std::max(nout, 1), -1);
        int32_t n = 0;
        const int rc = afv_match_bow(ctx, &j, 1, out.data(), &n);
        if (rc != AFV_OK) fatal("afv_match_bow", rc, ctx);
        out.resize((size_t)nout);
        return n;
    }
    afv_ctx *ctx;
    float mfNNratio;
    bool mbCheckOrientation;
};


// ---- AKAZE61 plugin (reference include/Feature_akaze61.h, src/Feature_akaze61.cpp) ----
class FeatureExtractor_akaze61_hip {
  public:
    FeatureExtractor_akaze61_hip(const int &nfeatures_, std::shared_ptr<FeatureExtractorSettings> &settings_, int device = 0,
                                 int max_width = 1280, int max_height = 720)
        : settings(settings_), nfeatures(nfeatures_) {
        afv_akaze_params p;
        afv_akaze_default_params(&p);
        p.omax = FeatureExtractorSettings::numOctaves0 / 4;        // Feature_akaze61.cpp:12
        p.nsublevels = FeatureExtractorSettings::numOctaves0 / 2;  // :13
        p.dthreshold = settings->detectTh;                         // :14
        p.nfeatures = nfeatures;
        p.scale_factor = FeatureExtractorSettings::scaleFactor0;
        p.max_width = max_width; p.max_height = max_height; p.max_batch = 1;
        const int rc = afv_akaze_create(device, &p, &akz);
        if (rc != AFV_OK) fatal("afv_akaze_create", rc, nullptr);
        cap = nfeatures + 64;
        kbuf.resize((size_t)cap);
        dbuf.resize((size_t)cap * 61);
    }
    ~FeatureExtractor_akaze61_hip() { afv_akaze_destroy(akz); }
    FeatureExtractor_akaze61_hip(const FeatureExtractor_akaze61_hip &) = delete;
    FeatureExtractor_akaze61_hip &operator=(const FeatureExtractor_akaze61_hip &) = delete;

    // detectAndCompute (Feature_akaze61.cpp:17-24): initializeExtractor + detectKeypoints + filterKeypoints + computeDescriptors +
    // mergeKeypointLevels in one call; descriptors = N x 61 CV_8U
    template <class ImageT, class MatT>
    void detectAndCompute(const ImageT &img, std::vector<KeyPoint> &keypoints, MatT &descriptors) {
        const auto &g = img.grayImg;
        if (g.empty()) return;
        int32_t n = 0;
        const int rc = afv_akaze_extract(akz, g.ptr(), 1, g.cols, g.rows, (int)row_step(g), 0, kbuf.data(), dbuf.data(), cap, &n);
        if (rc == AFV_ECAPACITY) {
            // a device-side capacity was exceeded on a very busy frame: the outputs are a truncated but valid result
            // (the reference has no such limit; losing the surplus beats terminating the SLAM process)
            std::fprintf(stderr, "afv: afv_akaze_extract: %s (%s) - keeping %d keypoints\n", afv_strerror(rc), afv_akaze_last_error(akz), (int)n);
            if (n < 0 || n > cap) n = 0;
        } else if (rc != AFV_OK) {
            std::fprintf(stderr, "afv: afv_akaze_extract failed: %s (%s)\n", afv_strerror(rc), afv_akaze_last_error(akz));
            std::terminate();
        }
        keypoints.resize((size_t)n);
        static_assert(sizeof(KeyPoint) == sizeof(afv_keypoint), "KeyPoint layout");
        if (n) std::memcpy(static_cast<void *>(keypoints.data()), kbuf.data(), (size_t)n * sizeof(afv_keypoint));
#ifdef AFV_WITH_OPENCV
        descriptors.create(n, 61, CV_8U);
#else
        descriptors.create(n, 61);
#endif
        for (int i = 0; i < n; ++i) std::memcpy(descriptors.ptr(i), dbuf.data() + (size_t)i * 61, 61);
    }
    int GetKeypointOctave(const KeyPoint &kp) const { return kp.class_id; }  // Feature_akaze61.cpp:55-57
    float GetKeypointSize(const KeyPoint &kp) const { return powf(FeatureExtractorSettings::scaleFactor0, float(GetKeypointOctave(kp))); }  // :59-61
    std::shared_ptr<FeatureExtractorSettings> settings;

  private:
    template <class M> static size_t row_step(const M &m) {  // ROI / non-continuous images: the true row stride
#ifdef AFV_WITH_OPENCV
        return (size_t)m.step;
#else
        return m.step();
#endif
    }
    int nfeatures, cap = 0;
    afv_akaze *akz = nullptr;
    std::vector<afv_keypoint> kbuf;
    std::vector<uint8_t> dbuf;
};

// ---- Vocabulary::transform on the GPU (reference include/Vocabulary.h, src/Vocabulary.cpp:156-206) ----
using BowVector = std::map<unsigned, double>;  // DBoW2::BowVector (word id -> weight)

class VocabularyHip {
  public:
    // nodes in DBoW2 id order (node 0 = root): parent id, leaf flag, 32-byte descriptor, weight — what loadFromTextFile reads
    VocabularyHip(afv_ctx *ctx_, int k_, int L_, const std::vector<int> &parent, const std::vector<uint8_t> &is_leaf,
                  const std::vector<uint8_t> &node_desc, const std::vector<double> &weight_)
        : ctx(ctx_), k(k_), L(L_), weight(weight_) {
        const int n = (int)parent.size();
        std::vector<int32_t> child_ptr((size_t)n + 1, 0), child_idx((size_t)std::max(n - 1, 1));
        for (int i = 1; i < n; ++i) child_ptr[(size_t)parent[i] + 1]++;
        for (int i = 0; i < n; ++i) child_ptr[i + 1] += child_ptr[i];
        std::vector<int32_t> fill(child_ptr.begin(), child_ptr.end() - 1);
        for (int i = 1; i < n; ++i) child_idx[(size_t)fill[parent[i]]++] = i;  // children keep their id order
        word_id.assign((size_t)n, -1);
        int words = 0;
        for (int i = 0; i < n; ++i)
            if (is_leaf[i]) word_id[i] = words++;
        int rc = afv_vocab_create(ctx, k, L, n, child_ptr.data(), child_idx.data(), node_desc.data(), 32, &voc);
        if (rc != AFV_OK) fatal("afv_vocab_create", rc, ctx);
        std::vector<uint8_t> stopped((size_t)n, 0);  // DBoW2 transform: a word enters the vectors only if (w > 0)
        bool any = false;
        for (int i = 0; i < n; ++i)
            if (is_leaf[i] && !(weight[(size_t)i] > 0)) stopped[(size_t)i] = 1, any = true;
        if (any) {
            rc = afv_vocab_set_stopped(ctx, voc, stopped.data());
            if (rc != AFV_OK) fatal("afv_vocab_set_stopped", rc, ctx);
        }
    }
    ~VocabularyHip() { afv_vocab_destroy(ctx, voc); }
    VocabularyHip(const VocabularyHip &) = delete;
    VocabularyHip &operator=(const VocabularyHip &) = delete;

    // transform(mDescriptors, mBowVec, mFeatVec) with levelsup = 4 (Vocabulary.cpp:156-206)
    void transform(const uint8_t *descriptors, int n, BowVector &bow, FeatureVector &fv, int levelsup = 4) {
        bow.clear();
        fv.clear();
        std::vector<int32_t> leaf((size_t)std::max(n, 1)), nid((size_t)std::max(n, 1));
        const int rc = afv_bow_transform(ctx, voc, descriptors, n, levelsup, leaf.data(), nid.data());
        if (rc != AFV_OK) fatal("afv_bow_transform", rc, ctx);
        for (int i = 0; i < n; ++i) {
            const double w = weight[(size_t)leaf[i]];
            if (w > 0) {
                bow[(unsigned)word_id[(size_t)leaf[i]]] += w;  // BowVector::addWeight
                fv[(unsigned)nid[i]].push_back((unsigned)i);    // FeatureVector::addFeature
            }
        }
        double s = 0;
        for (const auto &kv : bow) s += std::fabs(kv.second);
        if (s > 0)
            for (auto &kv : bow) kv.second /= s;  // BowVector::normalize(L1)
    }

    // Frame::ComputeBoW (Frame.cc:397-401) on a resident frame: mBowVec / mFeatVec for the host's own use (KeyFrameDatabase scoring);
    // the FeatureVector also stays on the device with the frame (SearchByBoW(KF, F) through afv_table_match_bow_frame_h, promotion)
    void transform(DeviceFrame &F, BowVector &bow, FeatureVector &fv, int levelsup = 4) {
        bow.clear();
        fv.clear();
        const int n = F.N();
        std::vector<int32_t> leaf((size_t)std::max(n, 1)), nid((size_t)std::max(n, 1));
        const int rc = afv_frame_bow_transform(F.handle(), voc, levelsup, leaf.data(), nid.data(), nullptr);
        if (rc != AFV_OK) fatal("afv_frame_bow_transform", rc, ctx);
        for (int i = 0; i < n; ++i) {
            const double w = weight[(size_t)leaf[i]];
            if (w > 0) {
                bow[(unsigned)word_id[(size_t)leaf[i]]] += w;
                fv[(unsigned)nid[i]].push_back((unsigned)i);
            }
        }
        double s = 0;
        for (const auto &kv : bow) s += std::fabs(kv.second);
        if (s > 0)
            for (auto &kv : bow) kv.second /= s;
    }
    afv_vocab *handle() { return voc; }

  private:
    afv_ctx *ctx;
    int k, L;
    std::vector<double> weight;
    std::vector<int32_t> word_id;
    afv_vocab *voc = nullptr;
};

// ---- KeyFrameDatabase (reference include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:40-309; LoopClosing.cc:137-157) over a keyframe
// table that holds the keyframes' BowVectors (afv_table_set_bowvec / afv_table_set_from_frame).  Words in common and Vocabulary::score
// of the query against every keyframe of the database come from ONE afv_table_score_bow call; the reference's float arithmetic (0.8f,
// 0.75f, the covisibility accumulation) stays here.  The covisibility graph is the caller's: GetConnectedKeyFrames comes in as a list,
// GetBestCovisibilityKeyFrames(10) as a function.  Keyframes are named by their table slot.  The candidate order is the reference's:
// (smallest shared word, add sequence) = the order its inverted-file walk meets the keyframes.  KeyFrame::mRelocScore outlives a query
// (KeyFrameDatabase.cc:273-276 reads it for neighbours this query did not score): kept per slot, 0 until first scored. ----
class KeyFrameDatabase {
  public:
    using Covisibles = std::function<std::vector<int>(int)>;
    KeyFrameDatabase(afv_ctx *ctx_, afv_table *table_, int nsets_) : ctx(ctx_), table(table_), nsets(nsets_), seq((size_t)nsets_, -1), reloc_score((size_t)nsets_, 0.0f) {}

    void add(int slot) {  // :40-46
        if (slot >= 0 && slot < nsets && seq[(size_t)slot] < 0) seq[(size_t)slot] = next++;
    }
    void erase(int slot) {  // :48-67
        if (slot >= 0 && slot < nsets) seq[(size_t)slot] = -1;
    }
    void clear() { std::fill(seq.begin(), seq.end(), -1L); }  // :69-73

    // DetectRelocalizationCandidates(Frame *F) (:199-309): the frame's resident BowVector is the query (VocabularyHip::transform(DeviceFrame &...)
    // on a vocabulary with weights ran before), or a host BowVector
    std::vector<int> DetectRelocalizationCandidates(DeviceFrame &F, const Covisibles &best_covisibles) {
        afv_bow_query q{};
        q.struct_size = sizeof(q);
        q.kind = AFV_BOW_QUERY_FRAME;
        q.frame = F.handle();
        return reloc(q, best_covisibles);
    }
    std::vector<int> DetectRelocalizationCandidates(const BowVector &bow, const Covisibles &best_covisibles) {
        std::vector<int32_t> w;
        std::vector<double> v;
        return reloc(host_query(bow, w, v), best_covisibles);
    }

    // DetectLoopCandidates(pKF, minScore) (:76-197); connected = pKF->GetConnectedKeyFrames()
    std::vector<int> DetectLoopCandidates(int slot, float minScore, const std::vector<int> &connected, const Covisibles &best_covisibles) {
        std::vector<uint8_t> mask = members();
        for (int s : connected)
            if (s >= 0 && s < nsets) mask[(size_t)s] = 0;
        afv_bow_query q = slot_query(slot);
        run(q, mask);
        std::vector<int> sharing = sharing_words(mask);
        if (sharing.empty()) return {};
        const int minCommonWords = min_common(sharing);
        std::vector<uint8_t> scored((size_t)nsets, 0);
        std::vector<float> loop_score((size_t)nsets, 0.0f);
        std::vector<std::pair<float, int>> lScoreAndMatch;
        for (int s : sharing)
            if (common[(size_t)s] > minCommonWords) {
                const float si = (float)score[(size_t)s];
                loop_score[(size_t)s] = si;
                scored[(size_t)s] = 1;
                if (si >= minScore) lScoreAndMatch.emplace_back(si, s);
            }
        if (lScoreAndMatch.empty()) return {};
        std::vector<std::pair<float, int>> lAccScoreAndMatch;
        float bestAccScore = minScore;
        for (const auto &it : lScoreAndMatch) {
            float bestScore = it.first, accScore = it.first;
            int best = it.second;
            for (int k2 : best_covisibles(it.second))
                if (k2 >= 0 && k2 < nsets && scored[(size_t)k2]) {  // mnLoopQuery == this query && mnLoopWords > minCommonWords
                    accScore += loop_score[(size_t)k2];
                    if (loop_score[(size_t)k2] > bestScore) {
                        best = k2;
                        bestScore = loop_score[(size_t)k2];
                    }
                }
            lAccScoreAndMatch.emplace_back(accScore, best);
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        return retain(lAccScoreAndMatch, bestAccScore);
    }

    // the reference score of LoopClosing::DetectLoop (LoopClosing.cc:142-155): the lowest score to a (not bad) covisible keyframe
    float min_score_to_connected(int slot, const std::vector<int> &connected) {
        float minScore = 1;
        if (connected.empty()) return minScore;
        std::vector<uint8_t> mask((size_t)nsets, 0);
        for (int s : connected)
            if (s >= 0 && s < nsets) mask[(size_t)s] = 1;
        afv_bow_query q = slot_query(slot);
        run(q, mask);
        for (int s : connected) {
            if (s < 0 || s >= nsets) continue;
            const float sc = (float)score[(size_t)s];
            if (sc < minScore) minScore = sc;
        }
        return minScore;
    }

    // Vocabulary::score of the last query against every slot (doubles, as DBoW2 returns them), -1 counts for slots left out
    const std::vector<double> &last_scores() const { return score; }
    const std::vector<int32_t> &last_common() const { return common; }

  private:
    std::vector<uint8_t> members() const {
        std::vector<uint8_t> mask((size_t)nsets, 0);
        for (int s = 0; s < nsets; ++s) mask[(size_t)s] = seq[(size_t)s] >= 0;
        return mask;
    }
    static afv_bow_query slot_query(int slot) {
        afv_bow_query q{};
        q.struct_size = sizeof(q);
        q.kind = AFV_BOW_QUERY_SLOT;
        q.slot = slot;
        return q;
    }
    static afv_bow_query host_query(const BowVector &bow, std::vector<int32_t> &w, std::vector<double> &v) {
        for (const auto &kv : bow) {
            w.push_back((int32_t)kv.first);
            v.push_back(kv.second);
        }
        afv_bow_query q{};
        q.struct_size = sizeof(q);
        q.kind = AFV_BOW_QUERY_HOST;
        q.n = (int32_t)w.size();
        q.word = w.data();
        q.value = v.data();
        return q;
    }
    void run(const afv_bow_query &q, const std::vector<uint8_t> &mask) {
        common.assign((size_t)nsets, -1);
        score.assign((size_t)nsets, 0.0);
        first.assign((size_t)nsets, -1);
        const int rc = afv_table_score_bow(table, &q, 1, mask.data(), common.data(), score.data(), first.data());
        if (rc != AFV_OK) fatal("afv_table_score_bow", rc, ctx);
    }
    // lKFsSharingWords in the order the inverted-file walk builds it
    std::vector<int> sharing_words(const std::vector<uint8_t> &mask) const {
        std::vector<int> sharing;
        for (int s = 0; s < nsets; ++s)
            if (mask[(size_t)s] && seq[(size_t)s] >= 0 && common[(size_t)s] > 0) sharing.push_back(s);
        std::sort(sharing.begin(), sharing.end(), [&](int a, int b) {
            return first[(size_t)a] != first[(size_t)b] ? first[(size_t)a] < first[(size_t)b] : seq[(size_t)a] < seq[(size_t)b];
        });
        return sharing;
    }
    int min_common(const std::vector<int> &sharing) const {
        int maxCommonWords = 0;
        for (int s : sharing)
            if (common[(size_t)s] > maxCommonWords) maxCommonWords = common[(size_t)s];
        return (int)(maxCommonWords * 0.8f);  // int minCommonWords = maxCommonWords*0.8f
    }
    std::vector<int> reloc(const afv_bow_query &q, const Covisibles &best_covisibles) {
        const std::vector<uint8_t> mask = members();
        run(q, mask);
        std::vector<int> sharing = sharing_words(mask);
        if (sharing.empty()) return {};
        const int minCommonWords = min_common(sharing);
        std::vector<uint8_t> in_query((size_t)nsets, 0);
        for (int s : sharing) in_query[(size_t)s] = 1;
        std::vector<std::pair<float, int>> lScoreAndMatch;
        for (int s : sharing)
            if (common[(size_t)s] > minCommonWords) {
                const float si = (float)score[(size_t)s];
                reloc_score[(size_t)s] = si;
                lScoreAndMatch.emplace_back(si, s);
            }
        if (lScoreAndMatch.empty()) return {};
        std::vector<std::pair<float, int>> lAccScoreAndMatch;
        float bestAccScore = 0;
        for (const auto &it : lScoreAndMatch) {
            float bestScore = it.first, accScore = bestScore;
            int best = it.second;
            for (int k2 : best_covisibles(it.second)) {
                if (k2 < 0 || k2 >= nsets || !in_query[(size_t)k2]) continue;  // mnRelocQuery != F->mnId
                accScore += reloc_score[(size_t)k2];
                if (reloc_score[(size_t)k2] > bestScore) {
                    best = k2;
                    bestScore = reloc_score[(size_t)k2];
                }
            }
            lAccScoreAndMatch.emplace_back(accScore, best);
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        return retain(lAccScoreAndMatch, bestAccScore);
    }
    static std::vector<int> retain(const std::vector<std::pair<float, int>> &lAccScoreAndMatch, float bestAccScore) {
        const float minScoreToRetain = 0.75f * bestAccScore;
        std::set<int> spAlreadyAddedKF;
        std::vector<int> out;
        for (const auto &it : lAccScoreAndMatch)
            if (it.first > minScoreToRetain && !spAlreadyAddedKF.count(it.second)) {
                out.push_back(it.second);
                spAlreadyAddedKF.insert(it.second);
            }
        return out;
    }
    afv_ctx *ctx;
    afv_table *table;
    int nsets;
    long next = 0;
    std::vector<long> seq;  // add sequence per slot, -1 = not in the database
    std::vector<float> reloc_score;
    std::vector<int32_t> common, first;
    std::vector<double> score;
};

// ---- new map points: the neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:265-472) over slots of the keyframe
// table (include/afv_hip.h, "new map points").  The keyframes' sizes, depths and distorted keypoints sit in the table's scale planes
// (afv_table_set_scale, or afv_table_set_from_frame at promotion); the new points land in the resident store without a host upload. ----
class NewMapPoints {
  public:
    struct Created {  // one new point: its id in the store and its two observations (slot, feature)
        int32_t id, slot1, idx1, slot2, idx2;
    };
    struct Result {  // per pair: rows of `cap` entries
        std::vector<uint8_t> status, route;  // AFV_TRI_* / AFV_TRI_ROUTE_*
        std::vector<float> x3d;              // cap x 3 per pair
        std::vector<int32_t> new_id, n_new;  // -1 = not accepted; per pair
    };
    NewMapPoints(afv_ctx *ctx_, afv_table *table_, int cap_) : ctx(ctx_), table(table_), cap(cap_) {}

    // the match loop (:315-461) for npairs pairs in ONE call: two launches, one wait.  match12: npairs rows of cap entries as
    // afv_table_match_triangulation returns them; points may be null
    Result Triangulate(const std::vector<int32_t> &pair_a, const std::vector<int32_t> &pair_b, std::vector<afv_tri_points_job> jobs,
                       const int32_t *match12, DeviceMapPoints *points, int32_t first_id) {
        const size_t np = pair_a.size(), cells = np * (size_t)cap;
        Result r;
        r.status.assign(cells, 0); r.route.assign(cells, 0); r.x3d.assign(cells * 3, 0.0f); r.new_id.assign(cells, -1); r.n_new.assign(np, 0);
        for (afv_tri_points_job &j : jobs) j.struct_size = (uint32_t)sizeof(afv_tri_points_job);
        const int rc = afv_table_triangulate(table, pair_a.data(), pair_b.data(), jobs.data(), (int)np, match12, points ? points->handle() : nullptr, first_id,
                                             r.status.data(), r.route.data(), r.x3d.data(), r.new_id.data(), r.n_new.data());
        if (rc != AFV_OK) fatal("afv_table_triangulate", rc, ctx);
        return r;
    }

    // the loop as the reference runs it: one neighbour at a time (one afv_table_match_triangulation and one afv_table_triangulate each);
    // between neighbours the features of `cur` and of that neighbour that received a point are marked in has_mp (one mask of cap bytes per
    // slot, UPDATED in place).  neighbours: the slots that survived the caller's baseline tests (:272-289); jobs[k] / tri[k] belong to
    // neighbour k (tri[k].has_mp1 / has_mp2 are set here).  Batching every neighbour into one Triangulate call is possible; a stale mask
    // then no longer gives the reference's answer (a feature may receive a point from several neighbours).
    std::vector<Created> CreateNewMapPoints(DeviceMapPoints &points, int32_t cur, const std::vector<int32_t> &neighbours,
                                            const std::vector<afv_tri_points_job> &jobs, std::vector<afv_table_tri_job> tri,
                                            std::vector<std::vector<uint8_t>> &has_mp, int32_t first_id) {
        std::vector<Created> out;
        std::vector<int32_t> m((size_t)cap);
        int32_t nid = first_id;
        for (size_t k = 0; k < neighbours.size(); ++k) {
            const int32_t nb = neighbours[k];
            int32_t nm = 0;
            tri[k].struct_size = (uint32_t)sizeof(afv_table_tri_job);
            tri[k].has_mp1 = has_mp[(size_t)cur].data();
            tri[k].has_mp2 = has_mp[(size_t)nb].data();
            const int rc = afv_table_match_triangulation(table, &cur, &nb, &tri[k], 1, m.data(), &nm);
            if (rc != AFV_OK) fatal("afv_table_match_triangulation", rc, ctx);
            const Result r = Triangulate({cur}, {nb}, {jobs[k]}, m.data(), &points, nid);
            for (int i = 0; i < cap; ++i)
                if (r.new_id[(size_t)i] >= 0) {
                    out.push_back(Created{r.new_id[(size_t)i], cur, i, nb, m[(size_t)i]});
                    has_mp[(size_t)cur][(size_t)i] = 1;
                    has_mp[(size_t)nb][(size_t)m[(size_t)i]] = 1;
                    ++nid;
                }
        }
        return out;
    }

    // the same loop with the same arguments and the same result from ONE afv_table_create_new_points call: one upload, two launches per
    // neighbour, one wait; the masks stay on the device between the neighbours and come back updated.  A store that cannot take the
    // points of a neighbour is fatal here as it is in the loop above (afv_table_create_new_points itself reports how far it came)
    std::vector<Created> CreateNewMapPointsChain(DeviceMapPoints &points, int32_t cur, const std::vector<int32_t> &neighbours,
                                                 std::vector<afv_tri_points_job> jobs, std::vector<afv_table_tri_job> tri,
                                                 std::vector<std::vector<uint8_t>> &has_mp, int32_t first_id) {
        const size_t nn = neighbours.size(), cells = nn * (size_t)cap;
        std::vector<uint8_t> nb_masks(cells);
        for (size_t k = 0; k < nn; ++k) {
            tri[k].struct_size = (uint32_t)sizeof(afv_table_tri_job);
            tri[k].has_mp1 = tri[k].has_mp2 = nullptr;
            jobs[k].struct_size = (uint32_t)sizeof(afv_tri_points_job);
            std::memcpy(nb_masks.data() + k * (size_t)cap, has_mp[(size_t)neighbours[k]].data(), (size_t)cap);
        }
        std::vector<int32_t> m(cells), new_id(cells), n_new(nn);
        int32_t n_done = 0;
        const int rc = afv_table_create_new_points(table, cur, neighbours.data(), (int)nn, tri.data(), jobs.data(), has_mp[(size_t)cur].data(),
                                                   nb_masks.data(), points.handle(), first_id, m.data(), nullptr, nullptr, nullptr, new_id.data(),
                                                   n_new.data(), &n_done);
        if (rc != AFV_OK) fatal("afv_table_create_new_points", rc, ctx);
        std::vector<Created> out;
        for (size_t k = 0; k < nn; ++k) {
            const size_t o = k * (size_t)cap;
            for (int i = 0; i < cap; ++i)
                if (new_id[o + (size_t)i] >= 0) out.push_back(Created{new_id[o + (size_t)i], cur, i, neighbours[k], m[o + (size_t)i]});
            std::memcpy(has_mp[(size_t)neighbours[k]].data(), nb_masks.data() + o, (size_t)cap);
        }
        return out;
    }

  private:
    afv_ctx *ctx;
    afv_table *table;
    int cap;
};

// ---- Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) as LoopClosing::ComputeSim3 uses it (src/LoopClosing.cc:247-416): Batch makes
// ONE afv_table_sim3_hypotheses call for all candidates of a loop check - every solver's constructor and every RANSAC hypothesis run on
// the device (include/afv_hip.h, "Sim3Solver": quirks Q1-Q3, deviations S1-S6) - and returns one solver per candidate.  iterate / find are
// host code over the per-hypothesis counts, transforms and inlier words: hypothesis h depends on (seed, h) alone, so the reference's
// sequential rule (running best, return on > minInliers) is a scan.  T12 is 16 floats row-major (cv::Mat 4 x 4 CV_32F in the reference).
class Sim3Solver {
  public:
    struct Camera {  // one keyframe of a job: Rcw row-major, tcw, the intrinsics
        float Rcw[9], tcw[3], fx, fy, cx, cy;
    };
    // cur: the slot of the current keyframe (mN1 = n1 features), cands: the candidates' slots; mp1[n1]: the point id per feature of the
    // current keyframe (GetMapPointMatches, -1 = none); mp2 / idx2: per candidate n1 entries, vpMatched12 as point ids and
    // GetIndexInKeyFrame of those points in their candidate; idx1: the same for mp1 in the current keyframe (empty: the feature itself);
    // candidate c draws from seed + c
    static std::vector<Sim3Solver> Batch(afv_ctx *ctx, afv_table *table, int cap, DeviceMapPoints &points, int32_t cur, const Camera &cam_cur,
                                         const std::vector<int32_t> &cands, const std::vector<Camera> &cam_cands, int n1,
                                         const std::vector<int32_t> &mp1, const std::vector<std::vector<int32_t>> &mp2,
                                         const std::vector<std::vector<int32_t>> &idx2, bool fix_scale, uint64_t seed = 0,
                                         const std::vector<int32_t> &idx1 = {}, int nhyp = 300) {
        const size_t nc = cands.size(), cells = nc * (size_t)cap;
        const int words = (cap + 31) / 32;
        std::vector<afv_sim3_job> jobs(nc);
        std::vector<int32_t> slot_a(nc, cur), r1(cells, -1), r2(cells, -1), k1(cells, -1), k2(cells, -1);
        for (size_t c = 0; c < nc; ++c) {
            afv_sim3_job &j = jobs[c];
            std::memset(&j, 0, sizeof(j));
            j.struct_size = (uint32_t)sizeof(afv_sim3_job);
            j.fix_scale = fix_scale ? 1 : 0;
            const uint64_t s = seed + c;
            j.seed_lo = (uint32_t)s; j.seed_hi = (uint32_t)(s >> 32);
            std::memcpy(j.Rcw1, cam_cur.Rcw, sizeof(j.Rcw1)); std::memcpy(j.tcw1, cam_cur.tcw, sizeof(j.tcw1));
            std::memcpy(j.Rcw2, cam_cands[c].Rcw, sizeof(j.Rcw2)); std::memcpy(j.tcw2, cam_cands[c].tcw, sizeof(j.tcw2));
            j.fx1 = cam_cur.fx; j.fy1 = cam_cur.fy; j.cx1 = cam_cur.cx; j.cy1 = cam_cur.cy;
            j.fx2 = cam_cands[c].fx; j.fy2 = cam_cands[c].fy; j.cx2 = cam_cands[c].cx; j.cy2 = cam_cands[c].cy;
            for (int i = 0; i < n1 && i < cap; ++i) {
                const size_t o = c * (size_t)cap + (size_t)i;
                r1[o] = mp1[(size_t)i]; r2[o] = mp2[c][(size_t)i]; k2[o] = idx2[c][(size_t)i];
                k1[o] = idx1.empty() ? i : idx1[(size_t)i];
            }
        }
        std::vector<int32_t> n(nc), index1(cells), count(nc * (size_t)nhyp);
        std::vector<uint8_t> degenerate(nc * (size_t)nhyp);
        std::vector<float> sim3(nc * (size_t)nhyp * 13);
        std::vector<uint32_t> inliers(nc * (size_t)nhyp * (size_t)words);
        const int rc = afv_table_sim3_hypotheses(table, points.handle(), slot_a.data(), cands.data(), jobs.data(), (int)nc, r1.data(), r2.data(),
                                                 k1.data(), k2.data(), nhyp, words, n.data(), index1.data(), count.data(), degenerate.data(),
                                                 sim3.data(), inliers.data(), nullptr, nullptr, nullptr);
        if (rc != AFV_OK) fatal("afv_table_sim3_hypotheses", rc, ctx);
        std::vector<Sim3Solver> out;
        for (size_t c = 0; c < nc; ++c) {
            Sim3Solver s;
            s.N = n[c]; s.mN1 = n1; s.nhyp = nhyp; s.words = words;
            s.index1.assign(index1.begin() + (long)(c * (size_t)cap), index1.begin() + (long)(c * (size_t)cap) + s.N);
            s.count.assign(count.begin() + (long)(c * (size_t)nhyp), count.begin() + (long)((c + 1) * (size_t)nhyp));
            s.degenerate.assign(degenerate.begin() + (long)(c * (size_t)nhyp), degenerate.begin() + (long)((c + 1) * (size_t)nhyp));
            s.sim3.assign(sim3.begin() + (long)(c * (size_t)nhyp * 13), sim3.begin() + (long)((c + 1) * (size_t)nhyp * 13));
            s.inliers.assign(inliers.begin() + (long)(c * (size_t)nhyp * (size_t)words), inliers.begin() + (long)((c + 1) * (size_t)nhyp * (size_t)words));
            s.SetRansacParameters(0.99, 6, std::min(300, nhyp));  // :109, within what the device evaluated
            out.push_back(std::move(s));
        }
        return out;
    }

    // :112-136 (Q3).  false (nothing changes): maxIterations beyond the evaluated hypotheses, or minInliers < 3
    bool SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        if (maxIterations > nhyp || minInliers < 3) return false;
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        const float epsilon = (float)minInliers / (float)N;
        double v = 1.0;
        if (minInliers != N) v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
        // a double outside int's range is undefined in the reference: here it saturates and a NaN reads maxIterations
        int nIterations = maxIterations;
        if (v == v) nIterations = v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (-2147483647 - 1) : (int)v);
        mRansacMaxIts = std::max(1, std::min(nIterations, maxIterations));
        mnIterations = 0;
        return true;
    }

    // :138-204.  T12: 16 floats when the return value is true
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float *T12) {
        bNoMore = false;
        vbInliers.assign((size_t)mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return false;
        }
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            const int h = mnIterations++;
            const int c = count[(size_t)h];  // a degenerate hypothesis counts 0 and still advances mnIterations
            if (c >= mnBestInliers) {
                mnBestInliers = c;
                best = h;
                if (c > mRansacMinInliers) {
                    nInliers = c;
                    const uint32_t *w = inliers.data() + (size_t)h * (size_t)words;
                    for (int i = 0; i < N; ++i)
                        if ((w[i >> 5] >> (i & 31)) & 1u) vbInliers[(size_t)index1[(size_t)i]] = true;
                    const float *r = sim3.data() + (size_t)h * 13;
                    for (int a = 0; a < 3; ++a) {
                        for (int b = 0; b < 3; ++b) T12[4 * a + b] = r[12] * r[3 * a + b];  // mat3f sR = s12i * R12i
                        T12[4 * a + 3] = r[9 + a];
                    }
                    T12[12] = T12[13] = T12[14] = 0.0f;
                    T12[15] = 1.0f;
                    return true;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return false;
    }

    bool find(std::vector<bool> &vbInliers12, int &nInliers, float *T12) {  // :206-210
        bool flag;
        return iterate(mRansacMaxIts, flag, vbInliers12, nInliers, T12);
    }

    // the best hypothesis so far (best < 0: none yet)
    const float *GetEstimatedRotation() const { return best < 0 ? nullptr : sim3.data() + (size_t)best * 13; }
    const float *GetEstimatedTranslation() const { return best < 0 ? nullptr : sim3.data() + (size_t)best * 13 + 9; }
    float GetEstimatedScale() const { return best < 0 ? 0.0f : sim3[(size_t)best * 13 + 12]; }

    int N = 0, mN1 = 0, nhyp = 0, words = 0;
    int mnIterations = 0, mnBestInliers = 0, best = -1;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    double mRansacProb = 0.99;
    std::vector<int32_t> index1, count;   // mvnIndices1; inliers per hypothesis
    std::vector<uint8_t> degenerate;      // S5 flags per hypothesis
    std::vector<float> sim3;              // [nhyp][13]: R12 row-major, t12, s12
    std::vector<uint32_t> inliers;        // [nhyp][words]
};

// ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:1033-1226) as LoopClosing::ComputeSim3 calls it once a solver found a transform
// (src/LoopClosing.cc:342): OptimizeSim3Batch makes ONE afv_table_optimize_sim3 call for all candidates - the edge sets, both optimize()
// calls and both classifications of every job run on the device, one wavefront per job (include/afv_hip.h, "OptimizeSim3": deviations
// O1-O7).  The slots hold the keyframes' mvKeysUn (afv_table_set_geometry) and GetKeyPt2DInf (afv_table_set_inf, or a promoted frame).
struct Sim3d {  // g2o::Sim3 without the quaternion: R row-major, t, s
    double R[9], t[3], s;
};
struct OptimizeSim3Answer {
    int nInliers;               // what the reference returns
    Sim3d g2oS12;               // after the call (the start itself when the call answered 0 for want of correspondences)
    afv_sim3opt_result trace;   // counts, iterations, trials, chi2 and lambda of both optimize() calls
};
// cur / cands / cam_cur / cam_cands / n1 / mp1 / idx2: as Sim3Solver::Batch takes them; vpMatches1[c]: the matches of candidate c as point
// ids (-1 = none), n1 entries - on return -1 where the reference wrote NULL; start[c]: g2oS12 going in, rounded to float (what
// Sim3Solver::GetEstimated* return)
inline std::vector<OptimizeSim3Answer> OptimizeSim3Batch(afv_ctx *ctx, afv_table *table, int cap, DeviceMapPoints &points, int32_t cur,
                                                         const Sim3Solver::Camera &cam_cur, const std::vector<int32_t> &cands,
                                                         const std::vector<Sim3Solver::Camera> &cam_cands, int n1, const std::vector<int32_t> &mp1,
                                                         std::vector<std::vector<int32_t>> &vpMatches1, const std::vector<std::vector<int32_t>> &idx2,
                                                         const std::vector<Sim3d> &start, float th2, bool bFixScale) {
    const size_t nc = cands.size(), cells = nc * (size_t)cap;
    std::vector<afv_sim3opt_job> jobs(nc);
    std::vector<int32_t> slot_a(nc, cur), r1(cells, -1), r2(cells, -1), k2(cells, -1);
    for (size_t c = 0; c < nc; ++c) {
        afv_sim3opt_job &j = jobs[c];
        std::memset(&j, 0, sizeof(j));
        j.struct_size = (uint32_t)sizeof(afv_sim3opt_job);
        j.fix_scale = bFixScale ? 1 : 0;
        j.th2 = th2;
        std::memcpy(j.Rcw1, cam_cur.Rcw, sizeof(j.Rcw1)); std::memcpy(j.tcw1, cam_cur.tcw, sizeof(j.tcw1));
        std::memcpy(j.Rcw2, cam_cands[c].Rcw, sizeof(j.Rcw2)); std::memcpy(j.tcw2, cam_cands[c].tcw, sizeof(j.tcw2));
        j.fx1 = cam_cur.fx; j.fy1 = cam_cur.fy; j.cx1 = cam_cur.cx; j.cy1 = cam_cur.cy;
        j.fx2 = cam_cands[c].fx; j.fy2 = cam_cands[c].fy; j.cx2 = cam_cands[c].cx; j.cy2 = cam_cands[c].cy;
        for (int k = 0; k < 9; ++k) j.R12[k] = (float)start[c].R[k];
        for (int k = 0; k < 3; ++k) j.t12[k] = (float)start[c].t[k];
        j.s12 = (float)start[c].s;
        for (int i = 0; i < n1 && i < cap; ++i) {
            const size_t o = c * (size_t)cap + (size_t)i;
            r1[o] = mp1[(size_t)i]; r2[o] = vpMatches1[c][(size_t)i]; k2[o] = idx2[c][(size_t)i];
        }
    }
    std::vector<afv_sim3opt_result> res(nc);
    std::vector<uint8_t> state(cells);
    const int rc = afv_table_optimize_sim3(table, points.handle(), slot_a.data(), cands.data(), jobs.data(), (int)nc, r1.data(), r2.data(), k2.data(),
                                           res.data(), state.data());
    if (rc != AFV_OK) fatal("afv_table_optimize_sim3", rc, ctx);
    std::vector<OptimizeSim3Answer> out(nc);
    for (size_t c = 0; c < nc; ++c) {
        out[c].nInliers = res[c].n_in;
        std::memcpy(out[c].g2oS12.R, res[c].R12, sizeof(res[c].R12));
        std::memcpy(out[c].g2oS12.t, res[c].t12, sizeof(res[c].t12));
        out[c].g2oS12.s = res[c].s12;
        out[c].trace = res[c];
        for (int i = 0; i < n1 && i < cap; ++i) {
            const uint8_t st = state[c * (size_t)cap + (size_t)i];
            if (st == AFV_SIM3OPT_REMOVED_FIRST || st == AFV_SIM3OPT_REMOVED_SECOND) vpMatches1[c][(size_t)i] = -1;
        }
    }
    return out;
}
// the reference's call shape for one candidate: vpMatches1 and g2oS12 are updated in place, nIn is returned
inline int OptimizeSim3(afv_ctx *ctx, afv_table *table, int cap, DeviceMapPoints &points, int32_t cur, const Sim3Solver::Camera &cam_cur, int32_t cand,
                        const Sim3Solver::Camera &cam_cand, int n1, const std::vector<int32_t> &mp1, std::vector<int32_t> &vpMatches1,
                        const std::vector<int32_t> &idx2, Sim3d &g2oS12, float th2, bool bFixScale) {
    std::vector<std::vector<int32_t>> m{vpMatches1};
    const std::vector<OptimizeSim3Answer> a =
        OptimizeSim3Batch(ctx, table, cap, points, cur, cam_cur, {cand}, {cam_cand}, n1, mp1, m, {idx2}, {g2oS12}, th2, bFixScale);
    vpMatches1 = m[0];
    g2oS12 = a[0].g2oS12;
    return a[0].nInliers;
}

// ---- Optimizer::LocalBundleAdjustment (src/Optimizer.cc:450-768) and Optimizer::BundleAdjustment (:61-243): ONE afv_table_bundle_adjust
// call over slots of the keyframe table and ids of the map-point store (include/afv_hip.h, "Bundle adjustment": quirk L-Q1, deviations
// L1-L9).  The slots hold the keyframes' mvKeysUn, mvuRight and GetKeyPt2DInf.  What stays with the host's map after a call:
// EraseMapPointMatch / EraseObservation for every pair of vToErase and SetPose from `poses`; UpdateNormalAndDepth of the moved points is
// RefreshAfterBundleAdjustment below, on the device.
struct BundleKeyFrame {  // a keyframe of the problem: its slot, whether its vertex is fixed (keyId == 0, lFixedCameras), GetPose(), intrinsics
    int32_t slot;
    bool fixed;
    float Rcw[9], tcw[3], fx, fy, cx, cy, mbf;
};
struct BundleObservation {  // pMP->GetObservations(): point id, keyframe slot, feature index - in the reference's order
    int32_t point, slot, idx;
};
struct Pose3d {  // g2o::SE3Quat without the quaternion: R row-major, t
    double R[9], t[3];
};
struct BundleAnswer {
    std::vector<std::pair<int32_t, Pose3d>> poses;          // (slot, pose) of every optimised keyframe, in the caller's order
    std::vector<double> xyz;                                // [np][3]; the store holds the float cast when write_points
    std::vector<std::pair<int32_t, int32_t>> vToErase;      // (slot, point id)
    std::vector<uint8_t> edge_state;                        // AFV_LBA_EDGE_* per observation
    afv_lba_result trace;
};
inline BundleAnswer BundleAdjust(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<BundleKeyFrame> &kfs,
                                 const std::vector<int32_t> &point_ids, const std::vector<BundleObservation> &observations, int it0, int it1,
                                 bool robust0, bool robust1, bool checks, bool write_points, const volatile int32_t *pbStopFlag,
                                 bool block_sparse = false) {  // true: afv_table_global_bundle_adjust (its own caps, deviation L7')
    std::vector<size_t> order;  // free keyframes first, each group in the caller's order
    for (size_t k = 0; k < kfs.size(); ++k)
        if (!kfs[k].fixed) order.push_back(k);
    const int n_free = (int)order.size();
    for (size_t k = 0; k < kfs.size(); ++k)
        if (kfs[k].fixed) order.push_back(k);
    std::vector<int32_t> slots(std::max<size_t>(kfs.size(), 1), 0);
    std::vector<afv_lba_cam> cams(std::max<size_t>(kfs.size(), 1));
    std::map<int32_t, int32_t> where_k, where_p;
    for (size_t i = 0; i < order.size(); ++i) {
        const BundleKeyFrame &K = kfs[order[i]];
        slots[i] = K.slot;
        where_k[K.slot] = (int32_t)i;
        afv_lba_cam &c = cams[i];
        std::memset(&c, 0, sizeof(c));
        c.struct_size = (uint32_t)sizeof(afv_lba_cam);
        std::memcpy(c.Rcw, K.Rcw, sizeof(c.Rcw)); std::memcpy(c.tcw, K.tcw, sizeof(c.tcw));
        c.fx = K.fx; c.fy = K.fy; c.cx = K.cx; c.cy = K.cy; c.bf = K.mbf;
    }
    for (size_t p = 0; p < point_ids.size(); ++p) where_p[point_ids[p]] = (int32_t)p;
    // the edges grouped by point in the order of point_ids; the observations of a point keep their order
    std::vector<size_t> eo(observations.size());
    for (size_t e = 0; e < eo.size(); ++e) eo[e] = e;
    std::vector<int32_t> pos_p(observations.size()), pos_k(observations.size());
    for (size_t e = 0; e < observations.size(); ++e) {
        const auto ip = where_p.find(observations[e].point);
        const auto ik = where_k.find(observations[e].slot);
        if (ip == where_p.end() || ik == where_k.end()) fatal("BundleAdjust: an observation names a point or keyframe outside the problem", AFV_EINVAL, ctx);
        pos_p[e] = ip->second;
        pos_k[e] = ik->second;
    }
    std::stable_sort(eo.begin(), eo.end(), [&](size_t a, size_t b) { return pos_p[a] < pos_p[b]; });
    const size_t ne = observations.size(), np = point_ids.size();
    std::vector<int32_t> op(std::max<size_t>(ne, 1), 0), ok(std::max<size_t>(ne, 1), 0), oi(std::max<size_t>(ne, 1), 0), ids(std::max<size_t>(np, 1), 0);
    for (size_t e = 0; e < ne; ++e) { op[e] = pos_p[eo[e]]; ok[e] = pos_k[eo[e]]; oi[e] = observations[eo[e]].idx; }
    std::copy(point_ids.begin(), point_ids.end(), ids.begin());
    afv_lba_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.struct_size = (uint32_t)sizeof(afv_lba_params);
    prm.iterations[0] = it0; prm.iterations[1] = it1; prm.robust[0] = robust0 ? 1 : 0; prm.robust[1] = robust1 ? 1 : 0;
    prm.checks = checks ? 1 : 0; prm.write_points = write_points ? 1 : 0;
    BundleAnswer A;
    std::memset(&A.trace, 0, sizeof(A.trace));
    std::vector<double> kf((size_t)std::max(n_free, 1) * 12, 0.0);
    std::vector<uint8_t> state(std::max<size_t>(ne, 1), 0);
    A.xyz.assign(std::max<size_t>(np, 1) * 3, 0.0);
    const int rc = (block_sparse ? afv_table_global_bundle_adjust : afv_table_bundle_adjust)(
        table, points.handle(), slots.data(), (int)kfs.size(), n_free, cams.data(), ids.data(), (int)np, op.data(), ok.data(), oi.data(), (int)ne, &prm,
        pbStopFlag, &A.trace, kf.data(), A.xyz.data(), state.data());
    if (rc != AFV_OK) fatal(block_sparse ? "afv_table_global_bundle_adjust" : "afv_table_bundle_adjust", rc, ctx);
    A.xyz.resize(np * 3);
    A.edge_state.assign(ne, 0);
    if (A.trace.stopped == 1) return A;  // the return at :645-647: nothing was written
    for (int i = 0; i < n_free; ++i) {
        Pose3d P;
        std::memcpy(P.R, kf.data() + (size_t)i * 12, sizeof(P.R));
        std::memcpy(P.t, kf.data() + (size_t)i * 12 + 9, sizeof(P.t));
        A.poses.emplace_back(slots[(size_t)i], P);
    }
    for (size_t e = 0; e < ne; ++e) A.edge_state[eo[e]] = state[e];
    for (size_t e = 0; e < ne; ++e)
        if (A.edge_state[e] == AFV_LBA_EDGE_ERASE) A.vToErase.emplace_back(observations[e].slot, observations[e].point);
    return A;
}
// the reference's call shapes.  kfs: lLocalKeyFrames then lFixedCameras (fixed = true for keyId == 0 and every fixed camera)
inline BundleAnswer LocalBundleAdjustment(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<BundleKeyFrame> &kfs,
                                          const std::vector<int32_t> &point_ids, const std::vector<BundleObservation> &observations,
                                          const volatile int32_t *pbStopFlag = nullptr) {
    return BundleAdjust(ctx, table, points, kfs, point_ids, observations, 5, 10, true, false, true, true, pbStopFlag);
}
// write_points = false is the nLoopKF != 0 path: the caller keeps xyz as mPosGBA and the poses as mTcwGBA, the store stays
inline BundleAnswer BundleAdjustment(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<BundleKeyFrame> &kfs,
                                     const std::vector<int32_t> &point_ids, const std::vector<BundleObservation> &observations, int nIterations = 5,
                                     const volatile int32_t *pbStopFlag = nullptr, bool bRobust = true, bool write_points = true) {
    return BundleAdjust(ctx, table, points, kfs, point_ids, observations, nIterations, 0, bRobust, false, false, write_points, pbStopFlag);
}
// Optimizer::GlobalBundleAdjustemnt (Optimizer.cc:53-58; defaults: Optimizer.h:42-43) over the whole map on the block-sparse route: up to
// AFV_GBA_MAX_KF keyframes, every one free except keyId == 0.  LoopClosing::RunGlobalBundleAdjustment passes (10, &mbStopGBA, false) and
// write_points = false, keeps xyz as mPosGBA and the poses as mTcwGBA, and moves the points the BA did not optimise with CorrectPointsSE3
inline BundleAnswer GlobalBundleAdjustment(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<BundleKeyFrame> &kfs,
                                           const std::vector<int32_t> &point_ids, const std::vector<BundleObservation> &observations, int nIterations = 5,
                                           const volatile int32_t *pbStopFlag = nullptr, bool bRobust = true, bool write_points = true) {
    return BundleAdjust(ctx, table, points, kfs, point_ids, observations, nIterations, 0, bRobust, false, false, write_points, pbStopFlag, true);
}
struct SE3f {  // 12 floats: R row-major, t
    float R[9], t[3];
};
// LoopClosing.cc:731-750 for the points the global BA did not optimise, in float, in the store, in place: Tcw_before[q] = mTcwBefGBA of
// reference keyframe q, Twc_after[q] = its GetPoseInverse() after SetPose(TcwGBA); pair_of_point[i] names the pair of point i, -1 none
inline std::vector<uint8_t> CorrectPointsSE3(afv_ctx *ctx, DeviceMapPoints &points, const std::vector<int32_t> &ids, const std::vector<int32_t> &pair_of_point,
                                             const std::vector<SE3f> &Tcw_before, const std::vector<SE3f> &Twc_after) {
    static_assert(sizeof(SE3f) == 48, "SE3f is 12 floats");
    if (pair_of_point.size() != ids.size() || Tcw_before.size() != Twc_after.size()) fatal("CorrectPointsSE3: mismatched arrays", AFV_EINVAL, ctx);
    std::vector<uint8_t> status(std::max<size_t>(ids.size(), 1), 0);
    const int rc = afv_points_correct_se3(points.handle(), ids.data(), (int)ids.size(), pair_of_point.data(), reinterpret_cast<const float *>(Tcw_before.data()),
                                          reinterpret_cast<const float *>(Twc_after.data()), (int)Tcw_before.size(), status.data());
    if (rc != AFV_OK) fatal("afv_points_correct_se3", rc, ctx);
    status.resize(ids.size());
    return status;
}

// ---- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:279-349) and MapPoint::UpdateNormalAndDepth (:372-418) of resident points:
// ONE afv_table_refresh_points call over the observation list of the bundle adjustment (include/afv_hip.h, "Refresh of resident map
// points": deviations R1-R3).  What stays with the host's map after a call: refKeyframe / refIndex of every point, from best_obs.
struct RefreshKeyFrame {  // a keyframe some observation names: its slot, GetCameraCenter(), maxKeyPtSize, isBad()
    int32_t slot;
    float centre[3], maxKeyPtSize;
    bool bad;
};
struct RefreshAnswer {
    std::vector<int32_t> status;       // AFV_REFRESH_* per point
    std::vector<int32_t> best_obs;     // the index into `observations` of the winning row | -1
    std::vector<int32_t> best_median;  // an int for binary tables, the bits of the float for float tables
};
// ref_slot[p]: the slot of mpRefKF of point_ids[p] | -1
inline RefreshAnswer RefreshMapPoints(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<RefreshKeyFrame> &kfs,
                                      const std::vector<int32_t> &point_ids, const std::vector<int32_t> &ref_slot,
                                      const std::vector<BundleObservation> &observations, bool descriptors = true, bool normals = true) {
    const size_t nk = kfs.size(), np = point_ids.size(), ne = observations.size();
    if (ref_slot.size() != np) fatal("RefreshMapPoints: one ref keyframe per point is expected", AFV_EINVAL, ctx);
    std::vector<int32_t> slots(std::max<size_t>(nk, 1), 0), ids(std::max<size_t>(np, 1), 0), ref(std::max<size_t>(np, 1), -1);
    std::vector<float> centres(std::max<size_t>(nk, 1) * 3, 0.0f), max_size(std::max<size_t>(nk, 1), 1.0f);
    std::vector<uint8_t> bad(std::max<size_t>(nk, 1), 0);
    std::map<int32_t, int32_t> where_k, where_p;
    for (size_t k = 0; k < nk; ++k) {
        slots[k] = kfs[k].slot;
        where_k[kfs[k].slot] = (int32_t)k;
        std::memcpy(&centres[3 * k], kfs[k].centre, sizeof(kfs[k].centre));
        max_size[k] = kfs[k].maxKeyPtSize;
        bad[k] = kfs[k].bad ? 1 : 0;
    }
    for (size_t p = 0; p < np; ++p) {
        ids[p] = point_ids[p];
        where_p[point_ids[p]] = (int32_t)p;
        const auto ik = where_k.find(ref_slot[p]);
        ref[p] = ik == where_k.end() ? -1 : ik->second;
    }
    // the observations grouped by point in the order of point_ids; the observations of a point keep their order
    std::vector<size_t> eo(ne);
    for (size_t e = 0; e < ne; ++e) eo[e] = e;
    std::vector<int32_t> pos_p(ne), pos_k(ne);
    for (size_t e = 0; e < ne; ++e) {
        const auto ip = where_p.find(observations[e].point);
        const auto ik = where_k.find(observations[e].slot);
        if (ip == where_p.end() || ik == where_k.end()) fatal("RefreshMapPoints: an observation names a point or keyframe outside the call", AFV_EINVAL, ctx);
        pos_p[e] = ip->second;
        pos_k[e] = ik->second;
    }
    std::stable_sort(eo.begin(), eo.end(), [&](size_t a, size_t b) { return pos_p[a] < pos_p[b]; });
    std::vector<int32_t> op(std::max<size_t>(ne, 1), 0), ok(std::max<size_t>(ne, 1), 0), oi(std::max<size_t>(ne, 1), 0);
    for (size_t e = 0; e < ne; ++e) { op[e] = pos_p[eo[e]]; ok[e] = pos_k[eo[e]]; oi[e] = observations[eo[e]].idx; }
    RefreshAnswer A;
    A.status.assign(std::max<size_t>(np, 1), 0);
    A.best_obs.assign(std::max<size_t>(np, 1), -1);
    A.best_median.assign(std::max<size_t>(np, 1), 0);
    afv_refresh_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.struct_size = (uint32_t)sizeof(prm);
    prm.descriptors = descriptors ? 1 : 0;
    prm.normals = normals ? 1 : 0;
    afv_refresh_out out;
    std::memset(&out, 0, sizeof(out));
    out.struct_size = (uint32_t)sizeof(out);
    out.status = A.status.data(); out.best_obs = A.best_obs.data(); out.best_median = A.best_median.data();
    const int rc = afv_table_refresh_points(table, points.handle(), slots.data(), (int)nk, centres.data(), max_size.data(), bad.data(), ids.data(), (int)np,
                                            ref.data(), op.data(), ok.data(), oi.data(), (int)ne, &prm, &out);
    if (rc != AFV_OK) fatal("afv_table_refresh_points", rc, ctx);
    A.status.resize(np); A.best_obs.resize(np); A.best_median.resize(np);
    for (int32_t &b : A.best_obs)
        if (b >= 0) b = (int32_t)eo[(size_t)b];
    return A;
}
// GetCameraCenter() after KeyFrame::SetPose (src/KeyFrame.cc:81-84): twc = -Rwc * tcw in float, a0 + (a1 + a2)
inline void CameraCentre(const float *Rcw, const float *tcw, float *centre) {
    for (int k = 0; k < 3; ++k) centre[k] = -Rcw[k] * tcw[0] + (-Rcw[3 + k] * tcw[1] + -Rcw[6 + k] * tcw[2]);
}
// What Optimizer::LocalBundleAdjustment / BundleAdjustment do after the write-back (Optimizer.cc:753-767, :207-234): `answer` is what
// afv::LocalBundleAdjustment returned for `kfs`; an optimised keyframe's centre is formed from the float cast of its new pose
// (Converter::toMatrix4f, then SetPose), a fixed one's from the pose it was given.  maxKeyPtSize[k] / bad[k] belong to kfs[k] (bad may be
// empty).  The normal part alone unless descriptors is set.
inline RefreshAnswer RefreshAfterBundleAdjustment(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<BundleKeyFrame> &kfs,
                                                  const BundleAnswer &answer, const std::vector<float> &maxKeyPtSize, const std::vector<uint8_t> &bad,
                                                  const std::vector<int32_t> &point_ids, const std::vector<int32_t> &ref_slot,
                                                  const std::vector<BundleObservation> &observations, bool descriptors = false) {
    if (maxKeyPtSize.size() != kfs.size()) fatal("RefreshAfterBundleAdjustment: one maxKeyPtSize per keyframe is expected", AFV_EINVAL, ctx);
    std::vector<RefreshKeyFrame> rk(kfs.size());
    for (size_t k = 0; k < kfs.size(); ++k) {
        float R[9], t[3];
        std::memcpy(R, kfs[k].Rcw, sizeof(R));
        std::memcpy(t, kfs[k].tcw, sizeof(t));
        for (const auto &moved : answer.poses)
            if (moved.first == kfs[k].slot) {
                for (int q = 0; q < 9; ++q) R[q] = (float)moved.second.R[q];
                for (int q = 0; q < 3; ++q) t[q] = (float)moved.second.t[q];
            }
        rk[k].slot = kfs[k].slot;
        CameraCentre(R, t, rk[k].centre);
        rk[k].maxKeyPtSize = maxKeyPtSize[k];
        rk[k].bad = k < bad.size() && bad[k] != 0;
    }
    return RefreshMapPoints(ctx, table, points, rk, point_ids, ref_slot, observations, descriptors, true);
}

// ---- PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) as Tracking::Relocalization uses it (src/Tracking.cc:1190-1216): Batch makes ONE
// afv_frame_pnp_hypotheses call for all candidates of a relocalisation - every solver's constructor, every EPnP RANSAC hypothesis and the
// Refine of every record run on the device (include/afv_hip.h, "PnPsolver": quirks Q1-Q6, deviations E1-E10) - and returns one solver per
// candidate.  iterate / find are host code over the per-hypothesis counts, poses and inlier words: hypothesis h depends on (seed, h) alone
// and Refine reads only the best set, which changes only at a record, so the reference's sequential rule is a scan.  Tcw is 16 floats
// row-major (cv::Mat 4 x 4 CV_32F in the reference).
class PnPsolver {
  public:
    // F: the current frame with its features and a pose (the intrinsics are the frame's); pts[c]: vvpMapPointMatches of candidate c as
    // point ids, one per feature of F, -1 = none; minInliers / epsilon / th2: what SetRansacParameters will be given; candidate c draws
    // from seed + c
    static std::vector<PnPsolver> Batch(afv_ctx *ctx, DeviceFrame &F, int nf, DeviceMapPoints &points, const std::vector<std::vector<int32_t>> &pts,
                                        uint64_t seed = 0, int nhyp = 300, int minInliers = 10, float epsilon = 0.5f, float th2 = 5.991f) {
        const size_t nc = pts.size(), cells = nc * (size_t)nf, hyps = nc * (size_t)nhyp;
        const int words = (nf + 31) / 32;
        std::vector<afv_pnp_job> jobs(nc);
        std::vector<int32_t> rows(cells, -1);
        for (size_t c = 0; c < nc; ++c) {
            afv_pnp_job &j = jobs[c];
            std::memset(&j, 0, sizeof(j));
            j.struct_size = (uint32_t)sizeof(afv_pnp_job);
            const uint64_t s = seed + c;
            j.seed_lo = (uint32_t)s; j.seed_hi = (uint32_t)(s >> 32);
            j.min_inliers = minInliers; j.epsilon = epsilon; j.th2 = th2;
            for (int i = 0; i < nf; ++i) rows[c * (size_t)nf + (size_t)i] = pts[c][(size_t)i];
        }
        std::vector<int32_t> n(nc), nmin(nc), index(cells), count(hyps), rcount(hyps);
        std::vector<uint8_t> degenerate(hyps), refined(hyps);
        std::vector<float> pose(hyps * 12), rpose(hyps * 12);
        std::vector<uint32_t> inliers(hyps * (size_t)words), rinliers(hyps * (size_t)words);
        const int rc = afv_frame_pnp_hypotheses(F.handle(), points.handle(), jobs.data(), (int)nc, rows.data(), nhyp, words, n.data(), nmin.data(),
                                                index.data(), count.data(), degenerate.data(), pose.data(), inliers.data(), refined.data(),
                                                rcount.data(), rpose.data(), rinliers.data(), nullptr, nullptr);
        if (rc != AFV_OK) fatal("afv_frame_pnp_hypotheses", rc, ctx);
        std::vector<PnPsolver> out;
        for (size_t c = 0; c < nc; ++c) {
            PnPsolver s;
            s.N = n[c]; s.nf = nf; s.nhyp = nhyp; s.words = words; s.device_min_inliers = nmin[c];
            s.given_min = minInliers; s.given_eps = epsilon; s.given_th2 = th2;
            const long h0 = (long)(c * (size_t)nhyp), h1 = (long)((c + 1) * (size_t)nhyp);
            s.index.assign(index.begin() + (long)(c * (size_t)nf), index.begin() + (long)(c * (size_t)nf) + s.N);
            s.count.assign(count.begin() + h0, count.begin() + h1);
            s.degenerate.assign(degenerate.begin() + h0, degenerate.begin() + h1);
            s.refined.assign(refined.begin() + h0, refined.begin() + h1);
            s.refined_count.assign(rcount.begin() + h0, rcount.begin() + h1);
            s.pose.assign(pose.begin() + h0 * 12, pose.begin() + h1 * 12);
            s.refined_pose.assign(rpose.begin() + h0 * 12, rpose.begin() + h1 * 12);
            s.inliers.assign(inliers.begin() + h0 * words, inliers.begin() + h1 * words);
            s.refined_inliers.assign(rinliers.begin() + h0 * words, rinliers.begin() + h1 * words);
            if (!s.SetRansacParameters(0.99, minInliers, std::min(300, nhyp), 4, epsilon, th2))
                fatal("PnPsolver::Batch: the device's mRansacMinInliers is not the host's", AFV_EINVAL, ctx);
            out.push_back(std::move(s));
        }
        return out;
    }

    // :121-157 (Q2): host mathematics only.  false (nothing changes): minInliers, epsilon or th2 differ from what the device call was
    // given, minSet != 4, or maxIterations beyond the evaluated hypotheses
    bool SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                             float th2 = 5.991f) {
        if (minInliers != given_min || epsilon != given_eps || th2 != given_th2 || minSet != 4 || maxIterations > nhyp) return false;
        const float prod = (float)N * epsilon;  // :134, the product in float, truncated
        int nMinInliers = !(prod < 2147483648.0f) ? 2147483647 : (int)prod;
        nMinInliers = std::max(std::max(nMinInliers, minInliers), minSet);
        if (nMinInliers != device_min_inliers) return false;
        mRansacProb = probability;
        mRansacMinInliers = nMinInliers;
        mRansacEpsilon = epsilon;
        if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
        double v = 1.0;
        if (mRansacMinInliers != N) v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)mRansacEpsilon, 3.0)));
        // a double outside int's range is undefined in the reference: here it saturates and a NaN reads maxIterations
        nIterationsWanted = maxIterations;
        if (v == v) nIterationsWanted = v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (-2147483647 - 1) : (int)v);
        mRansacMaxIts = std::max(1, std::min(nIterationsWanted, maxIterations));
        return true;
    }

    // :165-258.  Tcw: 16 floats when the return value is true.  A scan that would visit a hypothesis the device did not evaluate is fatal
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float *Tcw) {
        bNoMore = false;
        vbInliers.assign((size_t)nf, false);
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return false;
        }
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {  // Q1
            if (mnIterations >= nhyp) fatal("PnPsolver::iterate: a hypothesis the device did not evaluate", AFV_EINVAL, nullptr);
            nCurrentIterations++;
            const int h = mnIterations++;
            const int c = count[(size_t)h];  // a degenerate hypothesis counts 0 and still advances mnIterations
            if (c >= mRansacMinInliers) {
                if (c > mnBestInliers) {  // a record
                    mnBestInliers = c;
                    best = h;
                }
                // Q4: Refine on the best set so far; the device evaluated it at the record
                if (refined[(size_t)best] == 1 && refined_count[(size_t)best] > mRansacMinInliers) {
                    answer(refined_pose.data() + (size_t)best * 12, refined_inliers.data() + (size_t)best * (size_t)words, vbInliers, Tcw);
                    nInliers = refined_count[(size_t)best];
                    return true;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) {
            bNoMore = true;
            if (mnBestInliers >= mRansacMinInliers) {  // Q3: the unrefined best
                answer(pose.data() + (size_t)best * 12, inliers.data() + (size_t)best * (size_t)words, vbInliers, Tcw);
                nInliers = mnBestInliers;
                return true;
            }
        }
        return false;
    }

    bool find(std::vector<bool> &vbInliers, int &nInliers, float *Tcw) {  // :159-163
        bool flag;
        return iterate(mRansacMaxIts, flag, vbInliers, nInliers, Tcw);
    }

    int N = 0, nf = 0, nhyp = 0, words = 0, device_min_inliers = 0;
    int mnIterations = 0, mnBestInliers = 0, best = -1;
    int mRansacMinInliers = 8, mRansacMaxIts = 300, nIterationsWanted = 0;
    double mRansacProb = 0.99;
    float mRansacEpsilon = 0.4f;
    std::vector<int32_t> index, count, refined_count;  // mvKeyPointIndices; inliers per hypothesis; of its refinement
    std::vector<uint8_t> degenerate, refined;          // E8 flags; 0 no record, 1 refined, 2 record whose refinement is degenerate
    std::vector<float> pose, refined_pose;             // [nhyp][12]: Rcw row-major, tcw
    std::vector<uint32_t> inliers, refined_inliers;    // [nhyp][words]

  private:
    void answer(const float *p, const uint32_t *w, std::vector<bool> &vbInliers, float *Tcw) const {
        for (int i = 0; i < N; ++i)
            if ((w[i >> 5] >> (i & 31)) & 1u) vbInliers[(size_t)index[(size_t)i]] = true;
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) Tcw[4 * a + b] = p[3 * a + b];
            Tcw[4 * a + 3] = p[9 + a];
        }
        Tcw[12] = Tcw[13] = Tcw[14] = 0.0f;
        Tcw[15] = 1.0f;
    }
    int given_min = 0;
    float given_eps = 0.0f, given_th2 = 0.0f;
};

// ---- Initializer (include/Initializer.h, src/Initializer.cc) as Tracking::MonocularInitialization uses it (src/Tracking.cc:455, :487):
// built on the reference frame, asked once per current frame with the matches of SearchForInitialization.  Initialize makes ONE
// afv_frame_initializer call - the H and F RANSAC over all iterations, the selection, the motion hypotheses and CheckRT run on the device
// (include/afv_hip.h, "Initializer": the quirks, deviations I1-I11) - and returns what the reference returns.  The reference's constructor
// reads K from the frame; a DeviceFrame does not hold K, so it is handed over.  R21 is 9 floats row-major, t21 3 floats (mat3f / vec3f in
// the reference), a point of vP3D 3 floats.
class Initializer {
  public:
    Initializer(DeviceFrame &ReferenceFrame, float fx, float fy, float cx, float cy, float sigma = 1.0f, int iterations = 200, uint64_t seed = 0)
        : ref(ReferenceFrame) {
        std::memset(&job, 0, sizeof(job));
        job.struct_size = (uint32_t)sizeof(afv_init_job);
        job.iterations = iterations;
        job.seed_lo = (uint32_t)seed; job.seed_hi = (uint32_t)(seed >> 32);
        job.fx = fx; job.fy = fy; job.cx = cx; job.cy = cy; job.sigma = sigma;
        std::memset(&trace, 0, sizeof(trace));
    }

    // :41-114.  vMatches12: one entry per feature of the reference frame (the current frame's feature | -1).  vP3D / vbTriangulated get one
    // entry per feature of the reference frame; on false they read 0 / false (the reference leaves them untouched)
    bool Initialize(DeviceFrame &CurrentFrame, const std::vector<int> &vMatches12, float (&R21)[9], float (&t21)[3],
                    std::vector<std::array<float, 3>> &vP3D, std::vector<bool> &vbTriangulated) {
        const size_t n1 = vMatches12.size();
        std::vector<int32_t> m(vMatches12.begin(), vMatches12.end());
        std::vector<float> p3d(3 * std::max<size_t>(n1, 1));
        std::vector<uint8_t> tri(std::max<size_t>(n1, 1));
        int32_t ok = 0;
        trace.struct_size = (uint32_t)sizeof(afv_init_trace);
        const int rc = afv_frame_initializer(ref.handle(), CurrentFrame.handle(), &job, m.data(), &ok, &route, R21, t21, p3d.data(), tri.data(),
                                             &trace, nullptr, nullptr, nullptr, nullptr, 0);
        if (rc != AFV_OK) fatal("afv_frame_initializer", rc, nullptr);
        vP3D.resize(n1);
        vbTriangulated.assign(n1, false);
        for (size_t i = 0; i < n1; ++i) {
            vP3D[i] = {p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]};
            vbTriangulated[i] = tri[i] != 0;
        }
        return ok != 0;
    }

    afv_init_job job;      // iterations, seed, K, sigma: change between calls at will
    afv_init_trace trace;  // what the last Initialize decided on the way (cosines, not degrees: I6)
    int32_t route = AFV_INIT_ROUTE_F;

  private:
    DeviceFrame &ref;
};

// ---- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:771-1031) and the point correction of LoopClosing::CorrectLoop
// (LoopClosing.cc:487-516): ONE afv_essential_graph / afv_points_correct_sim3 call each (include/afv_hip.h, "Essential graph": quirk G-Q1,
// deviations G1-G11).  The caller lists the keyframes that are not bad in ascending keyId and the edges in the reference's order (:835-971);
// what stays with the host's map: SetPose from Tiw (the float cast), UpdateNormalAndDepth of the moved points (RefreshMapPoints).
struct EssentialGraphEdge {
    int32_t v0, v1;        // positions in the keyframe list; v0 the vertex of setVertex(0, ...)
    afv_sim3d measurement; // Sji
};
struct EssentialGraphAnswer {
    std::vector<afv_sim3d> CorrectedSiw;  // the optimised estimate of every keyframe
    std::vector<double> Tiw;              // [nk][12]: R row-major, t / s
    std::vector<double> xyz;              // [np][3]; the store holds the float cast when write_points
    std::vector<uint8_t> point_status;    // AFV_POINT_*
    afv_ess_result trace;
};
// points may be nullptr when no point is corrected.  S_init: CorrectedSim3 of a keyframe or (Rcw, tcw, 1); fixed: the position of pLoopKF;
// point_ref: per point the position of mnCorrectedReference (mnCorrectedByKF == pCurKF) or of mpRefKF in the keyframe list, -1 for none
inline EssentialGraphAnswer OptimizeEssentialGraph(afv_ctx *ctx, DeviceMapPoints *points, const std::vector<afv_sim3d> &S_init, int fixed,
                                                   const std::vector<EssentialGraphEdge> &edges, bool bFixScale, const std::vector<int32_t> &point_ids,
                                                   const std::vector<int32_t> &point_ref, int nIterations = 20, double userLambdaInit = 1e-16,
                                                   bool write_points = true) {
    const size_t nk = S_init.size(), ne = edges.size(), np = point_ids.size();
    if (point_ref.size() != np) fatal("OptimizeEssentialGraph: one reference per point is expected", AFV_EINVAL, ctx);
    std::vector<int32_t> v0(std::max<size_t>(ne, 1), 0), v1(std::max<size_t>(ne, 1), 0);
    std::vector<afv_sim3d> meas(std::max<size_t>(ne, 1));
    for (size_t e = 0; e < ne; ++e) { v0[e] = edges[e].v0; v1[e] = edges[e].v1; meas[e] = edges[e].measurement; }
    afv_ess_params prm;
    std::memset(&prm, 0, sizeof(prm));
    prm.struct_size = (uint32_t)sizeof(afv_ess_params);
    prm.iterations = nIterations; prm.lambda_init = userLambdaInit; prm.fix_scale = bFixScale ? 1 : 0; prm.write_points = write_points ? 1 : 0;
    EssentialGraphAnswer A;
    std::memset(&A.trace, 0, sizeof(A.trace));
    A.CorrectedSiw.resize(std::max<size_t>(nk, 1));
    A.Tiw.assign(std::max<size_t>(nk, 1) * 12, 0.0);
    A.xyz.assign(std::max<size_t>(np, 1) * 3, 0.0);
    A.point_status.assign(std::max<size_t>(np, 1), 0);
    const int rc = afv_essential_graph(ctx, points ? points->handle() : nullptr, S_init.data(), (int)nk, fixed, v0.data(), v1.data(), meas.data(), (int)ne,
                                       &prm, point_ids.data(), point_ref.data(), (int)np, &A.trace, A.CorrectedSiw.data(), A.Tiw.data(), A.xyz.data(),
                                       A.point_status.data());
    if (rc != AFV_OK) fatal("afv_essential_graph", rc, ctx);
    A.CorrectedSiw.resize(nk); A.Tiw.resize(nk * 12); A.xyz.resize(np * 3); A.point_status.resize(np);
    return A;
}
// CorrectedSwi.map(Siw.map(P)) of every listed point in the store, in place: pair_of_point[i] names the (S_from, S_to) pair of point i, -1 none
inline std::vector<uint8_t> CorrectPointsSim3(afv_ctx *ctx, DeviceMapPoints &points, const std::vector<int32_t> &ids, const std::vector<int32_t> &pair_of_point,
                                              const std::vector<afv_sim3d> &S_from, const std::vector<afv_sim3d> &S_to) {
    if (pair_of_point.size() != ids.size() || S_from.size() != S_to.size()) fatal("CorrectPointsSim3: mismatched arrays", AFV_EINVAL, ctx);
    std::vector<uint8_t> status(std::max<size_t>(ids.size(), 1), 0);
    const int rc = afv_points_correct_sim3(points.handle(), ids.data(), (int)ids.size(), pair_of_point.data(), S_from.data(), S_to.data(), (int)S_from.size(),
                                           status.data());
    if (rc != AFV_OK) fatal("afv_points_correct_sim3", rc, ctx);
    status.resize(ids.size());
    return status;
}

// ---- FeatureMatcher::Fuse into keyframes of the table (include/afv_hip.h afv_table_fuse_points; reference: FeatureMatcher.cc:794-940,
// :942-1064 as LocalMapping::SearchInNeighbors and LoopClosing::SearchAndFuse call them).  The slots carry the table's camera
// (afv_table_set_camera), KeyFrame::SetPose (afv_table_set_pose) and mvpMapPoints (afv_table_set_map_points): INTEGRATION.md, "Fusing into
// keyframes".  Every target is answered against the store and the planes AS THEY STAND: AddObservation (status 4), Replace (status 6) and
// ComputeDistinctiveDescriptors stay with the caller; one target per call with the map updated in between is the reference's loop. ----
struct FuseTarget {
    int32_t slot;
    const std::vector<int32_t> *ids;  // the points in the reference's iteration order, -1 allowed; targets naming ONE vector share its gather
};
struct FuseAnswer {  // per target, over its queries
    std::vector<std::vector<int32_t>> best, occupant;  // the winning feature | -1; the point id the keyframe holds there | -1
    std::vector<std::vector<uint8_t>> status;          // 0 .. 6, see afv_table_fuse_points
    std::vector<int32_t> nFused;                        // what Fuse returns
};
inline FuseAnswer FuseRun(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<FuseTarget> &targets, float radiusTh, float th_low,
                          bool use_inf_gate, const std::vector<afv_table_fuse_pose> *poses) {
    const size_t nt = targets.size();
    if (poses && poses->size() != nt) fatal("Fuse: one Scw per target", AFV_EINVAL, ctx);
    std::vector<afv_table_fuse_job> jobs(std::max<size_t>(nt, 1));
    size_t total = 0;
    for (size_t k = 0; k < nt; ++k) {
        afv_table_fuse_job &j = jobs[k];
        j = afv_table_fuse_job{};
        j.struct_size = (uint32_t)sizeof(j);
        j.slot = targets[k].slot;
        j.ids = targets[k].ids->data();
        j.nq = (int32_t)targets[k].ids->size();
        j.radius_th = radiusTh; j.radius_scale = 1.15f; j.th_low = th_low;  // FeatureMatcher's static radiusScale
        j.use_inf_gate = use_inf_gate ? 1 : 0;
        j.pose_override = poses ? &(*poses)[k] : nullptr;
        total += targets[k].ids->size();
    }
    std::vector<int32_t> best(std::max<size_t>(total, 1), -1), occ(std::max<size_t>(total, 1), -1), nf(std::max<size_t>(nt, 1), 0);
    std::vector<uint8_t> st(std::max<size_t>(total, 1), 0);
    const int rc = afv_table_fuse_points(table, points.handle(), jobs.data(), (int)nt, best.data(), occ.data(), st.data(), nf.data());
    if (rc != AFV_OK) fatal("afv_table_fuse_points", rc, ctx);
    FuseAnswer A;
    size_t at = 0;
    for (size_t k = 0; k < nt; ++k) {
        const size_t nq = targets[k].ids->size();
        A.best.emplace_back(best.begin() + at, best.begin() + at + nq);
        A.occupant.emplace_back(occ.begin() + at, occ.begin() + at + nq);
        A.status.emplace_back(st.begin() + at, st.begin() + at + nq);
        A.nFused.push_back(nf[k]);
        at += nq;
    }
    return A;
}
// Fuse(pKF, vpMapPoints, th) into every target (up to 64) in one call
inline FuseAnswer FuseIntoKeyFrames(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<FuseTarget> &targets, float th_low,
                                    float radiusTh = 3.0f) {
    return FuseRun(ctx, table, points, targets, radiusTh, th_low, true, nullptr);
}
// Rcw, tcw, Ow of a row-major 4 x 4 Scw as Fuse(pKF, Scw, ...) writes them (FeatureMatcher.cc:954-958): scw = |row 0 of sRcw|,
// Rcw = sRcw / scw, Ow = -Rcw^T tcw - and tcw is Scw's translation AS IT STANDS, the reference does not divide it by scw (a kept quirk).
// Compile the caller with -ffp-contract=off for the reference's bits.
inline afv_table_fuse_pose DecomposeScw(const float *Scw) {
    afv_table_fuse_pose p;
    const float s00 = Scw[0] * Scw[0], s01 = Scw[1] * Scw[1], s02 = Scw[2] * Scw[2];
    const float scw = std::sqrt(s00 + (s01 + s02));
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.R[3 * r + c] = Scw[4 * r + c] / scw;
        p.t[r] = Scw[4 * r + 3];
    }
    for (int k = 0; k < 3; ++k) {
        const float a0 = -p.R[k] * p.t[0], a1 = -p.R[3 + k] * p.t[1], a2 = -p.R[6 + k] * p.t[2];
        p.Ow[k] = a0 + (a1 + a2);
    }
    return p;
}
// Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): no reprojection gate, target k seen through Scw[k] (16 floats, row-major); status 6 is
// vpReplacePoint[iMP] = occupant
inline FuseAnswer FuseIntoKeyFramesSim3(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<FuseTarget> &targets,
                                        const std::vector<std::array<float, 16>> &Scw, float th_low, float radiusTh = 4.0f) {
    std::vector<afv_table_fuse_pose> poses;
    for (const std::array<float, 16> &S : Scw) poses.push_back(DecomposeScw(S.data()));
    return FuseRun(ctx, table, points, targets, radiusTh, th_low, false, &poses);
}

// ---- the covisibility count and the local map (include/afv_covis.h; reference: KeyFrame::UpdateConnections, AddConnection,
// UpdateBestCovisibles and the getters, KeyFrame.cc:131-219, :329-418; Tracking::UpdateLocalKeyFrames / UpdateLocalPoints, Tracking.cc:1040-1144).
// The device counts from the mvpMapPoints planes of the table (afv_table_set_map_points) and the flags of the store; what stays here is the
// bookkeeping of who is connected to whom.  Keyframes are named by their table slot and ordered by their keyId. ----
struct CovisQuery {  // one query of CovisibilityVotes: a position in the keyframe list (ids == nullptr) or a list of point ids
    int32_t position = -1;
    const std::vector<int32_t> *ids = nullptr;
    int32_t th = 15;
    bool skip_bad = false;
};
struct CovisAnswer {  // per query
    std::vector<std::vector<int32_t>> votes, order;  // [nk]; the positions of the connection rule
    std::vector<int32_t> best, n_nonzero;
};
inline CovisAnswer CovisibilityVotes(afv_ctx *ctx, afv_table *table, DeviceMapPoints &points, const std::vector<int32_t> &slots,
                                     const std::vector<int32_t> &key_ids, const std::vector<uint8_t> *kf_bad, const std::vector<CovisQuery> &queries) {
    const size_t nk = slots.size(), nq = queries.size();
    if (key_ids.size() != nk || (kf_bad && kf_bad->size() != nk)) fatal("CovisibilityVotes: one keyId and one flag per slot", AFV_EINVAL, ctx);
    std::vector<afv_covis_query> recs(std::max<size_t>(nq, 1));
    for (size_t q = 0; q < nq; ++q) {
        afv_covis_query &r = recs[q];
        r = afv_covis_query{};
        r.struct_size = (uint32_t)sizeof(r);
        r.th = queries[q].th;
        r.skip_bad = queries[q].skip_bad ? 1 : 0;
        if (queries[q].ids) {
            r.kind = AFV_COVIS_QUERY_IDS;
            r.n = (int32_t)queries[q].ids->size();
            r.ids = queries[q].ids->data();
        } else {
            r.kind = AFV_COVIS_QUERY_SLOT;
            r.position = queries[q].position;
        }
    }
    const size_t cells = std::max<size_t>(nq * nk, 1);
    std::vector<int32_t> votes(cells, 0), order(cells, -1), n_order(std::max<size_t>(nq, 1), 0), best(std::max<size_t>(nq, 1), -1), nz(std::max<size_t>(nq, 1), 0);
    const int rc = afv_table_covis_votes(table, points.handle(), slots.data(), key_ids.data(), kf_bad ? kf_bad->data() : nullptr, (int)nk, recs.data(),
                                         (int)nq, votes.data(), order.data(), n_order.data(), best.data(), nz.data());
    if (rc != AFV_OK) fatal("afv_table_covis_votes", rc, ctx);
    CovisAnswer A;
    for (size_t q = 0; q < nq; ++q) {
        A.votes.emplace_back(votes.begin() + q * nk, votes.begin() + (q + 1) * nk);
        A.order.emplace_back(order.begin() + q * nk, order.begin() + q * nk + n_order[q]);
        A.best.push_back(best[q]);
        A.n_nonzero.push_back(nz[q]);
    }
    return A;
}
struct LocalPointsAnswer {
    std::vector<int32_t> ids;   // localPts in the reference's order
    std::vector<uint8_t> seen;  // 1: a point of the frame (SearchLocalPoints skips it); empty without frame_pts
};
// Tracking::UpdateLocalPoints over `local`, the slots in the order of localKeyframes; cap = the table's features per slot
inline LocalPointsAnswer LocalPoints(afv_ctx *ctx, afv_table *table, int cap, DeviceMapPoints &points, const std::vector<int32_t> &local,
                                     const std::vector<int32_t> *frame_pts) {
    const size_t room = std::max<size_t>(local.size() * (size_t)cap, 1);
    LocalPointsAnswer A;
    A.ids.assign(room, -1);
    if (frame_pts) A.seen.assign(room, 0);
    int32_t n = 0;
    const int rc = afv_table_local_points(table, points.handle(), local.data(), (int)local.size(), frame_pts && !frame_pts->empty() ? frame_pts->data() : nullptr,
                                          frame_pts ? (int)frame_pts->size() : 0, (int)(local.size() * (size_t)cap), A.ids.data(),
                                          frame_pts ? A.seen.data() : nullptr, &n);
    if (rc != AFV_OK) fatal("afv_table_local_points", rc, ctx);
    A.ids.resize((size_t)n);
    if (frame_pts) A.seen.resize((size_t)n);
    return A;
}

class CovisibilityGraph {
  public:
    struct Node {  // the connection members of one KeyFrame
        int32_t slot = -1, key_id = -1;
        bool bad = false, first = true;
        std::map<int32_t, int32_t> weights;          // connectedKeyFrameWeights: slot -> weight
        std::vector<int32_t> ordered, ordered_w;     // orderedConnectedKeyFrames / orderedWeights
        int32_t parent = -1;                         // -1: none
        std::set<int32_t> children, loop_edges;
    };
    struct LocalMap {
        bool valid = false;                          // false: the reference returns before it touches the local map
        std::vector<int32_t> keyframes;              // localKeyframes (slots)
        int32_t ref = -1;                            // refKeyframe | -1
        std::vector<int32_t> ids;                    // localPts
        std::vector<uint8_t> seen;
    };
    int th = 15;  // KeyFrame.cc:369

    CovisibilityGraph(afv_ctx *ctx_, afv_table *table_, int cap_, DeviceMapPoints &points_) : ctx(ctx_), table(table_), cap(cap_), points(points_) {}

    void add_keyframe(int32_t slot, int32_t key_id) {
        if (kf.count(slot)) fatal("CovisibilityGraph::add_keyframe: the slot is listed", AFV_EINVAL, ctx);
        for (const auto &e : kf)
            if (e.second.key_id == key_id) fatal("CovisibilityGraph::add_keyframe: the keyId is listed", AFV_EINVAL, ctx);
        Node n;
        n.slot = slot;
        n.key_id = key_id;
        kf[slot] = n;
        listed.push_back(slot);
    }
    void set_bad(int32_t slot, bool bad = true) { node(slot).bad = bad; }

    void UpdateConnections(int32_t slot) { UpdateConnectionsBatch({slot}); }
    // one device call per 64 slots: the planes are read as they stand at the call, the host side effects are applied in list order
    void UpdateConnectionsBatch(const std::vector<int32_t> &batch) {
        std::vector<int32_t> keys;
        std::map<int32_t, int32_t> pos;
        for (size_t p = 0; p < listed.size(); ++p) {
            keys.push_back(kf[listed[p]].key_id);
            pos[listed[p]] = (int32_t)p;
        }
        for (size_t at = 0; at < batch.size(); at += AFV_COVIS_MAX_QUERIES) {
            const size_t end = std::min(batch.size(), at + AFV_COVIS_MAX_QUERIES);
            std::vector<CovisQuery> qs;
            for (size_t b = at; b < end; ++b) {
                if (!pos.count(batch[b])) fatal("CovisibilityGraph::UpdateConnections: unknown slot", AFV_EINVAL, ctx);
                CovisQuery q;
                q.position = pos[batch[b]];
                q.th = th;
                qs.push_back(q);
            }
            const CovisAnswer A = CovisibilityVotes(ctx, table, points, listed, keys, nullptr, qs);
            for (size_t b = at; b < end; ++b) Apply(batch[b], A.votes[b - at], A.order[b - at]);
        }
    }

    std::vector<int32_t> GetVectorCovisibleKeyFrames(int32_t slot) { return node(slot).ordered; }
    std::vector<int32_t> GetBestCovisibilityKeyFrames(int32_t slot, int N = 10) {
        const Node &n = node(slot);
        return std::vector<int32_t>(n.ordered.begin(), n.ordered.begin() + std::min<size_t>(n.ordered.size(), (size_t)std::max(N, 0)));
    }
    std::vector<int32_t> GetCovisiblesByWeight(int32_t slot, int w) {
        const Node &n = node(slot);
        size_t k = 0;
        while (k < n.ordered_w.size() && n.ordered_w[k] >= w) ++k;  // upper_bound with weightComp
        if (k == n.ordered_w.size()) return {};                     // it == end(): the reference answers an empty vector
        return std::vector<int32_t>(n.ordered.begin(), n.ordered.begin() + k);
    }
    int GetWeight(int32_t slot, int32_t other) {
        const Node &n = node(slot);
        const auto it = n.weights.find(other);
        return it == n.weights.end() ? 0 : it->second;
    }
    std::vector<int32_t> GetConnectedKeyFrames(int32_t slot) {  // ascending keyId, as the reference's map
        std::vector<int32_t> out;
        for (const auto &e : node(slot).weights) out.push_back(e.first);
        std::sort(out.begin(), out.end(), [&](int32_t a, int32_t b) { return kf[a].key_id < kf[b].key_id; });
        return out;
    }
    void EraseConnection(int32_t slot, int32_t other) {
        Node &n = node(slot);
        if (n.weights.erase(other)) Reorder(n);
    }
    int32_t GetParent(int32_t slot) { return node(slot).parent; }
    std::vector<int32_t> GetChilds(int32_t slot) {  // ascending keyId (the reference's set is ordered by pointer)
        const Node &n = node(slot);
        std::vector<int32_t> out(n.children.begin(), n.children.end());
        std::sort(out.begin(), out.end(), [&](int32_t a, int32_t b) { return kf[a].key_id < kf[b].key_id; });
        return out;
    }
    void AddLoopEdge(int32_t slot, int32_t other) { node(slot).loop_edges.insert(other); }
    // the pieces the edge list of OptimizeEssentialGraph is built from, keyed by keyId, over the keyframes that are not bad
    struct EssentialGraphPieces {
        std::map<int32_t, int32_t> parent;  // keyId -> keyId of the parent | -1
        std::map<int32_t, std::vector<int32_t>> loop_edges, covisibles;  // ascending keyId; GetCovisiblesByWeight(min_feat) in its order
    };
    EssentialGraphPieces essential_graph_dict(int min_feat = 100) {
        EssentialGraphPieces P;
        for (int32_t s : listed) {
            const Node &n = kf[s];
            if (n.bad) continue;
            P.parent[n.key_id] = n.parent < 0 ? -1 : kf[n.parent].key_id;
            std::vector<int32_t> le;
            for (int32_t o : n.loop_edges) le.push_back(kf[o].key_id);
            std::sort(le.begin(), le.end());
            P.loop_edges[n.key_id] = le;
            std::vector<int32_t> cv;
            for (int32_t o : GetCovisiblesByWeight(s, min_feat)) cv.push_back(kf[o].key_id);
            P.covisibles[n.key_id] = cv;
        }
        return P;
    }
    // what KeyFrameDatabase::DetectLoopCandidates / min_score_to_connected take as `connected` (a list) ...
    std::vector<int> connected(int32_t slot) {
        const std::vector<int32_t> c = GetConnectedKeyFrames(slot);
        return std::vector<int>(c.begin(), c.end());
    }
    // ... and what it and DetectRelocalizationCandidates take as `best_covisibles` (a callable): GetBestCovisibilityKeyFrames(10)
    std::function<std::vector<int>(int)> best_covisibles() {
        return [this](int slot) {
            const std::vector<int32_t> c = GetBestCovisibilityKeyFrames(slot, 10);
            return std::vector<int>(c.begin(), c.end());
        };
    }
    const Node &GetNode(int32_t slot) { return node(slot); }

    // Tracking::UpdateLocalMap: frame_pts = the point ids of the current frame, -1 = none
    LocalMap UpdateLocalMap(const std::vector<int32_t> &frame_pts, size_t max_keyframes = 80, int best_cov = 10) {
        LocalMap M;
        if (listed.empty()) return M;
        std::vector<int32_t> keys;
        std::vector<uint8_t> bad;
        for (int32_t s : listed) {
            keys.push_back(kf[s].key_id);
            bad.push_back(kf[s].bad ? 1 : 0);
        }
        CovisQuery q;
        q.ids = &frame_pts;
        q.th = 1;
        q.skip_bad = true;
        const CovisAnswer A = CovisibilityVotes(ctx, table, points, listed, keys, &bad, {q});
        if (A.n_nonzero[0] == 0) return M;
        M.valid = true;
        for (int32_t p : A.order[0]) M.keyframes.push_back(listed[(size_t)p]);
        std::sort(M.keyframes.begin(), M.keyframes.end(), [&](int32_t a, int32_t b) { return kf[a].key_id < kf[b].key_id; });  // the map iteration
        M.ref = A.best[0] >= 0 ? listed[(size_t)A.best[0]] : -1;
        std::set<int32_t> have(M.keyframes.begin(), M.keyframes.end());
        const size_t first_phase = M.keyframes.size();  // the range-for reads end() once: keyframes pushed below are not walked
        auto take = [&](int32_t s) {
            if (kf[s].bad || have.count(s)) return false;
            M.keyframes.push_back(s);
            have.insert(s);
            return true;
        };
        for (size_t k = 0; k < first_phase; ++k) {
            if (M.keyframes.size() > max_keyframes) break;
            const int32_t s = M.keyframes[k];
            for (int32_t nb : GetBestCovisibilityKeyFrames(s, best_cov))
                if (take(nb)) break;
            for (int32_t ch : GetChilds(s))
                if (take(ch)) break;
            const int32_t pa = kf[s].parent;
            if (pa >= 0 && take(pa)) break;
        }
        LocalPointsAnswer L = LocalPoints(ctx, table, cap, points, M.keyframes, &frame_pts);
        M.ids.swap(L.ids);
        M.seen.swap(L.seen);
        return M;
    }

  private:
    Node &node(int32_t slot) {
        const auto it = kf.find(slot);
        if (it == kf.end()) fatal("CovisibilityGraph: unknown slot", AFV_EINVAL, ctx);
        return it->second;
    }
    // weight descending, ties by keyId descending: KeyframeComparison and push_front
    void Reorder(Node &n) {
        std::vector<std::pair<int32_t, int32_t>> pairs;  // (weight, slot)
        for (const auto &e : n.weights) pairs.emplace_back(e.second, e.first);
        std::sort(pairs.begin(), pairs.end(), [&](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) {
            return a.first != b.first ? a.first > b.first : kf[a.second].key_id > kf[b.second].key_id;
        });
        n.ordered.clear();
        n.ordered_w.clear();
        for (const auto &e : pairs) {
            n.ordered.push_back(e.second);
            n.ordered_w.push_back(e.first);
        }
    }
    void AddConnection(Node &n, int32_t other, int32_t weight) {  // KeyFrame.cc:131-146
        const auto it = n.weights.find(other);
        if (it != n.weights.end() && it->second == weight) return;
        n.weights[other] = weight;
        Reorder(n);
    }
    void Apply(int32_t slot, const std::vector<int32_t> &row, const std::vector<int32_t> &order) {  // KeyFrame.cc:361-417
        Node &n = node(slot);
        std::map<int32_t, int32_t> counter;
        for (size_t p = 0; p < row.size(); ++p)
            if (row[p] > 0) counter[listed[p]] = row[p];
        if (counter.empty()) return;
        for (int32_t p : order) AddConnection(kf[listed[(size_t)p]], slot, row[(size_t)p]);
        n.weights = counter;  // the whole counter, not only the entries at the threshold (KeyFrame.cc:405)
        n.ordered.clear();
        n.ordered_w.clear();
        for (int32_t p : order) {
            n.ordered.push_back(listed[(size_t)p]);
            n.ordered_w.push_back(row[(size_t)p]);
        }
        if (n.first && n.key_id != 0) {
            n.parent = n.ordered.front();
            kf[n.parent].children.insert(slot);
            n.first = false;
        }
    }
    afv_ctx *ctx;
    afv_table *table;
    int cap;
    DeviceMapPoints &points;
    std::map<int32_t, Node> kf;
    std::vector<int32_t> listed;  // the slots in the order they were added
};

}  // namespace afv
