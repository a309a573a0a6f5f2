// plf.hpp -- header-only C++ host mirror of the reference classes over the C ABI (plf.h).
//
// The reference is compiled C++ and its hot path sits behind member calls, so the host side above the C ABI is
// C++ with the SAME class / method names and argument meaning:
//   ORB_SLAM2::ORBextractor   include/ORBextractor.h:44-112      -> plf::ORBextractor
//   ORB_SLAM2::LineSegment    include/ExtractLineSegment.h:29-57 -> plf::LineSegment
//   ORB_SLAM2::ORBmatcher     include/ORBmatcher.h:36-140        -> plf::ORBmatcher   (tracking overloads)
//   ORB_SLAM2::LSDmatcher     include/LSDmatcher.h:27-78         -> plf::LSDmatcher   (tracking overloads)
// OpenCV-free by default (plain structs that are bit-compatible with cv::KeyPoint / KeyLine / DMatch).  When
// OpenCV headers are available (`__has_include(<opencv2/core.hpp>)`), PLF_WITH_OPENCV adapters with the exact
// reference signatures (cv::InputArray, std::vector<cv::KeyPoint>&, cv::OutputArray ...) are provided as well --
// see INTEGRATION.md.  Error behaviour: the reference returns silently on an empty image and asserts on a wrong
// type; here empty -> outputs cleared, everything else -> plf::Error (never a silent fallback).
#pragma once
#include <cstring>
#include <stdexcept>
#include <string>
#include <algorithm>
#include <vector>
#include "plf.h"

namespace plf {

struct Error : std::runtime_error {
    int status;
    Error(int st, const char *what) : std::runtime_error(std::string(what) + ": " + plf_status_string(st)), status(st) {}
};
// errors (< 0) throw; warnings (> 0: the outputs are complete -- PLF_W_SLOW) are kept for the caller to look at
inline int &last_warning() { static thread_local int w = 0; return w; }
inline void check(int st, const char *what) { last_warning() = st > 0 ? st : 0; if (st < 0) throw Error(st, what); }

// ------------------------------------------------------------------ ORBextractor
class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int maxWidth = 640, int maxHeight = 480,
                 int maxBatch = 1, int device = 0)
    {
        plf_orb_params p = {nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, maxWidth, maxHeight, maxBatch};
        check(plf_orb_create(&p, &h_), "plf_orb_create");
        nlevels_ = nlevels; scaleFactor_ = scaleFactor;
        mvScaleFactor.resize(nlevels); mvInvScaleFactor.resize(nlevels); mvLevelSigma2.resize(nlevels); mvInvLevelSigma2.resize(nlevels);
        mnFeaturesPerLevel.resize(nlevels);
        check(plf_orb_get_tables(h_, nullptr, mvScaleFactor.data(), mvInvScaleFactor.data(), mvLevelSigma2.data(), mvInvLevelSigma2.data(),
                                 mnFeaturesPerLevel.data()), "plf_orb_get_tables");
    }
    ~ORBextractor() { plf_orb_destroy(h_); }
    ORBextractor(const ORBextractor &) = delete;
    ORBextractor &operator=(const ORBextractor &) = delete;

    // void operator()(InputArray image, InputArray mask, vector<KeyPoint>& keypoints, OutputArray descriptors)
    // image: 8-bit single channel; mask is ignored (as in the reference); descriptors: keypoints.size() x 32 bytes
    void operator()(const uint8_t *image, int width, int height, ptrdiff_t pitch, std::vector<plf_keypoint> &keypoints,
                    std::vector<uint8_t> &descriptors)
    {
        const int cap = plf_orb_capacity(h_);
        keypoints.resize(cap); descriptors.resize((size_t)cap * 32);
        int32_t n = 0;
        const int st = plf_orb_extract(h_, image, width, height, pitch, keypoints.data(), descriptors.data(), cap, &n);
        if (st == PLF_E_EMPTY) { keypoints.clear(); descriptors.clear(); return; }
        check(st, "plf_orb_extract");
        keypoints.resize(n); descriptors.resize((size_t)n * 32);
    }

    int GetLevels() const { return nlevels_; }
    float GetScaleFactor() const { return scaleFactor_; }
    std::vector<float> GetScaleFactors() const { return mvScaleFactor; }
    std::vector<float> GetInverseScaleFactors() const { return mvInvScaleFactor; }
    std::vector<float> GetScaleSigmaSquares() const { return mvLevelSigma2; }
    std::vector<float> GetInverseScaleSigmaSquares() const { return mvInvLevelSigma2; }

    // mvImagePyramid[level] of the last call (with its 19-px border), pitch = width + 38
    std::vector<uint8_t> ImagePyramidLevel(int level, int *w = nullptr, int *h = nullptr)
    {
        int32_t lw = 0, lh = 0;
        check(plf_orb_get_pyramid_level(h_, 0, level, nullptr, &lw, &lh), "plf_orb_get_pyramid_level");
        std::vector<uint8_t> out((size_t)(lw + 38) * (lh + 38));
        check(plf_orb_get_pyramid_level(h_, 0, level, out.data(), nullptr, nullptr), "plf_orb_get_pyramid_level");
        if (w) *w = lw;
        if (h) *h = lh;
        return out;
    }
    plf_orb *handle() { return h_; }

    std::vector<int32_t> mnFeaturesPerLevel;

private:
    plf_orb *h_ = nullptr;
    int nlevels_ = 0;
    float scaleFactor_ = 0;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
};

// ------------------------------------------------------------------ LineSegment
struct Vector3d { double v[3]; double operator()(int i) const { return v[i]; } };

class LineSegment {
public:
    // maxMs > 0: opt-in time budget of LSD region growing per call (plf_line_params.max_ms; the reference has none)
    explicit LineSegment(int nlines = 100, int maxWidth = 640, int maxHeight = 480, int maxBatch = 1, int device = 0, float maxMs = 0.f) : nlines_(nlines)
    {
        plf_line_params p = {nlines, 0, device, maxWidth, maxHeight, maxBatch, PLF_LBD_BLURRED, maxMs};
        check(plf_line_create(&p, &h_), "plf_line_create");
    }
    ~LineSegment() { plf_line_destroy(h_); }
    LineSegment(const LineSegment &) = delete;
    LineSegment &operator=(const LineSegment &) = delete;

    // void ExtractLineSegment(const Mat& img, vector<KeyLine>& keylines, Mat& ldesc, vector<Vector3d>& lineFunctions,
    //                         int scale = 1.2, int numOctaves = 1)     (scale truncates to 1, one octave)
    void ExtractLineSegment(const uint8_t *img, int width, int height, ptrdiff_t pitch, std::vector<plf_keyline> &vkeyLines,
                            std::vector<uint8_t> &ldesc, std::vector<Vector3d> &vkeylineFunctions, int scale = 1, int numOctaves = 1)
    {
        if (scale != 1 || numOctaves != 1) throw Error(PLF_E_BADARG, "ExtractLineSegment: only scale=1, numOctaves=1 (the reference's call)");
        vkeyLines.resize(nlines_); ldesc.resize((size_t)nlines_ * 32); vkeylineFunctions.resize(nlines_);
        int32_t n = 0;
        const int st = plf_line_extract(h_, img, width, height, pitch, vkeyLines.data(), ldesc.data(), &vkeylineFunctions[0].v[0], nlines_, &n);
        if (st == PLF_E_EMPTY) n = 0;
        else check(st, "plf_line_extract");
        vkeyLines.resize(n); ldesc.resize((size_t)n * 32); vkeylineFunctions.resize(n);
    }
    // void LineSegmentMathch(Mat &ldesc1, Mat &ldesc2)   include/ExtractLineSegment.h:41   (host descriptor rows, n x 32; knnMatch k = 2 into mvlineMatches)
    // void LineDescriptorMAD()                             include/ExtractLineSegment.h:44   (mnnMad, mnn12Mad of those matches; computed in the same device pass)
    void LineSegmentMathch(const uint8_t *ldesc1, int n1, const uint8_t *ldesc2, int n2, int device = 0)
    {
        mvlineMatches.clear(); mnnMad = mnn12Mad = 0.0;
        if (n1 < 1 || n2 < 2) return;
        plf_matcher *m = nullptr;
        check(plf_matcher_create(device, 64, 64, n1 > n2 ? n1 : n2, 1, &m), "plf_matcher_create");
        void *d1 = nullptr, *d2 = nullptr;
        int st = plf_device_alloc(device, (size_t)n1 * 32, &d1);
        if (st == PLF_OK) st = plf_device_alloc(device, (size_t)n2 * 32, &d2);
        if (st == PLF_OK) st = plf_upload(d1, ldesc1, (size_t)n1 * 32, nullptr);
        if (st == PLF_OK) st = plf_upload(d2, ldesc2, (size_t)n2 * 32, nullptr);
        std::vector<plf_dmatch> knn((size_t)n1 * 2);
        double mad[2] = {0.0, 0.0};
        if (st == PLF_OK) st = plf_line_descriptor_mad(m, (const uint8_t *)d1, n1, (const uint8_t *)d2, n2, knn.data(), mad, PLF_MEM_HOST, nullptr);
        plf_device_free(d1); plf_device_free(d2); plf_matcher_destroy(m);
        check(st, "plf_line_descriptor_mad");
        mvlineMatches.resize(n1);
        for (int q = 0; q < n1; q++) mvlineMatches[q] = {knn[2 * q], knn[2 * q + 1]};
        mnnMad = mad[0]; mnn12Mad = mad[1];
    }
    void LineDescriptorMAD(double &nn_mad, double &nn12_mad) const { nn_mad = mnnMad; nn12_mad = mnn12Mad; }
    // double LineSegmentOverlap(double spl_obs, double epl_obs, double spl_proj, double epl_proj)   include/ExtractLineSegment.h:47
    static double LineSegmentOverlap(double spl_obs, double epl_obs, double spl_proj, double epl_proj)
    {
        return plf_line_segment_overlap(spl_obs, epl_obs, spl_proj, epl_proj);
    }
    plf_line *handle() { return h_; }

    std::vector<std::vector<plf_dmatch>> mvlineMatches;   // include/ExtractLineSegment.h:51
    double mnnMad = 0.0, mnn12Mad = 0.0;                    // include/ExtractLineSegment.h:52

private:
    plf_line *h_ = nullptr;
    int nlines_;
};

// ------------------------------------------------------------------ matchers (device-resident views, see plf.h)
class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
    ORBmatcher(plf_matcher *m, float nnratio = 0.6f, bool checkOri = true) : m_(m), mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    static int DescriptorDistance(const uint8_t *a, const uint8_t *b) { return plf_hamming256(a, b); }
    // int SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th = 3)
    void SearchByProjection(const plf_frame_view &F, const plf_mappoint_view &vpMapPoints, float th, int32_t *match_of_kp_dev,
                            int32_t *nmatches_dev, void *stream = nullptr)
    {
        check(plf_match_project_points(m_, &F, 1, &vpMapPoints, th, mfNNratio, match_of_kp_dev, F.n, nmatches_dev, stream), "SearchByProjection");
    }
    // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
    void SearchByProjection(const plf_frame_view &CurrentFrame, const plf_lastframe_view &LastFrame, const plf_pose_pair &pose, float th, bool bMono,
                            int32_t *match_of_kp_dev, int32_t *nmatches_dev, void *stream = nullptr)
    {
        check(plf_match_project_lastframe(m_, &CurrentFrame, &LastFrame, &pose, th, bMono, mbCheckOrientation, match_of_kp_dev, nmatches_dev, stream),
              "SearchByProjection(last frame)");
    }
    // int SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const std::set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist)
    void SearchByProjection(const plf_frame_view &CurrentFrame, const plf_lastframe_view &pKF, const float *min_distance_dev, const float *max_distance_dev,
                            const plf_pose_pair &pose, float log_scale_factor, float th, int ORBdist, int32_t *match_of_kp_dev, int32_t *nmatches_dev,
                            void *stream = nullptr)
    {
        check(plf_match_project_keyframe(m_, &CurrentFrame, &pKF, min_distance_dev, max_distance_dev, &pose, log_scale_factor, th, ORBdist,
                                         mbCheckOrientation, match_of_kp_dev, nmatches_dev, stream), "SearchByProjection(keyframe)");
    }
    // int SearchByBoW(KeyFrame *pKF, Frame &F, std::vector<MapPoint*> &vpMapPointMatches)
    void SearchByBoW(const plf_bow_view &pKF_and_F, int32_t *match_of_f_dev, int32_t *nmatches_dev, void *stream = nullptr)
    {
        check(plf_match_bow(m_, &pKF_and_F, 1, mfNNratio, mbCheckOrientation, match_of_f_dev, pKF_and_F.n_f, nmatches_dev, stream), "SearchByBoW");
    }
    // int SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint*> &vpMatches12)
    void SearchByBoW(const plf_bow_view &pKF1_and_pKF2, int32_t *match12_dev, int32_t *nmatches_dev, bool /*keyframes*/, void *stream = nullptr)
    {
        check(plf_match_bow_kf(m_, &pKF1_and_pKF2, 1, mfNNratio, mbCheckOrientation, match12_dev, std::max(pKF1_and_pKF2.n_kf, pKF1_and_pKF2.n_f), nmatches_dev, stream),
              "SearchByBoW(keyframes)");
    }
    // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs, const bool bOnlyStereo)
    void SearchForTriangulation(const plf_tri_view &pKF1_and_pKF2, const float *F12, const float *Cw1, const plf_kf_pose &pose2, bool bOnlyStereo,
                                int32_t *match12_dev, int32_t *nmatches_dev, void *stream = nullptr)
    {
        check(plf_match_triangulation(m_, &pKF1_and_pKF2, F12, Cw1, &pose2, bOnlyStereo, mbCheckOrientation, match12_dev, nmatches_dev, stream),
              "SearchForTriangulation");
    }
    // int Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th = 3.0)   (search half; the caller applies Replace / AddObservation)
    void Fuse(const plf_frame_view &pKF, const plf_kf_pose &pose, const plf_points3d_view &vpMapPoints, float th, int32_t *best_idx_dev,
              int32_t *nfused_dev, void *stream = nullptr)
    {
        check(plf_match_fuse(m_, &pKF, &pose, &vpMapPoints, th, best_idx_dev, nfused_dev, stream), "Fuse");
    }
    // int Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th, vector<MapPoint*> &vpReplacePoint)
    void Fuse(const plf_frame_view &pKF, const float *Scw, const plf_kf_pose &intrinsics, const plf_points3d_view &vpPoints, float th,
              int32_t *best_idx_dev, int32_t *nfused_dev, void *stream = nullptr)
    {
        check(plf_match_fuse_sim3(m_, &pKF, Scw, &intrinsics, &vpPoints, th, best_idx_dev, nfused_dev, stream), "Fuse(Scw)");
    }
    // int SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
    void SearchByProjection(const plf_frame_view &pKF, const float *Scw, const plf_kf_pose &intrinsics, const plf_points3d_view &vpPoints, int th,
                            int32_t *match_of_kp_dev, int32_t *nmatches_dev, void *stream = nullptr)
    {
        check(plf_match_project_sim3(m_, &pKF, Scw, &intrinsics, &vpPoints, th, match_of_kp_dev, nmatches_dev, stream), "SearchByProjection(Scw)");
    }
    // int SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12, const cv::Mat &t12, const float th)
    void SearchBySim3(const plf_frame_view &pKF1, const plf_frame_view &pKF2, const plf_kf_pose &pose1, const plf_kf_pose &pose2, float s12, const float *R12,
                      const float *t12, float th, const plf_points3d_view &vpMapPoints1, const plf_points3d_view &vpMapPoints2, int32_t *match12_dev,
                      int32_t *nfound_dev, void *stream = nullptr)
    {
        check(plf_match_sim3(m_, &pKF1, &pKF2, &pose1, &pose2, s12, R12, t12, th, &vpMapPoints1, &vpMapPoints2, match12_dev, nfound_dev, stream), "SearchBySim3");
    }

private:
    plf_matcher *m_;
    float mfNNratio;
    bool mbCheckOrientation;
};

class LSDmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
    LSDmatcher(plf_matcher *m, float nnratio = 0.6f, bool checkOri = true) : m_(m), mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    static int DescriptorDistance(const uint8_t *a, const uint8_t *b) { return plf_hamming256(a, b); }
    // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)   (BF kNN + MAD rule)
    void SearchByProjection(const uint8_t *last_desc_dev, int nlast, const uint8_t *cur_desc_dev, int ncur, const uint8_t *last_has_mapline_dev,
                            int32_t *match_of_line_dev, int32_t *nmatches_dev, void *stream = nullptr)
    {
        check(plf_match_lines_lastframe(m_, last_desc_dev, nlast, cur_desc_dev, ncur, last_has_mapline_dev, match_of_line_dev, nmatches_dev, stream),
              "LSDmatcher::SearchByProjection(last frame)");
    }
    // int SearchByProjection(Frame &F, const vector<MapLine*> &vpMapLines, const float th = 3)
    void SearchByProjection(const plf_lineframe_view &F, const plf_mapline_view &vpMapLines, float th, int32_t *match_of_line_dev,
                            int32_t *nmatches_dev, void *stream = nullptr)
    {
        check(plf_match_project_lines(m_, &F, 1, &vpMapLines, th, mfNNratio, match_of_line_dev, F.n, nmatches_dev, stream), "LSDmatcher::SearchByProjection");
    }

    // int SearchByProjection(KeyFrame *pKF, Frame &F, vector<MapLine*> &vpMapLineMatches): the same rule, the keyframe's lines on the query side
    void SearchByProjection(const uint8_t *kf_desc_dev, int nkf, const uint8_t *f_desc_dev, int nf, const uint8_t *kf_has_mapline_dev, int32_t *match_of_line_dev,
                            int32_t *nmatches_dev, bool /*keyframe*/, void *stream = nullptr)
    {
        check(plf_match_lines_lastframe(m_, kf_desc_dev, nkf, f_desc_dev, nf, kf_has_mapline_dev, match_of_line_dev, nmatches_dev, stream),
              "LSDmatcher::SearchByProjection(keyframe)");
    }
    // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, vector<pair<size_t, size_t>> &vMatchedPairs, const bool bOnlyStereo)
    void SearchForTriangulation(const uint8_t *desc1_dev, int n1, const uint8_t *desc2_dev, int n2, const uint8_t *has_ml1_dev, const uint8_t *has_ml2_dev,
                                const uint8_t *stereo1_dev, const uint8_t *stereo2_dev, bool bOnlyStereo, int32_t *match12_dev, int32_t *nmatches_dev,
                                float mad_factor = 0.1f, void *stream = nullptr)
    {
        check(plf_match_lines_triangulation(m_, desc1_dev, n1, desc2_dev, n2, has_ml1_dev, has_ml2_dev, stereo1_dev, stereo2_dev, bOnlyStereo, mad_factor,
                                            match12_dev, nmatches_dev, stream), "LSDmatcher::SearchForTriangulation");
    }
    // int Fuse(KeyFrame *pKF, const vector<MapLine*> &vpMapLines)   (search half; the caller applies Replace / AddObservation / AddMapLine)
    void Fuse(const uint8_t *kf_desc_dev, int nkf, const uint8_t *ml_desc_dev, const uint8_t *valid_dev, int m, int32_t *best_idx_dev, int32_t *nfused_dev,
              void *stream = nullptr)
    {
        check(plf_match_lines_fuse(m_, kf_desc_dev, nkf, ml_desc_dev, valid_dev, m, best_idx_dev, nfused_dev, stream), "LSDmatcher::Fuse");
    }

private:
    plf_matcher *m_;
    float mfNNratio;
    bool mbCheckOrientation;
};

// RAII device array for host code that stages data for the matchers (plf_device_alloc / plf_upload / plf_download)
template <class T> class DeviceArray {
public:
    DeviceArray() = default;
    DeviceArray(size_t n, int device = 0) { reset(n, device); }
    template <class U> DeviceArray(const std::vector<U> &host, int device = 0) { assign(host, device); }
    ~DeviceArray() { plf_device_free(p_); }
    DeviceArray(const DeviceArray &) = delete;
    DeviceArray &operator=(const DeviceArray &) = delete;
    void reset(size_t n, int device = 0) { plf_device_free(p_); p_ = nullptr; n_ = n; void *q = nullptr; check(plf_device_alloc(device, n * sizeof(T), &q), "plf_device_alloc"); p_ = (T *)q; }
    void upload(const void *host, size_t n) { check(plf_upload(p_, host, n * sizeof(T), nullptr), "plf_upload"); }
    template <class U> void assign(const std::vector<U> &host, int device = 0) { static_assert(sizeof(U) == sizeof(T), "element size"); reset(host.size(), device); upload(host.data(), host.size()); }
    void fill(int byte, void *stream = nullptr) { check(plf_fill(p_, byte, n_ * sizeof(T), stream), "plf_fill"); }   // NULL: synchronous; else enqueued on `stream`
    std::vector<T> download() const { std::vector<T> v(n_); check(plf_download(v.data(), p_, n_ * sizeof(T), nullptr), "plf_download"); return v; }
    T *get() const { return p_; }
    size_t size() const { return n_; }
private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

// ORB_SLAM2::Frame members either side of the extractor / matcher path (include/Frame.h), stateless: device pointers in and out, one frame.
// Names and roles follow the reference; the reference works on its own member vectors, these take the same data as arrays.
struct Frame {
    // void Frame::UndistortKeyPoints()  include/Frame.h (so@0xf8630): mvKeys -> mvKeysUn
    static void UndistortKeyPoints(const plf_keypoint *mvKeys_dev, int N, const plf_camera &cam, plf_keypoint *mvKeysUn_dev, int device = 0,
                                   void *stream = nullptr)
    {
        check(plf_frame_tail(mvKeys_dev, nullptr, N, 1, N, nullptr, 0, 0, &cam, mvKeysUn_dev, nullptr, nullptr, device, stream), "Frame::UndistortKeyPoints");
    }
    // void Frame::ComputeStereoFromRGBD(const cv::Mat &imDepth) (so@0xf6860): mvuRight, mvDepth (also rewrites mvKeysUn: same values)
    static void ComputeStereoFromRGBD(const plf_keypoint *mvKeys_dev, int N, const float *imDepth_dev, int width, int height, const plf_camera &cam,
                                      plf_keypoint *mvKeysUn_dev, float *mvuRight_dev, float *mvDepth_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_frame_tail(mvKeys_dev, nullptr, N, 1, N, imDepth_dev, width, height, &cam, mvKeysUn_dev, mvuRight_dev, mvDepth_dev, device, stream),
              "Frame::ComputeStereoFromRGBD");
    }
    // void Frame::UndistortKeyLines() include/Frame.h:267 + mvuRightLineStart/End, mvDepthLineStart/End (:208-211)
    static void UndistortKeyLines(const plf_keyline *mvKeylines_dev, int NL, const float *imDepth_dev, int width, int height, const plf_camera &cam,
                                  plf_keyline *mvKeylinesUn_dev, float *mvuRightLineStart_dev, float *mvuRightLineEnd_dev, float *mvDepthLineStart_dev,
                                  float *mvDepthLineEnd_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_frame_line_tail(mvKeylines_dev, nullptr, NL, 1, NL, imDepth_dev, width, height, &cam, mvKeylinesUn_dev, mvuRightLineStart_dev,
                                  mvuRightLineEnd_dev, mvDepthLineStart_dev, mvDepthLineEnd_dev, device, stream), "Frame::UndistortKeyLines");
    }
    // bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit) include/Frame.h:104, for M map points at once -> the plf_mappoint_view fields
    static void isInFrustum(const float *world_pos_dev, const float *normal_dev, const float *min_distance_dev, const float *max_distance_dev, int M,
                            const plf_frustum_pose &pose, const plf_camera &cam, const float bounds[4], float mfLogScaleFactor, int mnScaleLevels,
                            float viewingCosLimit, float *mTrackProjX_dev, float *mTrackProjY_dev, float *mTrackProjXR_dev, int32_t *mnTrackScaleLevel_dev,
                            float *mTrackViewCos_dev, uint8_t *mbTrackInView_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_frustum_points(world_pos_dev, normal_dev, min_distance_dev, max_distance_dev, M, &pose, &cam, bounds[0], bounds[1], bounds[2], bounds[3],
                                 mfLogScaleFactor, mnScaleLevels, viewingCosLimit, mTrackProjX_dev, mTrackProjY_dev, mTrackProjXR_dev,
                                 mnTrackScaleLevel_dev, mTrackViewCos_dev, mbTrackInView_dev, device, stream), "Frame::isInFrustum(MapPoint)");
    }
    // bool Frame::isInFrustum(MapLine *pML, float viewingCosLimit) include/Frame.h:107, for M map lines (world_pos6: start xyz, end xyz)
    static void isInFrustum(const float *world_pos6_dev, const float *normal_dev, const float *min_distance_dev, const float *max_distance_dev, int M,
                            const plf_frustum_pose &pose, const plf_camera &cam, const float bounds[4], float mfLogScaleFactor, int mnScaleLevels,
                            float viewingCosLimit, float *mTrackProjX1_dev, float *mTrackProjY1_dev, float *mTrackProjX1R_dev, float *mTrackProjX2_dev,
                            float *mTrackProjY2_dev, float *mTrackProjX2R_dev, int32_t *mnTrackScaleLevel_dev, float *mTrackViewCos_dev,
                            uint8_t *mbTrackInView_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_frustum_lines(world_pos6_dev, normal_dev, min_distance_dev, max_distance_dev, M, &pose, &cam, bounds[0], bounds[1], bounds[2], bounds[3],
                                mfLogScaleFactor, mnScaleLevels, viewingCosLimit, mTrackProjX1_dev, mTrackProjY1_dev, mTrackProjX1R_dev, mTrackProjX2_dev,
                                mTrackProjY2_dev, mTrackProjX2R_dev, mnTrackScaleLevel_dev, mTrackViewCos_dev, mbTrackInView_dev, device, stream),
              "Frame::isInFrustum(MapLine)");
    }
};

// void MapPoint::ComputeDistinctiveDescriptors() include/MapPoint.h:75 (so@0x94460) for a batch of map points: device arrays in, the representative
// descriptors written in place into the array the matchers' views read (plf_map_distinctive_descriptors; obs in CSR form, see plf_map_obs_view)
struct MapPoint {
    static void ComputeDistinctiveDescriptors(const plf_map_obs_view &mObservations_dev, uint8_t *mDescriptor_dev, int map_rows, int32_t *best_obs_dev,
                                              int32_t *best_median_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_map_distinctive_descriptors(&mObservations_dev, mDescriptor_dev, map_rows, best_obs_dev, best_median_dev, device, stream),
              "MapPoint::ComputeDistinctiveDescriptors");
    }
    // void MapPoint::UpdateNormalAndDepth() (so@0x924e0), the statement after every ComputeDistinctiveDescriptors(): mNormalVector, mfMinDistance and
    // mfMaxDistance written in place into the arrays plf_frustum_points reads (plf_map_update_normal_depth; see plf_map_geom_view)
    static void UpdateNormalAndDepth(const plf_map_geom_view &mObservations_dev, const float *mWorldPos_dev, float *mNormalVector_dev, float *mfMinDistance_dev,
                                     float *mfMaxDistance_dev, int map_rows, int32_t *n_obs_used_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_map_update_normal_depth(&mObservations_dev, mWorldPos_dev, mNormalVector_dev, mfMinDistance_dev, mfMaxDistance_dev, map_rows, n_obs_used_dev,
                                          device, stream),
              "MapPoint::UpdateNormalAndDepth");
    }
};
// void MapLine::ComputeDistinctiveDescriptors() include/MapLine.h:93 -- declared without a body in the reference: the MapPoint rule over the keyframes'
// line descriptors with LSDmatcher::DescriptorDistance (PARITY UNPINNED); writes mLDescriptor
struct MapLine {
    static void ComputeDistinctiveDescriptors(const plf_map_obs_view &mObservations_dev, uint8_t *mLDescriptor_dev, int map_rows, int32_t *best_obs_dev,
                                              int32_t *best_median_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_map_distinctive_descriptors(&mObservations_dev, mLDescriptor_dev, map_rows, best_obs_dev, best_median_dev, device, stream),
              "MapLine::ComputeDistinctiveDescriptors");
    }
    // void MapLine::UpdateAverageDir() include/MapLine.h:97 -- declared without a body in the reference: the MapPoint rule at the segment's midpoint
    // (PARITY UNPINNED).  The view has pos_floats = 6 and the packed level form; the distances may both be NULL (direction only).
    static void UpdateAverageDir(const plf_map_geom_view &mObservations_dev, const float *mWorldPos_dev, float *mNormalVector_dev, float *mfMinDistance_dev,
                                 float *mfMaxDistance_dev, int map_rows, int32_t *n_obs_used_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_map_update_normal_depth(&mObservations_dev, mWorldPos_dev, mNormalVector_dev, mfMinDistance_dev, mfMaxDistance_dev, map_rows, n_obs_used_dev,
                                          device, stream),
              "MapLine::UpdateAverageDir");
    }
};

// void LocalMapping::KeyFrameCulling() (so@0x643e0) over device arrays: the candidates are rows of the view in the reference's order (a row of
// plf_covis_count's ord_kf when a keyframe's row index is its slot).  PLF_CULL_SEQUENTIAL gives the one-by-one loop with the erasures of
// KeyFrame::SetBadFlag applied in between; status_dev[0] < n_cand means more than max_culls erasures: call again for the rest (plf_keyframe_culling).
inline void KeyFrameCulling(const plf_cull_view &map_dev, const plf_cull_params &params, const int32_t *cand_row_dev, const uint8_t *cand_flags_dev, int n_cand,
                            int32_t *n_mps_dev, int32_t *n_redundant_dev, int32_t *decision_dev, uint8_t *kf_erased_dev, uint8_t *point_went_bad_dev,
                            int32_t *point_nobs_dev, int32_t *status_dev, int device = 0, void *stream = nullptr)
{
    check(plf_keyframe_culling(&map_dev, &params, cand_row_dev, cand_flags_dev, n_cand, n_mps_dev, n_redundant_dev, decision_dev, kf_erased_dev,
                               point_went_bad_dev, point_nobs_dev, status_dev, device, stream), "LocalMapping::KeyFrameCulling");
}
inline plf_cull_params KeyFrameCullingParams(int mode = PLF_CULL_SEQUENTIAL) { return plf_cull_params{mode, 3, 0, 0, 0.9}; }   // the reference's constants
// void LocalMapping::MapPointCulling() (so@0x593f0) over mlpRecentAddedMapPoints as device arrays, Observations() given per point: decision 0 keep,
// 1 erase from the list, 2 SetBadFlag() and erase.  cnThObs is 2 for a monocular system, 3 otherwise.
inline void MapPointCulling(int n, const int32_t *mnFound_dev, const int32_t *mnVisible_dev, const int64_t *mnFirstKFid_dev, const int32_t *nObs_dev,
                            const uint8_t *point_bad_dev, long unsigned int nCurrentKFid, int cnThObs, int32_t *decision_dev, int device = 0,
                            void *stream = nullptr)
{
    check(plf_map_point_culling(n, mnFound_dev, mnVisible_dev, mnFirstKFid_dev, nObs_dev, nullptr, nullptr, nullptr, 0, point_bad_dev, (int64_t)nCurrentKFid,
                                cnThObs, decision_dev, device, stream), "LocalMapping::MapPointCulling");
}

// ------------------------------------------------------------------ batches of independent host frames on all GPUs of the node
// The caller loop of the reference (Examples/RGB-D/rgbd_tum.cc:84-128 -> System::TrackRGBD -> Tracking::GrabImageRGBD -> RGB-D Frame::Frame,
// include/Frame.h:60) for N frames at once: plf_batch_* shards the frames over the GPUs in contiguous blocks (no collective), stages them through
// pinned double buffers and returns every Frame member the front-end produces.  Frames are independent: this is the offline / dataset-replay /
// multi-camera mode (BASELINE configs 3-4); the live loop uses ORBextractor / LineSegment above.
struct BatchFrames {   // outputs of one call: frame f at [f * kp_capacity, ...) / [f * line_capacity, ...)
    int n = 0, kp_capacity = 0, line_capacity = 0;
    std::vector<plf_keypoint> mvKeys, mvKeysUn; std::vector<uint8_t> mDescriptors; std::vector<int32_t> N;
    std::vector<float> mvuRight, mvDepth;
    std::vector<plf_keyline> mvKeylines, mvKeylinesUn; std::vector<uint8_t> mLdesc; std::vector<double> mvKeyLineFunctions; std::vector<int32_t> NL;
    std::vector<float> mvuRightLineStart, mvuRightLineEnd, mvDepthLineStart, mvDepthLineEnd;
    std::vector<int32_t> match_of_kp, n_kp_matches, match_of_line, n_line_matches;   // against the local map of set_local_map (-1 = none)
};

class BatchExtractor {
public:
    // devices empty = every visible GPU.  rgbd = the Frame-tail buffers of extract_rgbd.
    BatchExtractor(int nfeatures, int nlines, int width, int height, int frames_in_flight = 8, const std::vector<int> &devices = {},
                   int input_format = PLF_FMT_GRAY8, int max_mappoints = 0, int max_maplines = 0, bool rgbd = false, float scaleFactor = 1.2f, int nlevels = 8,
                   int iniThFAST = 20, int minThFAST = 7)
        : nfeatures_(nfeatures), nlines_(nlines), kp_cap_(nfeatures > 0 ? nfeatures + 4 * nlevels : 0)
    {
        plf_batch_params p;
        std::memset(&p, 0, sizeof(p));
        p.orb.nfeatures = nfeatures; p.orb.scale_factor = scaleFactor; p.orb.nlevels = nlevels; p.orb.ini_th_fast = iniThFAST; p.orb.min_th_fast = minThFAST;
        p.orb.max_width = width; p.orb.max_height = height; p.orb.max_batch = 1;
        p.line.nlines = nlines; p.line.max_width = width; p.line.max_height = height; p.line.max_batch = 1; p.line.lbd_sobel_input = PLF_LBD_BLURRED;
        std::vector<int32_t> dv(devices.begin(), devices.end());
        p.n_devices = (int32_t)dv.size(); p.devices = dv.empty() ? nullptr : dv.data();
        p.frames_in_flight = frames_in_flight; p.input_format = input_format; p.max_mappoints = max_mappoints; p.max_maplines = max_maplines; p.rgbd = rgbd ? 1 : 0;
        check(plf_batch_create(&p, &b_), "plf_batch_create");
    }
    ~BatchExtractor() { plf_batch_destroy(b_); }
    BatchExtractor(const BatchExtractor &) = delete;
    BatchExtractor &operator=(const BatchExtractor &) = delete;

    int device_count() const { return plf_batch_device_count(b_); }
    // host arrays of the tracking fields of the local map; replicated on every GPU (Tracking::SearchLocalPoints / SearchLocalLines feed)
    void set_local_map(const plf_mappoint_view *points, const plf_mapline_view *lines, float th, float nnratio, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY)
    {
        check(plf_batch_set_local_map(b_, points, lines, th, nnratio, mnMinX, mnMinY, mnMaxX, mnMaxY), "plf_batch_set_local_map");
        has_map_ = (points && points->m > 0) || (lines && lines->m > 0);
    }
    // gray / RGB / BGR frames (the format given to the constructor); returns PLF_OK or PLF_E_CAPACITY (outputs truncated), throws otherwise
    int extract(const uint8_t *images, int64_t n_frames, int width, int height, ptrdiff_t pitch, ptrdiff_t frame_stride, BatchFrames &out)
    {
        return run(images, n_frames, width, height, pitch, frame_stride, nullptr, nullptr, 0, 0, 0.f, out);
    }
    // RGB-D Frame constructor per frame: depth = uint16 images (NULL: none), mDepthMapFactor = 1 / DepthMapFactor of the settings file
    int extract_rgbd(const uint8_t *images, const uint16_t *depth, int64_t n_frames, int width, int height, ptrdiff_t pitch, ptrdiff_t frame_stride,
                     ptrdiff_t depth_pitch_elems, ptrdiff_t depth_frame_stride_elems, const plf_camera &cam, float mDepthMapFactor, BatchFrames &out)
    {
        return run(images, n_frames, width, height, pitch, frame_stride, &cam, depth, depth_pitch_elems, depth_frame_stride_elems, mDepthMapFactor, out);
    }
    plf_batch *handle() { return b_; }

private:
    int run(const uint8_t *images, int64_t n, int width, int height, ptrdiff_t pitch, ptrdiff_t frame_stride, const plf_camera *cam, const uint16_t *depth,
            ptrdiff_t dpitch, ptrdiff_t dstride, float factor, BatchFrames &o)
    {
        const size_t K = (size_t)n * kp_cap_, Lc = (size_t)n * nlines_;
        o.n = (int)n; o.kp_capacity = kp_cap_; o.line_capacity = nlines_;
        plf_batch_outputs O;
        std::memset(&O, 0, sizeof(O));
        if (nfeatures_ > 0) {
            o.mvKeys.assign(K, plf_keypoint()); o.mDescriptors.assign(K * 32, 0); o.N.assign(n, 0);
            O.kps = o.mvKeys.data(); O.desc = o.mDescriptors.data(); O.n_kps = o.N.data(); O.kp_capacity = kp_cap_;
            if (has_map_) { o.match_of_kp.assign(K, -1); o.n_kp_matches.assign(n, 0); O.match_of_kp = o.match_of_kp.data(); O.n_kp_matches = o.n_kp_matches.data(); }
        }
        if (nlines_ > 0) {
            o.mvKeylines.assign(Lc, plf_keyline()); o.mLdesc.assign(Lc * 32, 0); o.mvKeyLineFunctions.assign(Lc * 3, 0.0); o.NL.assign(n, 0);
            O.lines = o.mvKeylines.data(); O.ldesc = o.mLdesc.data(); O.line_eq = o.mvKeyLineFunctions.data(); O.n_lines = o.NL.data(); O.line_capacity = nlines_;
            if (has_map_) { o.match_of_line.assign(Lc, -1); o.n_line_matches.assign(n, 0); O.match_of_line = o.match_of_line.data(); O.n_line_matches = o.n_line_matches.data(); }
        }
        int st;
        if (!cam) st = plf_batch_extract(b_, images, n, width, height, pitch, frame_stride, &O);
        else {
            plf_batch_rgbd R;
            std::memset(&R, 0, sizeof(R));
            R.cam = *cam; R.depth_factor = factor; R.depth = depth; R.depth_pitch_elems = dpitch; R.depth_frame_stride_elems = dstride;
            if (nfeatures_ > 0) {
                o.mvKeysUn.assign(K, plf_keypoint()); o.mvuRight.assign(K, -1.f); o.mvDepth.assign(K, -1.f);
                R.kps_un = o.mvKeysUn.data(); R.uright = o.mvuRight.data(); R.kp_depth = o.mvDepth.data();
            }
            if (nlines_ > 0) {
                o.mvKeylinesUn.assign(Lc, plf_keyline());
                o.mvuRightLineStart.assign(Lc, -1.f); o.mvuRightLineEnd.assign(Lc, -1.f); o.mvDepthLineStart.assign(Lc, -1.f); o.mvDepthLineEnd.assign(Lc, -1.f);
                R.lines_un = o.mvKeylinesUn.data(); R.uright_start = o.mvuRightLineStart.data(); R.uright_end = o.mvuRightLineEnd.data();
                R.depth_start = o.mvDepthLineStart.data(); R.depth_end = o.mvDepthLineEnd.data();
            }
            st = plf_batch_extract_rgbd(b_, images, n, width, height, pitch, frame_stride, &O, &R);
        }
        if (st != PLF_OK && st != PLF_E_CAPACITY && st != PLF_E_EMPTY) check(st, "plf_batch_extract");
        return st;
    }
    plf_batch *b_ = nullptr;
    int nfeatures_, nlines_, kp_cap_;
    bool has_map_ = false;
};

// ORB_SLAM2::ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (include/ORBVocabulary.h, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h):
// loadFromTextFile, transform (Frame::ComputeBoW include/Frame.h:80, KeyFrame::ComputeBoW include/KeyFrame.h:77) and score on the GPU.
struct BowFlat {   // one frame's BowVector and FeatureVector as flat arrays (the layout plf_bow_view / plf_tri_view read)
    std::vector<uint32_t> word_id; std::vector<double> word_val;           // ascending word id
    std::vector<uint32_t> node_id; std::vector<int32_t> node_start, feat;  // ascending node id, CSR starts (nodes + 1), feature indices
};
class ORBVocabulary {
public:
    explicit ORBVocabulary(int device = 0) : device_(device) {}
    ~ORBVocabulary() { plf_vocab_destroy(v_); }
    ORBVocabulary(const ORBVocabulary &) = delete;
    ORBVocabulary &operator=(const ORBVocabulary &) = delete;
    // bool loadFromTextFile(const std::string &filename)  TemplatedVocabulary.h:1362 -- false for an unreadable or malformed file, as the reference;
    // a missing GPU is not a property of the file and throws.
    bool loadFromTextFile(const std::string &filename)
    {
        plf_vocab_destroy(v_); v_ = nullptr;
        const int st = plf_vocab_load_text(filename.c_str(), device_, &v_);
        if (st == PLF_E_BADARG || st == PLF_E_EMPTY) return false;
        check(st, "plf_vocab_load_text");
        return true;
    }
    void create(const plf_vocab_desc &d) { plf_vocab_destroy(v_); v_ = nullptr; check(plf_vocab_create(&d, device_, &v_), "plf_vocab_create"); }
    bool empty() const { return v_ == nullptr; }
    plf_vocab_info_t info() const { plf_vocab_info_t i{}; check(plf_vocab_info(v_, &i), "plf_vocab_info"); return i; }
    unsigned size() const { return empty() ? 0u : (unsigned)info().n_words; }
    plf_vocab *handle() const { return v_; }
    // transform(features, v, fv, levelsup)  TemplatedVocabulary.h:1151 -- desc: n x 32 bytes in HOST memory; flat vectors out
    void transform(const uint8_t *desc, int n, BowFlat &out, int levelsup) const
    {
        out = BowFlat();
        if (empty() || n <= 0) return;   // :1158
        out.word_id.resize(n); out.word_val.resize(n); out.node_id.resize(n); out.node_start.resize((size_t)n + 1); out.feat.resize(n);
        int32_t nw = 0, nn = 0;
        check(plf_bow_transform(v_, desc, n, levelsup, PLF_MEM_HOST, PLF_MEM_HOST, out.word_id.data(), out.word_val.data(), &nw, out.node_id.data(),
                                out.node_start.data(), out.feat.data(), &nn, nullptr), "plf_bow_transform");
        out.word_id.resize(nw); out.word_val.resize(nw); out.node_id.resize(nn); out.node_start.resize((size_t)nn + 1);
        out.feat.resize(out.node_start[nn]);
    }
    // double score(const BowVector &v1, const BowVector &v2)  TemplatedVocabulary.h:1223 -- flat vectors, ascending word id
    double score(const std::vector<uint32_t> &id1, const std::vector<double> &val1, const std::vector<uint32_t> &id2, const std::vector<double> &val2) const
    {
        const int32_t start[2] = {0, (int32_t)id2.size()};
        double out = 0.0;
        check(plf_bow_score(v_, id1.data(), val1.data(), (int32_t)id1.size(), id2.data(), val2.data(), start, 1, &out, PLF_MEM_HOST, nullptr), "plf_bow_score");
        return out;
    }
protected:
    plf_vocab *v_ = nullptr;
    int device_;
};

// ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h:48-58) over slots: add / erase / clear, DetectLoopCandidates, DetectRelocalizationCandidates
// on the GPU (plf_kfdb_*, include/plf.h "Keyframe database").  This form takes one query in HOST vectors and waits for its result; a pipeline that
// keeps its vectors on the device and queries in batches uses add_device / the C entry points with handle().
class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary &voc, int max_keyframes, int capacity) : S_(max_keyframes), C_(capacity)
    {
        check(plf_kfdb_create(voc.handle(), max_keyframes, capacity, &db_), "plf_kfdb_create");
        device_ = plf_vocab_device(voc.handle());
    }
    ~KeyFrameDatabase() { plf_kfdb_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;
    plf_kfdb *handle() const { return db_; }
    plf_kfdb_info_t info() const { plf_kfdb_info_t i{}; check(plf_kfdb_info(db_, &i), "plf_kfdb_info"); return i; }
    // void add(KeyFrame *pKF): the keyframe's mBowVec as flat ascending vectors, stored in `slot`
    void add(int slot, const std::vector<uint32_t> &word_id, const std::vector<double> &word_val)
    {
        const int32_t n = (int32_t)word_id.size(), s = slot;
        if (word_val.size() != word_id.size() || n > C_) throw Error(PLF_E_BADARG, "KeyFrameDatabase::add");
        DeviceArray<uint32_t> di((size_t)C_, device_); DeviceArray<double> dv((size_t)C_, device_); DeviceArray<int32_t> dn(1, device_);
        if (n > 0) { di.upload(word_id.data(), (size_t)n); dv.upload(word_val.data(), (size_t)n); }
        dn.upload(&n, 1);
        add_device(di.get(), dv.get(), dn.get(), 1, C_, &s, nullptr);
        wait();                                          // the staging arrays go out of scope
    }
    // n keyframes straight from plf_bow_transform_batch's device output; only enqueues
    void add_device(const uint32_t *word_id, const double *word_val, const int32_t *n_words, int n, int capacity, const int32_t *slots, void *stream)
    {
        check(plf_kfdb_add_batch(db_, word_id, word_val, n_words, n, capacity, slots, stream), "plf_kfdb_add_batch");
    }
    void erase(int slot) { const int32_t s = slot; check(plf_kfdb_erase_batch(db_, &s, 1), "plf_kfdb_erase_batch"); }
    void clear() { check(plf_kfdb_clear(db_), "plf_kfdb_clear"); }
    // covis_start / covis_slot: CSR over the slots (max_keyframes + 1 starts) of mvpOrderedConnectedKeyFrames, -1 = a keyframe outside the database;
    // both empty = no neighbours.  Returns the candidate slots in the reference's order.
    std::vector<int32_t> DetectRelocalizationCandidates(const std::vector<uint32_t> &word_id, const std::vector<double> &word_val,
                                                        const std::vector<int32_t> &covis_start, const std::vector<int32_t> &covis_slot,
                                                        plf_kfdb_stats *stats = nullptr)
    {
        return detect(false, word_id, word_val, covis_start, covis_slot, std::vector<int32_t>(), 0.0f, stats);
    }
    // connected: the slots of pKF->GetConnectedKeyFrames() (and pKF's own, if it was added), any order
    std::vector<int32_t> DetectLoopCandidates(const std::vector<uint32_t> &word_id, const std::vector<double> &word_val, float minScore,
                                              const std::vector<int32_t> &connected, const std::vector<int32_t> &covis_start,
                                              const std::vector<int32_t> &covis_slot, plf_kfdb_stats *stats = nullptr)
    {
        return detect(true, word_id, word_val, covis_start, covis_slot, connected, minScore, stats);
    }
private:
    void wait() { DeviceArray<int32_t> d(1, device_); (void)d.download(); }   // a NULL-stream download waits for the device first
    std::vector<int32_t> detect(bool loop, const std::vector<uint32_t> &word_id, const std::vector<double> &word_val, const std::vector<int32_t> &covis_start,
                                const std::vector<int32_t> &covis_slot, const std::vector<int32_t> &connected, float minScore, plf_kfdb_stats *stats)
    {
        const int32_t n = (int32_t)word_id.size();
        if (word_val.size() != word_id.size() || (!covis_start.empty() && covis_start.size() != (size_t)S_ + 1)) throw Error(PLF_E_BADARG, "KeyFrameDatabase::Detect");
        const int cap = n > 0 ? n : 1;
        DeviceArray<uint32_t> di((size_t)cap, device_); DeviceArray<double> dv((size_t)cap, device_); DeviceArray<int32_t> dn(1, device_);
        if (n > 0) { di.upload(word_id.data(), (size_t)n); dv.upload(word_val.data(), (size_t)n); }
        dn.upload(&n, 1);
        DeviceArray<int32_t> dcs(covis_start.size() + 1, device_), dci(covis_slot.size() + 1, device_), dcand((size_t)S_, device_), dnc(1, device_), dst(4, device_);
        if (!covis_start.empty()) dcs.upload(covis_start.data(), covis_start.size());
        if (!covis_slot.empty()) dci.upload(covis_slot.data(), covis_slot.size());
        const int32_t *cs = covis_start.empty() ? nullptr : dcs.get(), *ci = covis_start.empty() ? nullptr : dci.get();
        if (loop) {
            const int32_t es[2] = {0, (int32_t)connected.size()};
            DeviceArray<int32_t> des(2, device_), dei(connected.size() + 1, device_);
            DeviceArray<float> dms(1, device_);
            des.upload(es, 2); dms.upload(&minScore, 1);
            if (!connected.empty()) dei.upload(connected.data(), connected.size());
            check(plf_kfdb_detect_loop(db_, di.get(), dv.get(), dn.get(), 1, cap, cs, ci, des.get(), dei.get(), dms.get(), S_, dcand.get(), dnc.get(),
                                       (plf_kfdb_stats *)dst.get(), nullptr), "plf_kfdb_detect_loop");
            wait();
        } else
            check(plf_kfdb_detect_reloc(db_, di.get(), dv.get(), dn.get(), 1, cap, cs, ci, S_, dcand.get(), dnc.get(), (plf_kfdb_stats *)dst.get(), nullptr),
                  "plf_kfdb_detect_reloc");
        const std::vector<int32_t> nc = dnc.download();  // a NULL-stream download waits for the device first
        std::vector<int32_t> out = dcand.download();
        out.resize((size_t)nc[0]);
        if (stats) { const std::vector<int32_t> st = dst.download(); memcpy(stats, st.data(), sizeof(*stats)); }
        return out;
    }
    plf_kfdb *db_ = nullptr;
    int S_, C_, device_ = 0;
};

// The local map of tracked frames over arrays the caller keeps on the device (include/plf.h, "Local map"): plf_local_keyframes, then plf_local_items, for
// n_rows frames per call; Gather / Visible are plf_local_gather / plf_local_visible on the lists it holds.  Every call only enqueues on `stream` (the fills
// that leave -1 beyond the counts included), so an object reused frame after frame on one stream is ordered behind its own readers there; readers on
// OTHER streams are the caller's to order.  Nothing is read back: the members are the device lists, to be handed on to the frustum and projection calls or downloaded by the caller.
class LocalMap {
public:
    struct Graph {   // the covisibility rows and the spanning tree by slot: plf_local_kf_view without the seed
        const int32_t *covis_kf, *n_covis; int32_t covis_stride; const int32_t *child_start, *child_kf, *kf_parent; const uint8_t *kf_bad; int32_t n_kf;
    };
    struct Rows {    // each keyframe's mvpMapPoints (mvpMapLines) by slot
        const int32_t *kf_row_start, *kf_row_item; const uint8_t *item_bad; int32_t n_items;
    };
    LocalMap(int n_rows, int kf_stride, int item_stride, int device = 0)
        : local_kf((size_t)n_rows * kf_stride, device), n_local_kf(n_rows, device), kf_status(n_rows, device), local_item((size_t)n_rows * item_stride, device),
          n_local_item(n_rows, device), item_status(n_rows, device), seen((size_t)n_rows * item_stride, device), n_rows_(n_rows), kf_stride_(kf_stride),
          item_stride_(item_stride), device_(device) {}
    // seed_kf / n_seed: conn_kf / n_conn of a PLF_COVIS_VOTES call; frame_row_*: its rows (may be NULL: nothing is seen)
    void Update(const int32_t *seed_kf, const int32_t *n_seed, int seed_stride, const Graph &g, const Rows &r, const int32_t *frame_row_start = nullptr,
                const int32_t *frame_row_item = nullptr, void *stream = nullptr, int n_best = 10, int max_local = 80)
    {
        local_kf.fill(0xFF, stream);                                    // on the caller's stream: behind whatever still reads the lists there, and no host wait
        const plf_local_kf_view kv = {n_rows_, seed_kf, n_seed, seed_stride, g.covis_kf, g.n_covis, g.covis_stride, g.child_start, g.child_kf, g.kf_parent, g.kf_bad, g.n_kf};
        const plf_local_kf_params kp = {n_best, max_local, kf_stride_, 0};
        check(plf_local_keyframes(&kv, &kp, local_kf.get(), n_local_kf.get(), kf_status.get(), device_, stream), "Tracking::UpdateLocalKeyFrames");
        Items(g.n_kf, r, frame_row_start, frame_row_item, stream);
    }
    // UpdateLocalPoints alone, over whatever local_kf / n_local_kf hold
    void Items(int n_kf, const Rows &r, const int32_t *frame_row_start = nullptr, const int32_t *frame_row_item = nullptr, void *stream = nullptr)
    {
        const plf_local_items_view iv = {n_rows_, local_kf.get(), n_local_kf.get(), kf_stride_, r.kf_row_start, r.kf_row_item, n_kf, r.item_bad, r.n_items,
                                         frame_row_start, frame_row_item};
        const plf_local_items_params ip = {item_stride_, 0};
        local_item.fill(0xFF, stream); seen.fill(0, stream);
        check(plf_local_items(&iv, &ip, local_item.get(), n_local_item.get(), seen.get(), item_status.get(), device_, stream), "Tracking::UpdateLocalPoints");
    }
    void Gather(const plf_local_map_src &src, const plf_local_map_dst &dst, void *stream = nullptr) const
    {
        check(plf_local_gather(local_item.get(), n_local_item.get(), n_rows_, item_stride_, &src, &dst, device_, stream), "plf_local_gather");
    }
    // after plf_frustum_points / plf_frustum_lines on the gathered arrays: in_view &= !seen, n_to_match (n_rows), optionally the map's mnVisible
    void Visible(uint8_t *in_view, int32_t *n_to_match, int32_t *visible = nullptr, const int32_t *frame_row_start = nullptr, const int32_t *frame_row_item = nullptr,
                 const uint8_t *item_bad = nullptr, int n_items = 0, void *stream = nullptr) const
    {
        check(plf_local_visible(local_item.get(), n_local_item.get(), seen.get(), n_rows_, item_stride_, in_view, n_to_match, visible, frame_row_start, frame_row_item,
                                item_bad, n_items, device_, stream), "Tracking::SearchLocalPoints");
    }
    DeviceArray<int32_t> local_kf, n_local_kf, kf_status, local_item, n_local_item, item_status;
    DeviceArray<uint8_t> seen;
    int n_rows() const { return n_rows_; }
    int kf_stride() const { return kf_stride_; }
    int item_stride() const { return item_stride_; }
private:
    int n_rows_, kf_stride_, item_stride_, device_;
};

// The tail of Tracking::Track() over arrays the caller keeps on the device (include/plf.h, "Tracking tail"), stateless, any number of frames per call;
// every call only enqueues on `stream`.  Names follow the reference's members; points only, as the binary.
struct Tracking {
    // bool Tracking::NeedNewKeyFrame() (so@0x49750): counts (n_frames x 3: nTotal, nMap, nRefMatches) and decision (0 no, 1 insert, 2 the mapper is busy)
    static void NeedNewKeyFrame(const plf_track_view &v, const plf_track_kf_view &kf, const plf_track_kf_state *state_dev, const int32_t *mnMatchesInliers_dev,
                                float mThDepth, int32_t *counts_dev, int32_t *decision_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_track_need_keyframe(&v, &kf, state_dev, mnMatchesInliers_dev, mThDepth, counts_dev, decision_dev, device, stream), "Tracking::NeedNewKeyFrame");
    }
    // the point loop of void Tracking::CreateNewKeyFrame() (so@0x4e040): mvpMapPoints[new_kp] = id_base + k in place (v.match_of_kp is written)
    static void CreateNewKeyFrame(const plf_track_view &v, const plf_camera &cam, float mThDepth, const int32_t *id_base_dev, int new_stride, int32_t *new_kp_dev,
                                  float *new_pos_dev, int32_t *n_new_dev, int32_t *n_walked_dev, int32_t *status_dev, int device = 0, void *stream = nullptr,
                                  int min_points = 100)
    {
        const plf_track_close_params p = {mThDepth, min_points, id_base_dev ? PLF_TRACK_CLOSE_KEYFRAME : PLF_TRACK_CLOSE_LIST, new_stride};
        check(plf_track_close_points(&v, &cam, &p, id_base_dev, nullptr, new_kp_dev, new_pos_dev, n_new_dev, n_walked_dev, status_dev, device, stream),
              "Tracking::CreateNewKeyFrame");
    }
    // the temporal points of void Tracking::UpdateLastFrame() (so@0x4e570) into the arrays behind a plf_lastframe_view
    static void UpdateLastFrame(const plf_track_view &v, const plf_camera &cam, float mThDepth, const plf_track_lastframe_out &last, int new_stride, int32_t *new_kp_dev,
                                float *new_pos_dev, int32_t *n_new_dev, int32_t *n_walked_dev, int32_t *status_dev, int device = 0, void *stream = nullptr,
                                int min_points = 100)
    {
        const plf_track_close_params p = {mThDepth, min_points, PLF_TRACK_CLOSE_LASTFRAME, new_stride};
        check(plf_track_close_points(&v, &cam, &p, nullptr, &last, new_kp_dev, new_pos_dev, n_new_dev, n_walked_dev, status_dev, device, stream),
              "Tracking::UpdateLastFrame");
    }
    // mVelocity = mCurrentFrame.mTcw * LastTwc, SetPose(Tlr * pRef->GetPose()), SetPose(mVelocity * mLastFrame.mTcw): the products `flags` names
    static void MotionModel(int flags, int n_frames, const plf_pose34 *cur, const plf_frustum_pose *last_frustum, float *mVelocity, const plf_pose34 *last,
                            const plf_pose34 *Tlr, const plf_pose34 *Tref, plf_pose34 *last_out, plf_frustum_pose *last_frustum_out, plf_pose34 *pose_pred,
                            plf_frustum_pose *frustum_pred, int32_t *status_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_track_motion(flags, n_frames, cur, last_frustum, mVelocity, last, Tlr, Tref, last_out, last_frustum_out, pose_pred, frustum_pred, status_dev, device,
                               stream), "Tracking::MotionModel");
    }
    // "Clean VO matches" (PLF_TRACK_CLEAN_VO) and the outlier matches nulled after the key-frame decision (PLF_TRACK_CLEAN_OUTLIERS)
    static void CleanMatches(int mode, int32_t *mvpMapPoints_dev, uint8_t *mvbOutlier_dev, const int32_t *n_dev, int n_host, int n_frames, int kp_stride,
                             const int32_t *row_id, int id_stride, const int32_t *n_obs, int n_points, int device = 0, void *stream = nullptr)
    {
        check(plf_track_clean(mode, mvpMapPoints_dev, mvbOutlier_dev, n_dev, n_host, n_frames, kp_stride, row_id, id_stride, n_obs, n_points, device, stream),
              "Tracking::CleanMatches");
    }
};

// The loop body of void LocalMapping::CreateNewMapPoints() (so@0x5ce60) over keyframes the caller keeps on the device (include/plf.h, "New map points"),
// stateless, any number of (current keyframe, neighbour) jobs per call; the call only enqueues on `stream`.  match12 is what
// ORBmatcher::SearchForTriangulation wrote; with `marks` the next neighbour's search, enqueued behind this call, sees the new points.
struct Triangulator {
    static void CreateNewMapPoints(const plf_triangulate_view &keyframes, const plf_camera &cam, const plf_triangulate_jobs &jobs, const plf_triangulate_marks *marks,
                                   int32_t *new_i1_dev, int32_t *new_i2_dev, float *new_pos_dev, int32_t *n_new_dev, int32_t *status_dev, uint8_t *reason_dev,
                                   int device = 0, void *stream = nullptr)
    {
        check(plf_triangulate_points(&keyframes, &cam, &jobs, marks, new_i1_dev, new_i2_dev, new_pos_dev, n_new_dev, status_dev, reason_dev, device, stream),
              "LocalMapping::CreateNewMapPoints");
    }
    // one pair's outcome from its reason byte
    static bool Created(uint8_t reason) { return (reason & 15) == PLF_TRI_CREATED; }
    static int Branch(uint8_t reason) { return reason & PLF_TRI_BRANCH_MASK; }
};

// The Sim3 solver section of include/plf.h over arrays this object owns: n_jobs solvers, their pair sets, RANSAC state, raw random values, counts and
// hits.  Pairs() is Sim3Solver's constructor + SetRansacParameters for all jobs in one launch, Iterate() is iterate(n) for all in one call; both only
// enqueue on `stream`.  The table of SetRansacParameters (host libm) is filled and uploaded by SetRansacParameters().
class Sim3Batch {
public:
    Sim3Batch(int n_jobs, int kp_stride, int pair_stride, int rand_stride, int max_hits, int device = 0)
        : J(n_jobs), S(kp_stride), PS(pair_stride), RS(rand_stride), MH(max_hits), device_(device), idx1((size_t)J * PS, device), max_err1((size_t)J * PS, device),
          max_err2((size_t)J * PS, device), n_pairs(J, device), status(J, device), iterations_done(J, device), best_inliers(J, device), best_iter(J, device),
          max_its(J, device), count((size_t)J * RS, device), n_hits(J, device), hit_iter((size_t)J * MH, device), hit_inliers((size_t)J * MH, device),
          rand3((size_t)J * RS * 3, device), table((size_t)PS + 1, device), x3dc1((size_t)J * PS * 3, device), x3dc2((size_t)J * PS * 3, device),
          p1im1((size_t)J * PS * 2, device), p2im2((size_t)J * PS * 2, device), best_sim3((size_t)J * 13, device), hit_sim3((size_t)J * MH * 13, device),
          no_more(J, device), fix_scale(J, device), hit_inlier12((size_t)J * MH * S, device)
    {
    }
    void SetRansacParameters(double probability, int minInliers, int maxIterations)
    {
        std::vector<int32_t> t((size_t)PS + 1);
        check(plf_sim3_its_for_n(probability, minInliers, maxIterations, PS, t.data()), "Sim3Solver::SetRansacParameters");
        table.upload(t.data(), t.size());
        min_inliers = minInliers;
    }
    void Pairs(const plf_sim3_view &keyframes, const plf_camera &cam, const int32_t *job_kf1_dev, const int32_t *job_kf2_dev, const int32_t *match12_dev,
               void *stream = nullptr)
    {
        cam_ = cam;
        const plf_sim3_jobs jobs = {J, S, PS, job_kf1_dev, job_kf2_dev, match12_dev, fix_scale.get()};
        const plf_sim3_pairset p = pairset();
        const plf_sim3_state st = state();
        check(plf_sim3_pairs(&keyframes, &cam, &jobs, table.get(), &p, &st, device_, stream), "Sim3Solver::Sim3Solver");
    }
    void Iterate(int nIterations, const uint8_t *active_dev = nullptr, void *stream = nullptr)
    {
        const plf_sim3_jobs jobs = {J, S, PS, nullptr, nullptr, nullptr, fix_scale.get()};
        const plf_sim3_pairset p = pairset();
        const plf_sim3_state st = state();
        const plf_sim3_hits h = {MH, n_hits.get(), hit_iter.get(), hit_inliers.get(), hit_sim3.get(), hit_inlier12.get()};
        check(plf_sim3_iterate(&jobs, &cam_, &p, rand3.get(), RS, nIterations, min_inliers, active_dev, &st, count.get(), &h, device_, stream), "Sim3Solver::iterate");
    }
    // ComputeSim3's `vpMapPointMatches[i] = vbInliers[i] ? matches[i] : NULL` for every job, from the FIRST stored hit of the last Iterate(): match12_dev
    // (J x S, the rows Pairs() read, or a copy of them) is changed in place.  Needs max_hits == 1 (the hit rows are then kp_stride apart).
    void KeepInliers(int32_t *match12_dev, const int32_t *kf_n_of_job_dev = nullptr, void *stream = nullptr)
    {
        if (MH != 1) throw std::runtime_error("Sim3Batch::KeepInliers: max_hits must be 1");
        check(plf_sim3_keep_inliers(match12_dev, hit_inlier12.get(), kf_n_of_job_dev, J, S, device_, stream), "ComputeSim3: keep inliers");
    }
    // Optimizer::OptimizeSim3 of every job in one launch, started from sim3_in_dev (J x 13; default: the first stored hit of the last Iterate(), max_hits
    // == 1) with the jobs' fix_scale: match12_dev is vpMatches1 IN/OUT; sim3_out_dev J x 8 doubles (g2oS12: qx qy qz qw tx ty tz s), scw_out_dev J x 16
    // floats or NULL (mScw for plf_match_project_sim3 / plf_match_fuse_sim3), n_inliers_dev and status_dev J.  Only enqueues on `stream`.
    void Optimize(const plf_sim3_view &keyframes, const plf_camera &cam, const int32_t *job_kf1_dev, const int32_t *job_kf2_dev, int32_t *match12_dev,
                  const float *inv_level_sigma2_dev, float th2, double *sim3_out_dev, float *scw_out_dev, int32_t *n_inliers_dev, int32_t *status_dev,
                  const float *sim3_in_dev = nullptr, void *stream = nullptr)
    {
        if (!sim3_in_dev && MH != 1) throw std::runtime_error("Sim3Batch::Optimize: give sim3_in_dev, or store one hit per job");
        const plf_sim3opt_jobs jobs = {J, S, job_kf1_dev, job_kf2_dev, sim3_in_dev ? sim3_in_dev : hit_sim3.get(), fix_scale.get(), inv_level_sigma2_dev, th2};
        check(plf_sim3_optimize(&keyframes, &cam, &jobs, match12_dev, sim3_out_dev, scw_out_dev, n_inliers_dev, status_dev, device_, stream), "Optimizer::OptimizeSim3");
    }
    plf_sim3_pairset pairset() const { return {idx1.get(), x3dc1.get(), x3dc2.get(), max_err1.get(), max_err2.get(), p1im1.get(), p2im2.get(), n_pairs.get(), status.get()}; }
    plf_sim3_state state() const { return {iterations_done.get(), best_inliers.get(), best_iter.get(), max_its.get(), best_sim3.get(), no_more.get()}; }
    const int J, S, PS, RS, MH;
    int min_inliers = 6;
private:
    int device_;
    plf_camera cam_ = {};
public:
    DeviceArray<int32_t> idx1, max_err1, max_err2, n_pairs, status, iterations_done, best_inliers, best_iter, max_its, count, n_hits, hit_iter, hit_inliers, rand3, table;
    DeviceArray<float> x3dc1, x3dc2, p1im1, p2im2, best_sim3, hit_sim3;
    DeviceArray<uint8_t> no_more, fix_scale, hit_inlier12;
};

// LoopClosing::CorrectLoop's Sim3 pose propagation and map-point moves over the resident map (plf.h, "Loop correction"): the RAII form over the per-call
// arrays of the four calls -- K ranks (the entries of CorrectedSim3 in the caller's iteration order), n_points points, n_kf keyframe slots.  Everything a
// method takes is DEVICE memory; every method only enqueues on `stream`.  After Run(): corrected[r] is the Scw plf_match_fuse_sim3 takes for rank r
// (Converter::toCvMat of it, a host argument), owner_rank[p] the rank that moved point p (-1: left alone), n_obs_used what its UpdateNormalAndDepth counted.
// The two tails (OptimizeEssentialGraph, RunGlobalBundleAdjustment) are the static members: stateless calls.
class LoopCorrection {
public:
    LoopCorrection(int K_, int n_points_, int n_kf_, int device = 0)
        : K(K_), n_points(n_points_), n_kf(n_kf_), device_(device), corrected((size_t)std::max(K_, 1) * 8, device), noncorrected((size_t)std::max(K_, 1) * 8, device),
          scw(8, device), tcw_new(std::max(K_, 1), device), ow_new((size_t)std::max(K_, 1) * 3, device), owner_rank(std::max(n_points_, 1), device),
          n_obs_used(std::max(n_points_, 1), device), kf_rank(std::max(n_kf_, 1), device) {}
    // mg2oScw = gScm * Sim3(Rmw, tmw, 1.0) from a sim3_out row of plf_sim3_optimize, kept in `scw`
    void Scw(const double *scm_dev, const plf_pose34 *kf_tcw_dev, int matched_slot, void *stream = nullptr)
    {
        check(plf_loop_scw(scm_dev, kf_tcw_dev, n_kf, matched_slot, scw.get(), device_, stream), "ComputeSim3: mg2oScw");
    }
    // the two loops of CorrectLoop.  rank_kf_host: the host copy of rows.rank_kf (the rank of each slot is built from it and uploaded).
    void Run(const plf_loop_view &rows, int cur_slot, int64_t cur_kf_id, plf_pose34 *kf_tcw_dev, float *kf_ow_dev, const plf_map_geom_view &observations,
             float *world_pos_dev, int64_t *corrected_by_dev, int64_t *corrected_ref_dev, float *normal_dev, float *min_distance_dev, float *max_distance_dev,
             const std::vector<int32_t> &rank_kf_host, void *stream = nullptr)
    {
        std::vector<int32_t> rank(std::max(n_kf, 1), -1);
        for (int r = 0; r < K && r < (int)rank_kf_host.size(); r++)
            if (rank_kf_host[r] >= 0 && rank_kf_host[r] < n_kf) rank[rank_kf_host[r]] = r;
        kf_rank.upload(rank.data(), rank.size());             // (synchronous: `rank` is a local)
        check(plf_loop_sim3_pairs(kf_tcw_dev, kf_ow_dev, n_kf, rows.rank_kf, K, cur_slot, scw.get(), corrected.get(), noncorrected.get(), device_, stream),
              "CorrectLoop: CorrectedSim3");
        check(plf_loop_correct_points(&rows, corrected.get(), noncorrected.get(), cur_kf_id, world_pos_dev, corrected_by_dev, corrected_ref_dev, owner_rank.get(), device_,
                                      stream), "CorrectLoop: map points");
        check(plf_loop_new_poses(corrected.get(), K, tcw_new.get(), ow_new.get(), device_, stream), "CorrectLoop: poses");
        if (n_points > 0)
            check(plf_loop_normal_depth(&observations, kf_rank.get(), ow_new.get(), K, owner_rank.get(), world_pos_dev, normal_dev, min_distance_dev, max_distance_dev,
                                        n_points, n_obs_used.get(), device_, stream), "CorrectLoop: UpdateNormalAndDepth");
        check(plf_loop_commit_poses(rows.rank_kf, K, tcw_new.get(), ow_new.get(), kf_tcw_dev, kf_ow_dev, n_kf, device_, stream), "CorrectLoop: SetPose");
    }
    // the end of Optimizer::OptimizeEssentialGraph: SetPose of every keyframe from corrected_siw_dev (n_kf x 8), then the point loop.  The UpdateNormalAndDepth()
    // of that loop is NOT in here: the caller runs plf_map_update_normal_depth (MapPoint::UpdateNormalAndDepth) next, with the new centres.
    static void EssentialGraphTail(const double *corrected_siw_dev, const double *vScw_dev, const double *vCorrectedSwc_dev, int n_kf, plf_pose34 *kf_tcw_dev,
                                   float *kf_ow_dev, plf_pose34 *tcw_new_dev, float *ow_new_dev, const int32_t *every_slot_dev, int n_points, const uint8_t *point_bad_dev,
                                   const int32_t *ref_kf_dev, const int64_t *corrected_by_dev, const int64_t *corrected_ref_dev, int64_t cur_kf_id,
                                   const int32_t *id_to_slot_dev, int64_t n_ids, float *world_pos_dev, uint8_t *moved_dev = nullptr, int device = 0, void *stream = nullptr)
    {
        check(plf_loop_new_poses(corrected_siw_dev, n_kf, tcw_new_dev, ow_new_dev, device, stream), "OptimizeEssentialGraph: poses");
        check(plf_loop_commit_poses(every_slot_dev, n_kf, tcw_new_dev, ow_new_dev, kf_tcw_dev, kf_ow_dev, n_kf, device, stream), "OptimizeEssentialGraph: SetPose");
        check(plf_loop_correct_points_by_ref(n_points, point_bad_dev, ref_kf_dev, corrected_by_dev, corrected_ref_dev, cur_kf_id, id_to_slot_dev, n_ids, vScw_dev,
                                             vCorrectedSwc_dev, n_kf, world_pos_dev, moved_dev, device, stream), "OptimizeEssentialGraph: map points");
    }
    // the end of LoopClosing::RunGlobalBundleAdjustment
    static void GlobalBundleAdjustmentTail(const plf_gba_view &tree, int n_points, const uint8_t *point_bad_dev, const uint8_t *point_flag_dev, const float *pos_gba_dev,
                                           const int32_t *ref_kf_dev, float *world_pos_dev, int device = 0, void *stream = nullptr)
    {
        check(plf_gba_propagate_poses(&tree, device, stream), "RunGlobalBundleAdjustment: poses");
        check(plf_gba_correct_points(n_points, point_bad_dev, point_flag_dev, pos_gba_dev, ref_kf_dev, tree.kf_flag, tree.tcw_bef, tree.kf_tcw, tree.kf_ow, tree.n_kf,
                                     world_pos_dev, device, stream), "RunGlobalBundleAdjustment: map points");
    }
    const int K, n_points, n_kf;
private:
    int device_;
public:
    DeviceArray<double> corrected, noncorrected, scw;
    DeviceArray<plf_pose34> tcw_new;
    DeviceArray<float> ow_new;
    DeviceArray<int32_t> owner_rank, n_obs_used, kf_rank;
};

}  // namespace plf

// ---------------------------------------------------------------------------------------------------------------
// Drop-in adapters with the EXACT reference signatures; compiled only where OpenCV (+ contrib line_descriptor) headers exist
// (tests/mock/ holds a minimal stand-in so that tests/test_abi.py can at least compile them in this image).
// The matcher adapters are templates over the reference's own Frame / KeyFrame / MapPoint / MapLine classes (include/Frame.h,
// KeyFrame.h, MapPoint.h, MapLine.h): they read exactly the members the reference bodies read, flatten them into the plf_*_view
// structs, run the device search and write the result back into mvpMapPoints / mvpMapLines -- the state the reference loop leaves.
// ---------------------------------------------------------------------------------------------------------------
#if defined(PLF_WITH_OPENCV) && defined(__has_include)
#if __has_include(<opencv2/core.hpp>)
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <opencv2/core.hpp>
#include <opencv2/features2d.hpp>
#include <opencv2/line_descriptor/descriptor.hpp>
namespace ORB_SLAM2_PLF {
static_assert(sizeof(cv::KeyPoint) == sizeof(plf_keypoint), "cv::KeyPoint must be 28 bytes");
static_assert(sizeof(cv::line_descriptor::KeyLine) == sizeof(plf_keyline), "cv::line_descriptor::KeyLine must be 68 bytes");

class ORBextractor : public plf::ORBextractor {
public:
    using plf::ORBextractor::ORBextractor;
    using plf::ORBextractor::operator();
    // include/ORBextractor.h:59-61
    void operator()(cv::InputArray image, cv::InputArray /*mask*/, std::vector<cv::KeyPoint> &keypoints, cv::OutputArray descriptors)
    {
        if (image.empty()) return;  // so@0x76dda
        cv::Mat im = image.getMat();
        CV_Assert(im.type() == CV_8UC1);
        std::vector<plf_keypoint> k;
        std::vector<uint8_t> d;
        plf::ORBextractor::operator()(im.data, im.cols, im.rows, (ptrdiff_t)im.step, k, d);
        keypoints.resize(k.size());
        if (!k.empty()) memcpy((void *)keypoints.data(), k.data(), k.size() * sizeof(plf_keypoint));
        if (k.empty()) { descriptors.release(); return; }
        descriptors.create((int)k.size(), 32, CV_8U);
        memcpy(descriptors.getMat().data, d.data(), d.size());
    }
};

// include/ExtractLineSegment.h:29-57.  Vector3dT = Eigen::Vector3d in the reference (any type with operator()(int) or [] assignable from double works).
class LineSegment : public plf::LineSegment {
public:
    using plf::LineSegment::LineSegment;
    using plf::LineSegment::ExtractLineSegment;
    // void ExtractLineSegment(const Mat &img, vector<KeyLine> &keylines, Mat &ldesc, vector<Vector3d> &keylineFunctions, int scale = 1.2, int numOctaves = 1)
    template <class Vector3dT>
    void ExtractLineSegment(const cv::Mat &img, std::vector<cv::line_descriptor::KeyLine> &keylines, cv::Mat &ldesc, std::vector<Vector3dT> &keylineFunctions,
                            int scale = 1.2, int numOctaves = 1)
    {
        keylines.clear(); keylineFunctions.clear();
        if (img.empty()) { ldesc.release(); return; }
        CV_Assert(img.type() == CV_8UC1);
        std::vector<plf_keyline> kl;
        std::vector<uint8_t> d;
        std::vector<plf::Vector3d> eq;
        plf::LineSegment::ExtractLineSegment(img.data, img.cols, img.rows, (ptrdiff_t)img.step, kl, d, eq, scale, numOctaves);
        keylines.resize(kl.size());
        if (!kl.empty()) memcpy((void *)keylines.data(), kl.data(), kl.size() * sizeof(plf_keyline));
        if (kl.empty()) { ldesc.release(); return; }
        ldesc.create((int)kl.size(), 32, CV_8U);
        memcpy(ldesc.data, d.data(), d.size());
        keylineFunctions.resize(eq.size());
        for (size_t i = 0; i < eq.size(); i++) { keylineFunctions[i][0] = eq[i].v[0]; keylineFunctions[i][1] = eq[i].v[1]; keylineFunctions[i][2] = eq[i].v[2]; }
    }
};

namespace detail {
inline std::vector<uint8_t> rows32(const cv::Mat &m)   // n x 32 CV_8U, rows possibly strided -> packed
{
    std::vector<uint8_t> out((size_t)m.rows * 32);
    for (int r = 0; r < m.rows; r++) memcpy(&out[(size_t)r * 32], m.data + (size_t)r * m.step, 32);
    return out;
}
// ---- cv::Mat (CV_32F) <-> the float arrays of the C ABI.  A 3-vector is read with at<float>(k): a 3 x 1 or a 1 x 3 matrix.
inline void put3(float *dst, const cv::Mat &v) { for (int k = 0; k < 3; k++) dst[k] = v.at<float>(k); }
inline void put3(std::vector<float> &dst, const cv::Mat &v) { dst.resize(dst.size() + 3); put3(&dst[dst.size() - 3], v); }
inline plf_pose34 pose34(const cv::Mat &Tcw)   // 3 x 4 or 4 x 4
{
    plf_pose34 T;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) T.Tcw[4 * r + c] = Tcw.at<float>(r, c);
    return T;
}
inline void pose34(const cv::Mat &Tcw, float *R, float *t)
{
    const plf_pose34 T = pose34(Tcw);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) R[3 * r + c] = T.Tcw[4 * r + c]; t[r] = T.Tcw[4 * r + 3]; }
}
inline plf_frustum_pose frustum_pose(const cv::Mat &Rcw, const cv::Mat &tcw, const cv::Mat &Ow = cv::Mat())   // an empty tcw / Ow stays 0
{
    plf_frustum_pose p = {};
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) p.Rcw[3 * r + c] = Rcw.at<float>(r, c);
    if (!tcw.empty()) put3(p.tcw, tcw);
    if (!Ow.empty()) put3(p.Ow, Ow);
    return p;
}
inline cv::Mat mat31(const float *v) { cv::Mat m(3, 1, CV_32F); memcpy(m.data, v, 3 * sizeof(float)); return m; }   // (a new matrix is continuous)
inline cv::Mat mat44(const plf_pose34 &T)   // [Rcw | tcw] over the row 0 0 0 1
{
    const float last[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    cv::Mat m(4, 4, CV_32F);
    memcpy(m.data, T.Tcw, sizeof(T.Tcw)); memcpy(m.data + sizeof(T.Tcw), last, sizeof(last));
    return m;
}

// ---- rows of map points -> point ids, observation CSR and keyframe slots: the host walk of every adapter that starts from the reference's map objects.
// Slots and ids are handed out in order of first appearance, so the order in which an adapter calls slot() / point() / row() is part of its result.
// The adapter's own arrays are filled by three callables, inlined into the one pass: onKeyFrame(pKF) when a keyframe gets its slot, onObservation(pKF, idx)
// per appended observation, onPoint(gatherer, pMP, observations) when a point gets its id, after its observations are appended.
struct Ignore { template <class... A> void operator()(A &&...) const {} };
template <class KeyFrameT> using MapPointOf =
    typename std::remove_pointer<typename std::decay<decltype(std::declval<KeyFrameT &>().GetMapPointMatches())>::type::value_type>::type;
template <class PointT> using KeyFrameOf =
    typename std::remove_pointer<typename std::decay<decltype(std::declval<PointT &>().GetObservations())>::type::key_type>::type;
// THE rule for empty device arrays: the C ABI accepts them (0 bytes allocate, upload and download fine), and an array that is indexed through a CSR gets one
// element of padding beyond its ranges, never read, appended here and nowhere else: -1 for indices, 0 for flags and values.
template <class T, class U> const std::vector<T> &padded(std::vector<T> &v, U pad) { v.push_back((T)pad); return v; }
template <class KeyFrameT, class MapPointT, class OnKeyFrame = Ignore, class OnPoint = Ignore, class OnObservation = Ignore> struct MapGather {
    std::vector<KeyFrameT *> kfs;                                   // by slot
    std::vector<MapPointT *> pts;                                   // by id
    std::vector<int32_t> row_start{0}, row_point, obs_start{0}, obs_kf;
    std::vector<uint8_t> point_bad;
    explicit MapGather(OnKeyFrame k = OnKeyFrame(), OnPoint p = OnPoint(), OnObservation o = OnObservation()) : on_kf_(k), on_point_(p), on_obs_(o) {}
    int slot(KeyFrameT *pKF)
    {
        const auto at = slot_.emplace(pKF, (int)kfs.size());
        if (at.second) { kfs.push_back(pKF); on_kf_(pKF); }
        return at.first->second;
    }
    // one range of the observation CSR, in the std::map's order (the point-list adapters, which give no ids, call this per entry)
    template <class Observations> void observed(const Observations &observations)
    {
        for (const auto &ob : observations) { obs_kf.push_back(slot(ob.first)); on_obs_(ob.first, (size_t)ob.second); }
        obs_start.push_back((int32_t)obs_kf.size());
    }
    // with_observations = false: an id and a bad flag only (a point that only fills rows; all such points come after the observed ones)
    int point(MapPointT *pMP, bool with_observations = true)
    {
        const auto at = id_.emplace(pMP, (int)pts.size());
        if (at.second) {
            pts.push_back(pMP); point_bad.push_back(pMP->isBad());
            if (with_observations) { const auto observations = pMP->GetObservations(); observed(observations); on_point_(*this, pMP, observations); }
        }
        return at.first->second;
    }
    void row(const std::vector<MapPointT *> &points, bool with_observations = true)
    {
        for (MapPointT *pMP : points) row_point.push_back(pMP ? point(pMP, with_observations) : -1);
        row_start.push_back((int32_t)row_point.size());
    }
    // the upload: the five arrays as they stand, the indexed ones padded
    struct Device {
        plf::DeviceArray<int32_t> row_start, row_point, obs_start, obs_kf;
        plf::DeviceArray<uint8_t> point_bad;
        Device(MapGather &g, int device)
            : row_start(g.row_start, device), row_point(padded(g.row_point, -1), device), obs_start(g.obs_start, device), obs_kf(padded(g.obs_kf, -1), device),
              point_bad(padded(g.point_bad, 0), device) {}
    };
private:
    std::unordered_map<KeyFrameT *, int> slot_;
    std::unordered_map<MapPointT *, int> id_;
    OnKeyFrame on_kf_;
    OnPoint on_point_;
    OnObservation on_obs_;
};
template <class KeyFrameT, class MapPointT, class OnKeyFrame = Ignore, class OnPoint = Ignore, class OnObservation = Ignore>
MapGather<KeyFrameT, MapPointT, OnKeyFrame, OnPoint, OnObservation> map_gather(OnKeyFrame k = OnKeyFrame(), OnPoint p = OnPoint(), OnObservation o = OnObservation())
{
    return MapGather<KeyFrameT, MapPointT, OnKeyFrame, OnPoint, OnObservation>(k, p, o);
}
// MapPoint::UpdateNormalAndDepth's reference keyframe and level, as its operator[] resolves them: none (-1, level 0) without a reference keyframe or an
// observation; index 0 for a reference keyframe that does not observe the point; octave 0 for an index beyond mvKeysUn.  The scale table of the first
// reference keyframe met serves the call (`scale` is filled once): every keyframe of a map carries the same one.
template <class Gather, class KeyFrameT, class Observations>
void ref_level(Gather &g, KeyFrameT *pRefKF, const Observations &observations, std::vector<float> &scale, int32_t &ref, int32_t &level)
{
    ref = -1; level = 0;
    if (!pRefKF || observations.empty()) return;
    ref = g.slot(pRefKF);
    const auto it = observations.find(pRefKF);
    const size_t idx = it == observations.end() ? 0 : it->second;
    level = idx < pRefKF->mvKeysUn.size() ? pRefKF->mvKeysUn[idx].octave : 0;
    if (scale.empty()) scale.assign(pRefKF->mvScaleFactors.begin(), pRefKF->mvScaleFactors.begin() + pRefKF->mnScaleLevels);
}
}  // namespace detail

// include/ORBmatcher.h:36-140, the two tracking overloads with their reference signatures
class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
    ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0, int maxKeypoints = 8192, int maxMapPoints = 65535)
        : mfNNratio(nnratio), mbCheckOrientation(checkOri), device_(device)
    {
        plf::check(plf_matcher_create(device, maxKeypoints, maxMapPoints, 1024, 1, &m_), "plf_matcher_create");
    }
    ~ORBmatcher() { plf_matcher_destroy(m_); }
    ORBmatcher(const ORBmatcher &) = delete;
    ORBmatcher &operator=(const ORBmatcher &) = delete;
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b) { return plf_hamming256(a.data, b.data); }   // include/ORBmatcher.h:44

    // int SearchByProjection(Frame &F, const std::vector<MapPoint*> &vpMapPoints, const float th = 3)   include/ORBmatcher.h:61
    template <class FrameT, class MapPointT> int SearchByProjection(FrameT &F, const std::vector<MapPointT *> &vpMapPoints, const float th = 3)
    {
        const int N = (int)F.mvKeysUn.size(), M = (int)vpMapPoints.size();
        if (N == 0 || M == 0) return 0;
        std::vector<float> px(M), py(M), pxr(M), vc(M);
        std::vector<int32_t> lvl(M);
        std::vector<uint8_t> inview(M), obs(M), desc((size_t)M * 32);
        for (int i = 0; i < M; i++) {
            MapPointT *p = vpMapPoints[i];
            inview[i] = p && p->mbTrackInView && !p->isBad();
            if (!inview[i]) continue;
            px[i] = p->mTrackProjX; py[i] = p->mTrackProjY; pxr[i] = p->mTrackProjXR; lvl[i] = p->mnTrackScaleLevel; vc[i] = p->mTrackViewCos;
            obs[i] = p->Observations() > 0;
            const cv::Mat d = p->GetDescriptor();
            memcpy(&desc[(size_t)i * 32], d.data, 32);
        }
        std::vector<int32_t> init(N, -1);
        for (int k = 0; k < N; k++)
            if (F.mvpMapPoints[k] && F.mvpMapPoints[k]->Observations() > 0) init[k] = -2;
        plf::DeviceArray<plf_keypoint> dk(N, device_); dk.upload(F.mvKeysUn.data(), N);
        plf::DeviceArray<float> dur(F.mvuRight, device_), dsc(F.mvScaleFactors, device_);
        plf::DeviceArray<uint8_t> dd(detail::rows32(F.mDescriptors), device_), dmd(desc, device_), div(inview, device_), dob(obs, device_);
        plf::DeviceArray<float> dpx(px, device_), dpy(py, device_), dpxr(pxr, device_), dvc(vc, device_);
        plf::DeviceArray<int32_t> dl(lvl, device_), dm(init, device_), dn(1, device_);
        plf_frame_view fv = {N, nullptr, dk.get(), dur.get(), dd.get(), FrameT::mnMinX, FrameT::mnMinY, FrameT::mnMaxX, FrameT::mnMaxY, dsc.get(),
                             (int32_t)F.mvScaleFactors.size()};
        plf_mappoint_view mv = {M, dpx.get(), dpy.get(), dpxr.get(), dl.get(), dvc.get(), div.get(), dmd.get(), dob.get()};
        plf::check(plf_match_project_points(m_, &fv, 1, &mv, th, mfNNratio, dm.get(), N, dn.get(), nullptr), "ORBmatcher::SearchByProjection");
        const std::vector<int32_t> match = dm.download();
        for (int k = 0; k < N; k++)
            if (match[k] >= 0) F.mvpMapPoints[k] = vpMapPoints[match[k]];
        return dn.download()[0];
    }

    // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)   include/ORBmatcher.h:78
    template <class FrameT> int SearchByProjection(FrameT &CurrentFrame, const FrameT &LastFrame, const float th, const bool bMono)
    {
        const int N = (int)CurrentFrame.mvKeysUn.size(), NLst = (int)LastFrame.mvKeys.size();
        if (N == 0 || NLst == 0) return 0;
        std::vector<uint8_t> has(NLst), outl(NLst), obs(NLst), desc((size_t)NLst * 32);
        std::vector<float> xw((size_t)NLst * 3);
        for (int i = 0; i < NLst; i++) {
            auto *p = LastFrame.mvpMapPoints[i];
            has[i] = p != nullptr; outl[i] = LastFrame.mvbOutlier[i];
            if (!p) continue;
            obs[i] = p->Observations() > 0;
            detail::put3(&xw[(size_t)i * 3], p->GetWorldPos());
            const cv::Mat d = p->GetDescriptor();
            memcpy(&desc[(size_t)i * 32], d.data, 32);
        }
        std::vector<int32_t> init(N, -1);
        for (int k = 0; k < N; k++)
            if (CurrentFrame.mvpMapPoints[k] && CurrentFrame.mvpMapPoints[k]->Observations() > 0) init[k] = -2;
        plf_pose_pair P;
        detail::pose34(CurrentFrame.mTcw, P.Rcw, P.tcw); detail::pose34(LastFrame.mTcw, P.Rlw, P.tlw);
        P.fx = FrameT::fx; P.fy = FrameT::fy; P.cx = FrameT::cx; P.cy = FrameT::cy; P.bf = CurrentFrame.mbf; P.b = CurrentFrame.mb;
        plf::DeviceArray<plf_keypoint> dk(N, device_), dlk(NLst, device_);
        dk.upload(CurrentFrame.mvKeysUn.data(), N); dlk.upload(LastFrame.mvKeysUn.data(), NLst);
        plf::DeviceArray<float> dur(CurrentFrame.mvuRight, device_), dsc(CurrentFrame.mvScaleFactors, device_), dxw(xw, device_);
        plf::DeviceArray<uint8_t> dd(detail::rows32(CurrentFrame.mDescriptors), device_), dh(has, device_), dou(outl, device_), dob(obs, device_), dmd(desc, device_);
        plf::DeviceArray<int32_t> dm(init, device_), dn(1, device_);
        plf_frame_view fv = {N, nullptr, dk.get(), dur.get(), dd.get(), FrameT::mnMinX, FrameT::mnMinY, FrameT::mnMaxX, FrameT::mnMaxY, dsc.get(),
                             (int32_t)CurrentFrame.mvScaleFactors.size()};
        plf_lastframe_view lv = {NLst, dh.get(), dou.get(), dxw.get(), dlk.get(), dmd.get(), dob.get()};
        plf::check(plf_match_project_lastframe(m_, &fv, &lv, &P, th, bMono, mbCheckOrientation ? 2 : 0, dm.get(), dn.get(), nullptr), "ORBmatcher::SearchByProjection(last frame)");
        const std::vector<int32_t> match = dm.download();
        for (int k = 0; k < N; k++) {
            if (match[k] >= 0) CurrentFrame.mvpMapPoints[k] = LastFrame.mvpMapPoints[match[k]];
            else if (match[k] == -3) CurrentFrame.mvpMapPoints[k] = NULL;   // assigned, then removed by the rotation-consistency check: NULL in the reference, whatever the key point held before
        }
        return dn.download()[0];
    }
    plf_matcher *handle() { return m_; }

private:
    plf_matcher *m_ = nullptr;
    float mfNNratio;
    bool mbCheckOrientation;
    int device_;
};

// include/LSDmatcher.h:27-78, the three SearchByProjection overloads with their reference signatures (+ SearchForTriangulation / Fuse)
class LSDmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
    LSDmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0, int maxLines = 4096, int maxMapLines = 65535)
        : mfNNratio(nnratio), mbCheckOrientation(checkOri), device_(device)
    {
        plf::check(plf_matcher_create(device, 1, maxMapLines, maxLines, 1, &m_), "plf_matcher_create");
    }
    ~LSDmatcher() { plf_matcher_destroy(m_); }
    LSDmatcher(const LSDmatcher &) = delete;
    LSDmatcher &operator=(const LSDmatcher &) = delete;
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b) { return plf_hamming256(a.data, b.data); }   // include/LSDmatcher.h:43

    // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th = 3, const bool bMono = false)   include/LSDmatcher.h:32
    template <class FrameT> int SearchByProjection(FrameT &CurrentFrame, const FrameT &LastFrame, const float /*th*/ = 3, const bool /*bMono*/ = false)
    {
        return knn_assign(LastFrame.mLdesc, LastFrame.mvpMapLines, CurrentFrame.mLdesc, CurrentFrame.mvpMapLines);
    }
    // int SearchByProjection(KeyFrame *pKF, Frame &F, std::vector<MapLine*> &vpMapLineMatches)   include/LSDmatcher.h:35
    template <class KeyFrameT, class FrameT, class MapLineT> int SearchByProjection(KeyFrameT *pKF, FrameT &F, std::vector<MapLineT *> &vpMapLineMatches)
    {
        vpMapLineMatches.assign((size_t)F.mLdesc.rows, nullptr);
        const std::vector<MapLineT *> kfLines = pKF->GetMapLineMatches();
        return knn_assign(pKF->mLineDescriptors, kfLines, F.mLdesc, vpMapLineMatches);
    }
    // int SearchByProjection(Frame &F, const std::vector<MapLine*> &vpMapLines, const float th = 3)   include/LSDmatcher.h:40
    template <class FrameT, class MapLineT> int SearchByProjection(FrameT &F, const std::vector<MapLineT *> &vpMapLines, const float th = 3)
    {
        const int NL = (int)F.mvKeylinesUn.size(), M = (int)vpMapLines.size();
        if (NL == 0 || M == 0) return 0;
        std::vector<float> x1(M), y1(M), x2(M), y2(M), vc(M);
        std::vector<int32_t> lvl(M);
        std::vector<uint8_t> inview(M), desc((size_t)M * 32);
        for (int i = 0; i < M; i++) {
            MapLineT *p = vpMapLines[i];
            inview[i] = p && p->mbTrackInView && !p->isBad();
            if (!inview[i]) continue;
            x1[i] = p->mTrackProjX1; y1[i] = p->mTrackProjY1; x2[i] = p->mTrackProjX2; y2[i] = p->mTrackProjY2; lvl[i] = p->mnTrackScaleLevel; vc[i] = p->mTrackViewCos;
            const cv::Mat d = p->GetDescriptor();
            memcpy(&desc[(size_t)i * 32], d.data, 32);
        }
        std::vector<int32_t> init(NL, -1);
        for (int k = 0; k < NL; k++)
            if (F.mvpMapLines[k] && F.mvpMapLines[k]->Observations() > 0) init[k] = -2;
        plf::DeviceArray<plf_keyline> dkl(NL, device_); dkl.upload(F.mvKeylinesUn.data(), NL);
        plf::DeviceArray<float> dsc(F.mvScaleFactors, device_), dx1(x1, device_), dy1(y1, device_), dx2(x2, device_), dy2(y2, device_), dvc(vc, device_);
        plf::DeviceArray<uint8_t> dd(detail::rows32(F.mLdesc), device_), dmd(desc, device_), div(inview, device_);
        plf::DeviceArray<int32_t> dl(lvl, device_), dm(init, device_), dn(1, device_);
        plf_lineframe_view fv = {NL, nullptr, dkl.get(), dd.get(), dsc.get()};
        plf_mapline_view mv = {M, dx1.get(), dy1.get(), dx2.get(), dy2.get(), dl.get(), dvc.get(), div.get(), dmd.get()};
        plf::check(plf_match_project_lines(m_, &fv, 1, &mv, th, mfNNratio, dm.get(), NL, dn.get(), nullptr), "LSDmatcher::SearchByProjection");
        const std::vector<int32_t> match = dm.download();
        for (int k = 0; k < NL; k++)
            if (match[k] >= 0) F.mvpMapLines[k] = vpMapLines[match[k]];
        return dn.download()[0];
    }
    // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, vector<pair<size_t, size_t>> &vMatchedPairs, const bool bOnlyStereo)   include/LSDmatcher.h:54
    template <class KeyFrameT> int SearchForTriangulation(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<std::pair<size_t, size_t>> &vMatchedPairs, const bool bOnlyStereo)
    {
        vMatchedPairs.clear();
        const int n1 = pKF1->mLineDescriptors.rows, n2 = pKF2->mLineDescriptors.rows;
        if (n1 == 0 || n2 < 2) return 0;
        std::vector<uint8_t> h1(n1), h2(n2), s1(n1), s2(n2);
        for (int i = 0; i < n1; i++) { h1[i] = pKF1->GetMapLine(i) != nullptr; s1[i] = pKF1->mvuRightLineStart[i] >= 0 && pKF1->mvuRightLineEnd[i] >= 0; }
        for (int i = 0; i < n2; i++) { h2[i] = pKF2->GetMapLine(i) != nullptr; s2[i] = pKF2->mvuRightLineStart[i] >= 0 && pKF2->mvuRightLineEnd[i] >= 0; }
        plf::DeviceArray<uint8_t> d1(detail::rows32(pKF1->mLineDescriptors), device_), d2(detail::rows32(pKF2->mLineDescriptors), device_), dh1(h1, device_),
            dh2(h2, device_), ds1(s1, device_), ds2(s2, device_);
        plf::DeviceArray<int32_t> dm(n1, device_), dn(1, device_);
        plf::check(plf_match_lines_triangulation(m_, d1.get(), n1, d2.get(), n2, dh1.get(), dh2.get(), ds1.get(), ds2.get(), bOnlyStereo, 0.1f, dm.get(), dn.get(), nullptr),
                   "LSDmatcher::SearchForTriangulation");
        const std::vector<int32_t> match = dm.download();
        for (int q = 0; q < n1; q++)
            if (match[q] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)q, (size_t)match[q]));
        return (int)vMatchedPairs.size();
    }
    // int Fuse(KeyFrame *pKF, const vector<MapLine*> &vpMapLines)   include/LSDmatcher.h:58: the device search, then the reference's map mutation in list order
    template <class KeyFrameT, class MapLineT> int Fuse(KeyFrameT *pKF, const std::vector<MapLineT *> &vpMapLines)
    {
        const int nkf = pKF->mLineDescriptors.rows, M = (int)vpMapLines.size();
        if (M == 0) return 0;
        std::vector<uint8_t> valid(M), desc((size_t)M * 32);
        for (int i = 0; i < M; i++) {
            MapLineT *p = vpMapLines[i];
            valid[i] = p && !p->isBad() && !p->IsInKeyFrame(pKF);
            if (!valid[i]) continue;
            const cv::Mat d = p->GetDescriptor();
            memcpy(&desc[(size_t)i * 32], d.data, 32);
        }
        plf::DeviceArray<uint8_t> dk(detail::rows32(pKF->mLineDescriptors), device_), dmd(desc, device_), dv(valid, device_);
        plf::DeviceArray<int32_t> db(M, device_), dn(1, device_);
        plf::check(plf_match_lines_fuse(m_, dk.get(), nkf, dmd.get(), dv.get(), M, db.get(), dn.get(), nullptr), "LSDmatcher::Fuse");
        const std::vector<int32_t> best = db.download();
        int nFused = 0;
        for (int i = 0; i < M; i++) {
            if (best[i] < 0) continue;
            MapLineT *pML = vpMapLines[i], *pMLinKF = pKF->GetMapLine((size_t)best[i]);
            if (pMLinKF) {
                if (!pMLinKF->isBad()) { if (pMLinKF->Observations() > pML->Observations()) pML->Replace(pMLinKF); else pMLinKF->Replace(pML); }
            } else { pML->AddObservation(pKF, (size_t)best[i]); pKF->AddMapLine(pML, (size_t)best[i]); }
            nFused++;
        }
        return nFused;
    }
    plf_matcher *handle() { return m_; }

private:
    // the brute-force kNN + MAD rule shared by the two frame / keyframe overloads: query = the side that holds MapLines, train = the frame being filled
    template <class VecQ, class VecT> int knn_assign(const cv::Mat &qdesc, const VecQ &qlines, const cv::Mat &tdesc, VecT &tlines)
    {
        const int nq = qdesc.rows, nt = tdesc.rows;
        if (nq == 0 || nt < 2) return 0;
        std::vector<uint8_t> has(nq);
        for (int q = 0; q < nq; q++) has[q] = qlines[q] != nullptr;
        plf::DeviceArray<uint8_t> dq(detail::rows32(qdesc), device_), dt(detail::rows32(tdesc), device_), dh(has, device_);
        plf::DeviceArray<int32_t> dm(nt, device_), dn(1, device_);
        dm.fill(0xFF);
        plf::check(plf_match_lines_lastframe(m_, dq.get(), nq, dt.get(), nt, dh.get(), dm.get(), dn.get(), nullptr), "LSDmatcher::SearchByProjection(kNN)");
        const std::vector<int32_t> match = dm.download();
        for (int t = 0; t < nt; t++)
            if (match[t] >= 0) tlines[t] = qlines[match[t]];
        return dn.download()[0];
    }
    plf_matcher *m_ = nullptr;
    float mfNNratio;
    bool mbCheckOrientation;
    int device_;
};
// include/ORBVocabulary.h: ORBVocabulary::transform / score with the reference's signatures.  BowVectorT = DBoW2::BowVector (a std::map<WordId, WordValue>),
// FeatureVectorT = DBoW2::FeatureVector (a std::map<NodeId, std::vector<unsigned int>>): templates, so that this header needs no DBoW2 header.
class ORBVocabulary : public plf::ORBVocabulary {
public:
    using plf::ORBVocabulary::ORBVocabulary;
    using plf::ORBVocabulary::transform;
    using plf::ORBVocabulary::score;
    // void transform(const std::vector<TDescriptor> &features, BowVector &v, FeatureVector &fv, int levelsup) const   TemplatedVocabulary.h:1151
    template <class BowVectorT, class FeatureVectorT>
    void transform(const std::vector<cv::Mat> &features, BowVectorT &v, FeatureVectorT &fv, int levelsup) const
    {
        v.clear(); fv.clear();
        std::vector<uint8_t> d(features.size() * 32);
        for (size_t i = 0; i < features.size(); i++) memcpy(&d[i * 32], features[i].data, 32);   // FORB::TDescriptor: 1 x 32 CV_8U
        plf::BowFlat f;
        plf::ORBVocabulary::transform(d.data(), (int)features.size(), f, levelsup);
        for (size_t i = 0; i < f.word_id.size(); i++) v.insert(v.end(), typename BowVectorT::value_type(f.word_id[i], f.word_val[i]));
        for (size_t j = 0; j < f.node_id.size(); j++) {
            auto &dst = fv[f.node_id[j]];
            dst.assign(f.feat.begin() + f.node_start[j], f.feat.begin() + f.node_start[j + 1]);
        }
    }
    // double score(const BowVector &a, const BowVector &b) const   TemplatedVocabulary.h:1223
    template <class BowVectorT>
    double score(const BowVectorT &a, const BowVectorT &b) const
    {
        std::vector<uint32_t> ia, ib; std::vector<double> va, vb;
        for (const auto &e : a) { ia.push_back(e.first); va.push_back(e.second); }
        for (const auto &e : b) { ib.push_back(e.first); vb.push_back(e.second); }
        return plf::ORBVocabulary::score(ia, va, ib, vb);
    }
};

// include/KeyFrameDatabase.h:48-58 with the reference's signatures over its own KeyFrame / Frame classes (templates, so that this header needs none of
// the reference's).  Keeps the pointer <-> slot table, stages mBowVec at add and at every query, and reads GetBestCovisibilityKeyFrames(10) of every
// stored keyframe and pKF->GetConnectedKeyFrames() from the objects at query time (a keyframe outside the database becomes -1).
// The price of starting from host objects, as with the map adapter below: add() finds a free slot by a linear scan over max_keyframes, and EVERY QUERY
// rebuilds and uploads the covisibility CSR of all stored keyframes (one GetBestCovisibilityKeyFrames(10) per stored keyframe), stages the query vector,
// allocates its device arrays and waits for the result.  It exists for signature parity; a caller that keeps its vectors and its covisibility CSR on
// the device uses plf::KeyFrameDatabase::add_device / the C entry points and uploads nothing per query.
template <class KeyFrameT, class FrameT> class KeyFrameDatabase {
public:
    explicit KeyFrameDatabase(const plf::ORBVocabulary &voc, int max_keyframes = 4096, int capacity = 2048)
        : db_(voc, max_keyframes, capacity), kf_((size_t)max_keyframes, nullptr) {}
    void add(KeyFrameT *pKF)
    {
        if (slot_.count(pKF)) return;
        int s = 0;
        while (s < (int)kf_.size() && kf_[s]) s++;
        if (s == (int)kf_.size()) throw plf::Error(PLF_E_CAPACITY, "KeyFrameDatabase::add");
        std::vector<uint32_t> id; std::vector<double> val;
        flat(pKF->mBowVec, id, val);
        db_.add(s, id, val);
        kf_[s] = pKF; slot_[pKF] = s;
    }
    void erase(KeyFrameT *pKF)
    {
        const auto it = slot_.find(pKF);
        if (it == slot_.end()) return;
        db_.erase(it->second);
        kf_[it->second] = nullptr; slot_.erase(it);
    }
    void clear() { db_.clear(); slot_.clear(); std::fill(kf_.begin(), kf_.end(), nullptr); }
    std::vector<KeyFrameT *> DetectLoopCandidates(KeyFrameT *pKF, float minScore)
    {
        std::vector<uint32_t> id; std::vector<double> val;
        flat(pKF->mBowVec, id, val);
        std::vector<int32_t> conn, cs, ci;
        for (KeyFrameT *c : pKF->GetConnectedKeyFrames()) { const auto it = slot_.find(c); if (it != slot_.end()) conn.push_back(it->second); }
        const auto self = slot_.find(pKF);
        if (self != slot_.end()) conn.push_back(self->second);   // the reference's walk meets pKF itself only through mnLoopQuery == mnId: never a candidate
        covis(cs, ci);
        return pointers(db_.DetectLoopCandidates(id, val, minScore, conn, cs, ci));
    }
    std::vector<KeyFrameT *> DetectRelocalizationCandidates(FrameT *F)
    {
        std::vector<uint32_t> id; std::vector<double> val;
        flat(F->mBowVec, id, val);
        std::vector<int32_t> cs, ci;
        covis(cs, ci);
        return pointers(db_.DetectRelocalizationCandidates(id, val, cs, ci));
    }
    plf::KeyFrameDatabase &device() { return db_; }
private:
    template <class BowVectorT> static void flat(const BowVectorT &v, std::vector<uint32_t> &id, std::vector<double> &val)
    {
        for (const auto &e : v) { id.push_back(e.first); val.push_back(e.second); }
    }
    void covis(std::vector<int32_t> &cs, std::vector<int32_t> &ci)
    {
        cs.assign(kf_.size() + 1, 0);
        for (size_t s = 0; s < kf_.size(); s++) {
            if (kf_[s])
                for (KeyFrameT *n : kf_[s]->GetBestCovisibilityKeyFrames(10)) { const auto it = slot_.find(n); ci.push_back(it == slot_.end() ? -1 : it->second); }
            cs[s + 1] = (int32_t)ci.size();
        }
    }
    std::vector<KeyFrameT *> pointers(const std::vector<int32_t> &slots) const
    {
        std::vector<KeyFrameT *> out;
        for (int32_t s : slots) out.push_back(kf_[s]);
        return out;
    }
    plf::KeyFrameDatabase db_;
    std::vector<KeyFrameT *> kf_;
    std::unordered_map<KeyFrameT *, int> slot_;
};

// MapPoint::ComputeDistinctiveDescriptors / MapLine::ComputeDistinctiveDescriptors for a LIST of points of the reference's own types (what LocalMapping
// runs after Fuse and after CreateNewMapPoints / CreateNewMapLines).  Walks GetObservations() (the std::map's order), KeyFrame::isBad() and the keyframes'
// descriptor matrices, builds the CSR and calls plf_map_distinctive_descriptors in its indirect form.  EVERY CALL uploads the whole descriptor matrix of
// every keyframe the listed points are observed from (once per keyframe and call): that is the price of starting from host cv::Mat members, and it is
// only worth paying for a long list.  A caller whose keyframe descriptors already live on the device uses the C entry point and uploads nothing.
// mDescriptor / mLDescriptor are protected in the reference: the forwarder inside MapPoint.cc / MapLine.cc assigns desc.row(i).
struct DistinctiveDescriptors {
    cv::Mat desc;                               // points x 32 CV_8U: row i = the new mDescriptor of point i (meaningful where best_obs[i] >= 0)
    std::vector<int32_t> best_obs, best_median; // position in the point's GetObservations() order (bad keyframes counted), -1 = leave mDescriptor alone
};
namespace detail {
template <class PointT, class DescOf> DistinctiveDescriptors distinctive(const std::vector<PointT *> &points, DescOf descOf, int device)
{
    DistinctiveDescriptors out;
    const int P = (int)points.size();
    out.best_obs.assign(P, -1); out.best_median.assign(P, -1);
    out.desc.create(P, 32, CV_8U);
    if (P == 0) return out;
    memset(out.desc.data, 0, (size_t)P * 32);
    typedef KeyFrameOf<PointT> KeyFrameT;
    std::vector<int32_t> idx;
    std::vector<uint8_t> valid;
    std::vector<std::vector<uint8_t>> rows;
    auto g = map_gather<KeyFrameT, PointT>([&](KeyFrameT *pKF) { rows.push_back(rows32(descOf(pKF))); }, Ignore(),
                                           [&](KeyFrameT *pKF, size_t i) { idx.push_back((int32_t)i); valid.push_back(!pKF->isBad()); });
    for (PointT *p : points) {                                      // one range per entry, a point listed twice included; a null entry: an empty range
        if (p) g.observed(p->GetObservations());
        else g.obs_start.push_back(g.obs_start.back());
    }
    const size_t n_kf = g.kfs.size();
    if (g.obs_kf.empty()) return out;
    std::vector<plf::DeviceArray<uint8_t>> dkf(n_kf);
    std::vector<const uint8_t *> table(n_kf);
    for (size_t k = 0; k < n_kf; k++) {
        dkf[k].reset(rows[k].size() + 32, device);
        if (!rows[k].empty()) dkf[k].upload(rows[k].data(), rows[k].size());
        table[k] = dkf[k].get();
    }
    plf::DeviceArray<int32_t> dstart(g.obs_start, device), dk(g.obs_kf, device), di(idx, device), dbo(P, device), dbm(P, device);
    plf::DeviceArray<uint8_t> dv(valid, device), dmap((size_t)P * 32, device);
    plf::DeviceArray<const uint8_t *> dtab(table, device);
    dmap.fill(0);
    plf_map_obs_view v = {P, dstart.get(), nullptr, dk.get(), di.get(), dtab.get(), (int32_t)n_kf, dv.get(), nullptr};
    plf::check(plf_map_distinctive_descriptors(&v, dmap.get(), P, dbo.get(), dbm.get(), device, nullptr), "ComputeDistinctiveDescriptors");
    const std::vector<uint8_t> d = dmap.download();          // a NULL-stream download waits for the device first
    memcpy(out.desc.data, d.data(), d.size());
    out.best_obs = dbo.download(); out.best_median = dbm.download();
    return out;
}
}  // namespace detail
template <class MapPointT> DistinctiveDescriptors ComputeDistinctiveDescriptors(const std::vector<MapPointT *> &vpMapPoints, int device = 0)
{
    return detail::distinctive(vpMapPoints, [](auto *pKF) -> const cv::Mat & { return pKF->mDescriptors; }, device);
}
template <class MapLineT> DistinctiveDescriptors ComputeDistinctiveLineDescriptors(const std::vector<MapLineT *> &vpMapLines, int device = 0)
{
    return detail::distinctive(vpMapLines, [](auto *pKF) -> const cv::Mat & { return pKF->mLineDescriptors; }, device);
}
// MapPoint::UpdateNormalAndDepth for a LIST of points of the reference's own types (the statement after ComputeDistinctiveDescriptors() in LocalMapping,
// loop closing and after the bundle adjustments).  Reads isBad(), GetObservations() (the std::map's order), GetReferenceKeyFrame(), GetWorldPos(),
// pKF->GetCameraCenter(), and of the reference keyframe mvKeysUn, mvScaleFactors and mnScaleLevels (the scale table of the first reference keyframe met
// serves the call: every keyframe of a map carries the same one).  The level is resolved on the host, as operator[] does it (index 0 for a reference
// keyframe that does not observe the point), and goes to the device in the packed form.  Uploads once per call; for ONE point the adapter is slower
// than the loop it replaces.  mNormalVector / mfMinDistance / mfMaxDistance are protected in the reference: the forwarder inside MapPoint.cc assigns
// them.  A null entry of the list is treated like a bad point.
struct NormalAndDepth {
    std::vector<float> normal;                  // points x 3: the new mNormalVector of point i (meaningful where n[i] > 0)
    std::vector<float> minDistance, maxDistance;
    std::vector<int32_t> n;                     // observations counted, -1 = leave the three members alone (bad point, no observation)
};
template <class MapPointT> NormalAndDepth UpdateNormalAndDepth(const std::vector<MapPointT *> &vpMapPoints, int device = 0)
{
    NormalAndDepth out;
    const int P = (int)vpMapPoints.size();
    out.normal.assign((size_t)P * 3, 0.0f); out.minDistance.assign(P, 0.0f); out.maxDistance.assign(P, 0.0f); out.n.assign(P, -1);
    if (P == 0) return out;
    typedef detail::KeyFrameOf<MapPointT> KeyFrameT;
    std::vector<int32_t> ref(P, -1), level(P, 0);
    std::vector<uint8_t> bad(P, 1);
    std::vector<float> pos((size_t)P * 3, 0.0f), ow, scale;
    auto g = detail::map_gather<KeyFrameT, MapPointT>([&](KeyFrameT *pKF) { detail::put3(ow, pKF->GetCameraCenter()); });
    for (int i = 0; i < P; i++) {                                   // one range per entry, a point listed twice included; null or bad: an empty range
        MapPointT *pMP = vpMapPoints[i];
        if (pMP && !pMP->isBad()) {
            bad[i] = 0;
            const auto observations = pMP->GetObservations();
            detail::put3(&pos[(size_t)i * 3], pMP->GetWorldPos());
            g.observed(observations);
            detail::ref_level(g, pMP->GetReferenceKeyFrame(), observations, scale, ref[i], level[i]);
        } else g.obs_start.push_back(g.obs_start.back());
    }
    if (g.obs_kf.empty() || scale.empty()) return out;
    plf::DeviceArray<int32_t> dstart(g.obs_start, device), dk(g.obs_kf, device), dref(ref, device), dlevel(level, device), dn(P, device);
    plf::DeviceArray<uint8_t> dbad(bad, device);
    plf::DeviceArray<float> dpos(pos, device), dow(ow, device), dscale(scale, device), dnormal(out.normal, device), dmin(out.minDistance, device),
        dmax(out.maxDistance, device);
    plf_map_geom_view v = {};
    v.n_points = P; v.obs_start = dstart.get(); v.obs_kf = dk.get(); v.kf_ow = dow.get(); v.n_kf = (int32_t)g.kfs.size(); v.ref_kf = dref.get();
    v.ref_level = dlevel.get(); v.scale_factors = dscale.get(); v.nlevels = (int32_t)scale.size(); v.point_bad = dbad.get(); v.pos_floats = 3;
    plf::check(plf_map_update_normal_depth(&v, dpos.get(), dnormal.get(), dmin.get(), dmax.get(), P, dn.get(), device, nullptr), "UpdateNormalAndDepth");
    out.normal = dnormal.download();                       // a NULL-stream download waits for the device first
    out.minDistance = dmin.download(); out.maxDistance = dmax.download(); out.n = dn.download();
    return out;
}
// The covisibility graph over the reference's own KeyFrame / MapPoint / Frame classes: KeyFrame::UpdateConnections (so@0x9fb60) for a LIST of keyframes in
// one device call, and the KeyFrame queries that read its result -- GetConnectedKeyFrames (so@0x9c7c0), GetVectorCovisibleKeyFrames,
// GetBestCovisibilityKeyFrames (so@0x9cdb0), GetCovisiblesByWeight (so@0x9cff0) -- with the keyframe as first argument, because the lists live here and
// not in the keyframe.  Meant for the lists of keyframes a SLAM thread touches at a time, tens to a few thousand.  kf_key is the keyframe's ADDRESS, so ties resolve exactly as the reference's std::map<KeyFrame*, int> does.  What stays with the
// caller: AddConnection on the OTHER keyframes (or list every keyframe, which recomputes every row), mbFirstConnection / mpParent / AddChild (Parent() names
// the front of the ordered list).  EVERY CALL uploads the observation CSR of the points the listed keyframes hold: the price of starting from host
// pointer members; a caller whose CSR is resident uses plf_covis_count and uploads nothing.
template <class KeyFrameT, class MapPointT> class CovisibilityGraph {
public:
    struct Row {
        std::vector<KeyFrameT *> connected;        // mConnectedKeyFrameWeights in key (address) order ...
        std::vector<int> connectedWeights;         // ... and its weights
        std::vector<KeyFrameT *> ordered;          // mvpOrderedConnectedKeyFrames
        std::vector<int> orderedWeights;           // mvOrderedWeights
    };
    struct Votes {
        std::vector<KeyFrameT *> vpLocalKeyFrames; // in keyframeCounter order, bad keyframes left out: mvpLocalKeyFrames before its expansion
        std::vector<int> votes;
        KeyFrameT *pKFmax = nullptr;
        int max = 0;
    };
    explicit CovisibilityGraph(int device = 0, int first_stride = 256) : device_(device), first_stride_(std::max(first_stride, 1)) {}

    // pKF->UpdateConnections() for every keyframe of the list.  A keyframe whose KFcounter is empty keeps its lists, as in the reference.
    void UpdateConnections(const std::vector<KeyFrameT *> &vpKFs, int th = 15)
    {
        Gather g;
        std::vector<int32_t> row_self;
        for (KeyFrameT *pKF : vpKFs) {                  // slots: a row's owner before the observers its row brings
            row_self.push_back(g.slot(pKF));
            g.row(pKF->GetMapPointMatches());
        }
        if (vpKFs.empty()) return;
        const int R = (int)vpKFs.size(), S = (int)g.kfs.size();
        Device d(g, device_);
        plf::DeviceArray<int32_t> self(row_self, device_), cn(R, device_), on(R, device_), mk(R, device_), mw(R, device_), ck, cw, ok, ow;
        plf_covis_view v = d.view(R, S);
        v.row_self = self.get();
        // the outputs are R x stride: a first pass with a stride that holds an ordinary neighbourhood, and -- the counts are the true ones -- a second
        // pass at the longest list only if some row did not fit.  (R x S would be 1.6 GB for a whole graph of 10,000 keyframes.)
        int stride = std::max(1, std::min(S, first_stride_));
        std::vector<int32_t> hcn, hon;
        for (;;) {
            ck.reset((size_t)R * stride, device_); cw.reset((size_t)R * stride, device_); ok.reset((size_t)R * stride, device_); ow.reset((size_t)R * stride, device_);
            const plf_covis_params p = {PLF_COVIS_CONNECTIONS, th, stride, 0, 0};
            plf::check(plf_covis_count(&v, &p, ck.get(), cw.get(), cn.get(), ok.get(), ow.get(), on.get(), mk.get(), mw.get(), device_, nullptr),
                       "KeyFrame::UpdateConnections");
            hcn = cn.download(); hon = on.download();
            const int longest = *std::max_element(hcn.begin(), hcn.end());      // n_ord <= n_conn
            if (longest <= stride) break;
            stride = longest;
        }
        const std::vector<int32_t> hck = ck.download(), hcw = cw.download(), hok = ok.download(), how = ow.download();
        for (int r = 0; r < R; r++) {
            if (hcn[r] == 0) continue;
            Row &row = rows_[vpKFs[r]];
            row = Row();
            for (int i = 0; i < hcn[r]; i++) { row.connected.push_back(g.kfs[hck[(size_t)r * stride + i]]); row.connectedWeights.push_back(hcw[(size_t)r * stride + i]); }
            for (int i = 0; i < hon[r]; i++) { row.ordered.push_back(g.kfs[hok[(size_t)r * stride + i]]); row.orderedWeights.push_back(how[(size_t)r * stride + i]); }
        }
    }
    void UpdateConnections(KeyFrameT *pKF) { UpdateConnections(std::vector<KeyFrameT *>(1, pKF)); }

    std::set<KeyFrameT *> GetConnectedKeyFrames(KeyFrameT *pKF) const
    {
        const Row *r = find(pKF);
        return r ? std::set<KeyFrameT *>(r->connected.begin(), r->connected.end()) : std::set<KeyFrameT *>();
    }
    std::vector<KeyFrameT *> GetVectorCovisibleKeyFrames(KeyFrameT *pKF) const { const Row *r = find(pKF); return r ? r->ordered : std::vector<KeyFrameT *>(); }
    std::vector<KeyFrameT *> GetBestCovisibilityKeyFrames(KeyFrameT *pKF, const int &N) const
    {
        const Row *r = find(pKF);
        if (!r) return std::vector<KeyFrameT *>();
        return std::vector<KeyFrameT *>(r->ordered.begin(), r->ordered.begin() + std::min<size_t>(r->ordered.size(), (size_t)std::max(N, 0)));
    }
    // the lists are host vectors here, so this is the binary's own search (plf_covis_by_weight is the same rule over device rows): the prefix before the
    // first weight below w; when no weight is below w, the whole list (the fork's `&& back() < w` cannot hold there; upstream returns the empty list)
    std::vector<KeyFrameT *> GetCovisiblesByWeight(KeyFrameT *pKF, const int &w) const
    {
        const Row *r = find(pKF);
        if (!r || r->ordered.empty()) return std::vector<KeyFrameT *>();
        const auto it = std::upper_bound(r->orderedWeights.begin(), r->orderedWeights.end(), w, [](int a, int b) { return a > b; });
        if (it == r->orderedWeights.end() && r->orderedWeights.back() < w) return std::vector<KeyFrameT *>();
        return std::vector<KeyFrameT *>(r->ordered.begin(), r->ordered.begin() + (it - r->orderedWeights.begin()));
    }
    int GetWeight(KeyFrameT *pKF, KeyFrameT *pOther) const
    {
        const Row *r = find(pKF);
        if (r) for (size_t i = 0; i < r->connected.size(); i++) if (r->connected[i] == pOther) return r->connectedWeights[i];
        return 0;
    }
    KeyFrameT *Parent(KeyFrameT *pKF) const { const Row *r = find(pKF); return r && !r->ordered.empty() ? r->ordered.front() : nullptr; }   // what mbFirstConnection assigns
    const Row *find(KeyFrameT *pKF) const { const auto it = rows_.find(pKF); return it == rows_.end() ? nullptr : &it->second; }

    // the head of Tracking::UpdateLocalKeyFrames (so@0x4d5a0) for one frame: the votes of F.mvpMapPoints; an entry whose point isBad() is set to NULL, as there
    template <class FrameT> Votes LocalKeyFrameVotes(FrameT &F) const
    {
        Votes out;
        Gather g;
        for (auto &pMP : F.mvpMapPoints) if (pMP && pMP->isBad()) pMP = nullptr;
        g.row(F.mvpMapPoints);
        const int S = (int)g.kfs.size(), stride = std::max(S, 1);
        if (S == 0) return out;
        Device d(g, device_);
        std::vector<uint8_t> bad(S);
        for (int s = 0; s < S; s++) bad[s] = g.kfs[s]->isBad();
        plf::DeviceArray<uint8_t> dbad(bad, device_);
        plf::DeviceArray<int32_t> ck(stride, device_), cw(stride, device_), cn(1, device_), mk(1, device_), mw(1, device_);
        plf_covis_view v = d.view(1, S);
        v.kf_bad = dbad.get();
        const plf_covis_params p = {PLF_COVIS_VOTES, 1, stride, 0, 0};
        plf::check(plf_covis_count(&v, &p, ck.get(), cw.get(), cn.get(), nullptr, nullptr, nullptr, mk.get(), mw.get(), device_, nullptr), "Tracking::UpdateLocalKeyFrames");
        const std::vector<int32_t> hck = ck.download(), hcw = cw.download();
        const int n = cn.download()[0], kmax = mk.download()[0];
        for (int i = 0; i < n; i++) { out.vpLocalKeyFrames.push_back(g.kfs[hck[i]]); out.votes.push_back(hcw[i]); }
        if (kmax >= 0) { out.pKFmax = g.kfs[kmax]; out.max = mw.download()[0]; }
        return out;
    }

private:
    typedef detail::MapGather<KeyFrameT, MapPointT> Gather;
    struct Device : Gather::Device {
        int n_points;
        plf::DeviceArray<int64_t> key;                  // the keyframes' addresses (padded like the gathered arrays)
        Device(Gather &g, int device) : Gather::Device(g, device), n_points((int)g.pts.size()), key(keys(g.kfs), device) {}
        static std::vector<int64_t> keys(const std::vector<KeyFrameT *> &kfs)
        {
            std::vector<int64_t> k;
            for (KeyFrameT *pKF : kfs) k.push_back((int64_t)(intptr_t)pKF);
            return detail::padded(k, 0);
        }
        plf_covis_view view(int n_rows, int n_kf) const
        {
            return plf_covis_view{n_rows, this->row_start.get(), this->row_point.get(), nullptr, n_points, this->obs_start.get(), this->obs_kf.get(),
                                  this->point_bad.get(), n_kf, nullptr, key.get()};
        }
    };
    int device_, first_stride_;
    std::unordered_map<KeyFrameT *, Row> rows_;
};
// LocalMapping::KeyFrameCulling (so@0x643e0) over the reference's own KeyFrame / MapPoint classes: the candidates are
// mpCurrentKeyFrame->GetVectorCovisibleKeyFrames(), in that order.  Reads pKF->mnId, GetMapPointMatches(), mvKeysUn, mvDepth, mvuRight (the weight of an
// observation: 2 where mvuRight[idx] >= 0), mThDepth (the first candidate's: one camera), pMP->isBad() and GetObservations().  mbNotErase is protected in the
// reference, so the forwarder inside LocalMapping.cc / KeyFrame.cc passes it (vbNotErase, parallel to the candidates; empty = none).  The decisions equal
// the reference's one-by-one loop, the erasures between candidates included; the call resumes by itself when a list needs more than one call's erasures.
// NOTHING is applied to the objects: the caller runs pKF->SetBadFlag() on `erase` in order, which repeats on the host members exactly the erasures the device
// applied to its copy.  Uploads the rows of the candidates and the observations of their points once per call.  Map lines are not weighed.
template <class KeyFrameT> struct KeyFrameCullingResult {
    std::vector<int32_t> nMPs, nRedundantObservations, decision;   // per candidate: PLF decision 0 keep, 1 erase, 2 redundant but mbNotErase, 3 skipped (mnId == 0)
    std::vector<KeyFrameT *> erase;                                // the candidates with decision 1, in order
    int calls = 0;                                                 // device calls the list took
};
template <class KeyFrameT> KeyFrameCullingResult<KeyFrameT> KeyFrameCulling(const std::vector<KeyFrameT *> &vpLocalKeyFrames, bool mbMonocular,
                                                                           const std::vector<bool> &vbNotErase = std::vector<bool>(), int device = 0,
                                                                           int max_culls = 0)
{
    KeyFrameCullingResult<KeyFrameT> out;
    const int C = (int)vpLocalKeyFrames.size();
    out.nMPs.assign(C, -1); out.nRedundantObservations.assign(C, -1); out.decision.assign(C, 3);
    if (C == 0) return out;
    std::vector<int32_t> row_kf, row_level, obs_level, cand_row(C);
    std::vector<float> row_depth;
    std::vector<uint8_t> obs_w, cand_flags(C, 0);
    auto g = detail::map_gather<KeyFrameT, detail::MapPointOf<KeyFrameT>>(detail::Ignore(), detail::Ignore(), [&](KeyFrameT *pKFi, size_t idx) {
        obs_level.push_back(idx < pKFi->mvKeysUn.size() ? pKFi->mvKeysUn[idx].octave : 0);
        obs_w.push_back(idx < pKFi->mvuRight.size() && pKFi->mvuRight[idx] >= 0 ? 2 : 1);
    });
    float th_depth = 0.0f;
    for (int j = 0; j < C; j++) {
        KeyFrameT *pKF = vpLocalKeyFrames[j];
        cand_row[j] = j;
        cand_flags[j] = (uint8_t)((pKF->mnId == 0 ? 1 : 0) | (j < (int)vbNotErase.size() && vbNotErase[j] ? 2 : 0));
        if (j == 0) th_depth = pKF->mThDepth;
        row_kf.push_back(g.slot(pKF));                              // slots: the candidate before the observers its row brings
        const auto vpMapPoints = pKF->GetMapPointMatches();
        for (size_t i = 0; i < vpMapPoints.size(); i++) {           // per entry of the row, a null one included
            row_level.push_back(i < pKF->mvKeysUn.size() ? pKF->mvKeysUn[i].octave : 0);
            row_depth.push_back(i < pKF->mvDepth.size() ? pKF->mvDepth[i] : 0.0f);
        }
        g.row(vpMapPoints);
    }
    const int P = (int)g.pts.size(), S = (int)g.kfs.size();
    typename decltype(g)::Device d(g, device);
    std::vector<uint8_t> &point_bad = g.point_bad, gone(S + 1, 0);
    plf::DeviceArray<int32_t> d_row_kf(row_kf, device), d_row_level(detail::padded(row_level, 0), device), d_obs_level(detail::padded(obs_level, 0), device),
        d_cand(cand_row, device), d_mps(C, device), d_red(C, device), d_dec(C, device), d_status(2, device);
    plf::DeviceArray<float> d_row_depth(detail::padded(row_depth, 0.0f), device);
    plf::DeviceArray<uint8_t> &d_bad = d.point_bad;
    plf::DeviceArray<uint8_t> d_obs_w(detail::padded(obs_w, 1), device), d_flags(cand_flags, device), d_gone(gone, device), d_erased(gone, device),
        d_went(point_bad.size(), device);
    d_went.fill(0);
    plf_cull_view v = {};
    v.n_rows = C; v.row_start = d.row_start.get(); v.row_point = d.row_point.get(); v.row_kf = d_row_kf.get(); v.n_points = P; v.obs_start = d.obs_start.get();
    v.obs_kf = d.obs_kf.get(); v.obs_w = d_obs_w.get(); v.point_bad = d_bad.get(); v.n_kf = S; v.kf_gone = d_gone.get(); v.row_level = d_row_level.get();
    v.obs_level = d_obs_level.get(); v.row_depth = mbMonocular ? nullptr : d_row_depth.get(); v.th_depth = th_depth; v.monocular = mbMonocular ? 1 : 0;
    const plf_cull_params p = {PLF_CULL_SEQUENTIAL, 3, max_culls, 0, 0.9};
    for (int done = 0; done < C;) {
        plf::check(plf_keyframe_culling(&v, &p, d_cand.get() + done, d_flags.get() + done, C - done, d_mps.get() + done, d_red.get() + done, d_dec.get() + done,
                                        d_erased.get(), d_went.get(), nullptr, d_status.get(), device, nullptr), "LocalMapping::KeyFrameCulling");
        out.calls++;
        const int decided = d_status.download()[0];                 // a NULL-stream download waits for the device first
        if (decided <= 0) break;                                    // cannot happen: a call decides at least its first candidate
        done += decided;
        if (done < C) {                                             // more erasures than one call applies: go on from the applied state
            const std::vector<uint8_t> went = d_went.download(), erased = d_erased.download();
            for (int q = 0; q < P; q++) point_bad[q] = point_bad[q] || went[q] == 1;
            for (int s = 0; s < S; s++) gone[s] = erased[s] == 1;
            d_bad.upload(point_bad.data(), point_bad.size()); d_gone.upload(gone.data(), gone.size());
        }
    }
    out.nMPs = d_mps.download(); out.nRedundantObservations = d_red.download(); out.decision = d_dec.download();
    for (int j = 0; j < C; j++) if (out.decision[j] == 1) out.erase.push_back(vpLocalKeyFrames[j]);
    return out;
}
// Tracking::UpdateLocalMap -- UpdateLocalKeyFrames (so@0x4d5a0) and UpdateLocalPoints (so@0x49cc0) -- over the reference's own Frame / KeyFrame / MapPoint
// classes, for one frame: the votes, the expansion and the point list run on the device back to back (plf_covis_count, plf_local_keyframes,
// plf_local_items), one download at the end.  Reads mCurrentFrame.mvpMapPoints, pMP->isBad() / GetObservations(), pKF->isBad() / GetMapPointMatches() /
// GetBestCovisibilityKeyFrames(10) / GetChilds() / GetParent(); writes what the two functions leave: a bad own point set to NULL, mvpLocalKeyFrames,
// mvpLocalMapPoints, mpReferenceKF (when there is a pKFmax).  The marks (mnTrackReferenceForFrame) are not written: nothing reads them afterwards.
// The device work runs on `stream` (NULL: the null stream); the uploads before it and the download after it are synchronous.
// `seen` says which local points carry mnLastFrameSeen == the frame's id after the first loop of SearchLocalPoints.
// A frame without a single vote keeps mvpLocalKeyFrames, as the reference does, and only the points are listed again.
// EVERY CALL uploads what it reads, starting from host pointer members: every keyframe that observes an own point (the possible seeds) with its ten
// neighbours, children and parent, and the rows of all of these; a caller whose map is resident uses plf::LocalMap and uploads nothing.
template <class KeyFrameT, class MapPointT> struct LocalMapResult {
    std::vector<uint8_t> seen;            // parallel to mvpLocalMapPoints
    KeyFrameT *pKFmax = nullptr;
    int votes = 0;                        // of pKFmax
};
template <class KeyFrameT, class MapPointT, class FrameT>
LocalMapResult<KeyFrameT, MapPointT> UpdateLocalMap(FrameT &mCurrentFrame, std::vector<KeyFrameT *> &mvpLocalKeyFrames, std::vector<MapPointT *> &mvpLocalMapPoints,
                                                     KeyFrameT *&mpReferenceKF, int device = 0, void *stream = nullptr)
{
    LocalMapResult<KeyFrameT, MapPointT> out;
    detail::MapGather<KeyFrameT, MapPointT> g;
    std::vector<KeyFrameT *> &kfs = g.kfs;
    std::vector<int32_t> &obs_kf = g.obs_kf;
    auto slot_of = [&](KeyFrameT *pKF) { return g.slot(pKF); };
    // ---- the frame's own row and the observations of its points: the votes.  The row is set aside; the gatherer's rows are the keyframes' from here on.
    for (auto &pMP : mCurrentFrame.mvpMapPoints) if (pMP && pMP->isBad()) pMP = nullptr;
    g.row(mCurrentFrame.mvpMapPoints);
    std::vector<int32_t> frame_start{0}, frame_item;
    frame_start.swap(g.row_start); frame_item.swap(g.row_point);
    const int own_points = (int)g.pts.size(), S1 = (int)kfs.size();
    const bool voted = S1 > 0;
    // ---- the possible seeds with their neighbours, children and parent; without a vote the list that stays
    std::vector<int32_t> covis, n_covis, child_start{0}, child_kf, parent, keep;
    const int n_best = 10;
    for (int s = 0; s < S1; s++) {
        KeyFrameT *pKF = kfs[s];                                        // (kfs grows: no reference is held across slot_of)
        const std::vector<KeyFrameT *> vNeighs = pKF->GetBestCovisibilityKeyFrames(n_best);
        n_covis.push_back((int32_t)std::min<size_t>(vNeighs.size(), (size_t)n_best));
        for (int i = 0; i < n_best; i++) covis.push_back(i < (int)vNeighs.size() ? slot_of(vNeighs[i]) : -1);
        const std::set<KeyFrameT *> spChilds = pKF->GetChilds();
        for (KeyFrameT *pChild : spChilds) child_kf.push_back(slot_of(pChild));
        child_start.push_back((int32_t)child_kf.size());
        KeyFrameT *pParent = pKF->GetParent();
        parent.push_back(pParent ? slot_of(pParent) : -1);
    }
    if (!voted) for (KeyFrameT *pKF : mvpLocalKeyFrames) keep.push_back(slot_of(pKF));
    const int S = (int)kfs.size();
    if (S == 0) { mvpLocalMapPoints.clear(); return out; }
    covis.resize((size_t)S * n_best, -1); n_covis.resize(S, 0); child_start.resize(S + 1, (int32_t)child_kf.size()); parent.resize(S, -1);
    // ---- slots in ADDRESS order from here on: the slot is then the key of the reference's std::map<KeyFrame*, int>, and the votes need no kf_key
    std::vector<int> order(S);
    for (int s = 0; s < S; s++) order[s] = s;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return (uintptr_t)kfs[x] < (uintptr_t)kfs[y]; });
    std::vector<int32_t> to(S);
    for (int i = 0; i < S; i++) to[order[i]] = i;
    auto moved = [&](int32_t s) { return s < 0 ? -1 : to[s]; };
    {
        std::vector<KeyFrameT *> kfs2(S);
        std::vector<int32_t> covis2((size_t)S * n_best), n_covis2(S), parent2(S), child_start2{0}, child_kf2;
        for (int i = 0; i < S; i++) {
            const int o = order[i];
            kfs2[i] = kfs[o]; n_covis2[i] = n_covis[o]; parent2[i] = moved(parent[o]);
            for (int j = 0; j < n_best; j++) covis2[(size_t)i * n_best + j] = moved(covis[(size_t)o * n_best + j]);
            for (int32_t c = child_start[o]; c < child_start[o + 1]; c++) child_kf2.push_back(moved(child_kf[c]));
            child_start2.push_back((int32_t)child_kf2.size());
        }
        kfs.swap(kfs2); covis.swap(covis2); n_covis.swap(n_covis2); parent.swap(parent2); child_start.swap(child_start2); child_kf.swap(child_kf2);
        for (int32_t &k : obs_kf) k = moved(k);
        for (int32_t &k : keep) k = moved(k);
    }
    // ---- the rows of every keyframe that can end up in the list; a point first met here gets an id and a bad flag, no observations: it cannot vote
    // (the slots were renumbered above, so slot() is not called any more)
    std::vector<uint8_t> kf_bad(S);
    for (int s = 0; s < S; s++) {
        kf_bad[s] = kfs[s]->isBad();
        g.row(kfs[s]->GetMapPointMatches(), false);
    }
    const std::vector<MapPointT *> &pts = g.pts;
    const int P = (int)pts.size(), kf_stride = std::max(S, (int)keep.size()), item_stride = std::max(P, 1);
    const typename decltype(g)::Device d(g, device);
    plf::DeviceArray<int32_t> d_fs(frame_start, device), d_fi(detail::padded(frame_item, -1), device), d_cov(covis, device), d_ncov(n_covis, device),
        d_cs(child_start, device), d_ck(detail::padded(child_kf, -1), device), d_par(parent, device), d_seed(std::max(S1, 1), device),
        d_w(std::max(S1, 1), device), d_nseed(1, device), d_mk(1, device), d_mw(1, device);
    plf::DeviceArray<uint8_t> d_kbad(kf_bad, device);
    plf::LocalMap lm(1, kf_stride, item_stride, device);
    const plf::LocalMap::Rows rows = {d.row_start.get(), d.row_point.get(), d.point_bad.get(), P};
    if (voted) {
        const plf_covis_view v = {1, d_fs.get(), d_fi.get(), nullptr, own_points, d.obs_start.get(), d.obs_kf.get(), d.point_bad.get(), S, d_kbad.get(), nullptr};
        const plf_covis_params p = {PLF_COVIS_VOTES, 1, std::max(S1, 1), 0, 0};
        plf::check(plf_covis_count(&v, &p, d_seed.get(), d_w.get(), d_nseed.get(), nullptr, nullptr, nullptr, d_mk.get(), d_mw.get(), device, stream),
                   "Tracking::UpdateLocalKeyFrames");
        const plf::LocalMap::Graph graph = {d_cov.get(), d_ncov.get(), n_best, d_cs.get(), d_ck.get(), d_par.get(), d_kbad.get(), S};
        lm.Update(d_seed.get(), d_nseed.get(), std::max(S1, 1), graph, rows, d_fs.get(), d_fi.get(), stream, n_best, 80);
    } else {
        keep.resize(kf_stride, -1);
        const std::vector<int32_t> n_keep(1, (int32_t)mvpLocalKeyFrames.size());
        lm.local_kf.upload(keep.data(), keep.size()); lm.n_local_kf.upload(n_keep.data(), 1);
        lm.Items(S, rows, d_fs.get(), d_fi.get(), stream);
    }
    // ---- one download: the lists by pointer
    const std::vector<int32_t> h_item = lm.local_item.download(), h_n = lm.n_local_item.download();   // a NULL-stream download waits for the device first
    const std::vector<uint8_t> h_seen = lm.seen.download();
    if (voted) {
        const std::vector<int32_t> h_kf = lm.local_kf.download(), h_nkf = lm.n_local_kf.download();
        mvpLocalKeyFrames.clear();
        for (int i = 0; i < h_nkf[0]; i++) mvpLocalKeyFrames.push_back(kfs[h_kf[i]]);
        const int kmax = d_mk.download()[0];
        if (kmax >= 0) { out.pKFmax = kfs[kmax]; out.votes = d_mw.download()[0]; mpReferenceKF = out.pKFmax; }
    }
    mvpLocalMapPoints.clear();
    for (int i = 0; i < h_n[0]; i++) { mvpLocalMapPoints.push_back(pts[h_item[i]]); out.seen.push_back(h_seen[i]); }
    return out;
}
// Optimizer::PoseOptimization(Frame*) (so@0xaef50), the reference's signature over its own Frame / MapPoint: the matched key points of ONE frame go to the
// device as a plf_pose_view, plf_pose_optimize refines mTcw, and the frame gets what the reference's body leaves in it -- mvbOutlier of every matched key
// point, SetPose(the refined Tcw) -- and the call returns nInitialCorrespondences - nBad.  Points only, as the binary (the header's
// PoseOptimizationWithLine has no body anywhere).  With fewer than 3 matches: returns 0, frame untouched.  For ONE frame the adapter uploads and waits; a
// tracker with its frames resident calls plf_pose_optimize on all of them at once and reads nothing back.  fx, fy, cx, cy are static members of Frame in
// the reference, mbf an ordinary one: read as pFrame->fx etc.
struct Optimizer {
    template <class FrameT> static int PoseOptimization(FrameT *pFrame, int device = 0)
    {
        const int N = pFrame->N;
        if (N <= 0) return 0;
        std::vector<plf_keypoint> keys(N);
        std::vector<float> uright(N, -1.0f), pos;
        std::vector<int32_t> match(N, -1);
        std::vector<uint8_t> flags(N, 0);
        int nInitialCorrespondences = 0;
        for (int i = 0; i < N; i++) {
            const cv::KeyPoint &kp = pFrame->mvKeysUn[i];
            keys[i] = plf_keypoint{kp.pt.x, kp.pt.y, kp.size, kp.angle, kp.response, kp.octave, kp.class_id};
            uright[i] = pFrame->mvuRight[i];
            flags[i] = pFrame->mvbOutlier[i] ? 1 : 0;
            auto *pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            match[i] = nInitialCorrespondences++;
            detail::put3(pos, pMP->GetWorldPos());
        }
        if (nInitialCorrespondences < 3) return 0;
        const plf_pose34 pin = detail::pose34(pFrame->mTcw);
        const std::vector<float> sigma2(pFrame->mvInvLevelSigma2.begin(), pFrame->mvInvLevelSigma2.end());
        plf::DeviceArray<plf_keypoint> dkeys(keys, device);
        plf::DeviceArray<float> dur(uright, device), dpos(pos, device), dsig(sigma2, device);
        plf::DeviceArray<int32_t> dmatch(match, device), dn(1, device), dst(1, device);
        plf::DeviceArray<uint8_t> dflags(flags, device);
        plf::DeviceArray<plf_pose34> dout(1, device);
        plf_pose_view v = {};
        v.n_frames = 1; v.kp_stride = N; v.pos_stride = 0; v.keys_un = dkeys.get(); v.uright = dur.get(); v.n_host = N; v.match_of_kp = dmatch.get();
        v.world_pos = dpos.get(); v.inv_level_sigma2 = dsig.get(); v.nlevels = (int32_t)sigma2.size();
        plf_camera cam = {};
        cam.fx = pFrame->fx; cam.fy = pFrame->fy; cam.cx = pFrame->cx; cam.cy = pFrame->cy; cam.bf = pFrame->mbf;
        plf::check(plf_pose_optimize(&v, &cam, &pin, PLF_MEM_HOST, dout.get(), nullptr, dflags.get(), dn.get(), dst.get(), device, nullptr), "PoseOptimization");
        const plf_pose34 pout = dout.download()[0];           // a NULL-stream download waits for the device first
        flags = dflags.download();
        for (int i = 0; i < N; i++)
            if (match[i] >= 0) pFrame->mvbOutlier[i] = flags[i] != 0;
        pFrame->SetPose(detail::mat44(pout));
        return dn.download()[0];
    }

    // Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (so@0xb60c0), the reference's signature over its own KeyFrame / MapPoint and
    // g2o::Sim3: the two keyframes, the points either sees and the matches go to the device as a plf_sim3_view of two slots, plf_sim3_optimize refines the
    // transform, and the caller gets what the reference's body leaves: the culled matches NULL in vpMatches1, g2oS12 = the estimate (untouched when the
    // call returns 0 at its `< 10` test), the return value nIn.  plf_sim3_optimize takes the start as the floats ComputeSim3 has (R, t, s): g2oS12 is
    // narrowed to them -- rotation().toRotationMatrix() (Eigen's 2x form), translation() and scale() rounded to float -- and widened again on the device,
    // which for a g2oS12 built from floats as ComputeSim3 builds it differs from it by the rounding of that round trip only.  The camera and
    // mvInvLevelSigma2 are taken from pKF1 for both keyframes (the reference reads pKF2->mK and pKF2->mvInvLevelSigma2 for the second edge): the same values
    // for one sensor.  A match whose GetIndexInKeyFrame(pKF2) is no key point of pKF2 is skipped, as in the reference, and stays as it is.  For ONE
    // candidate the adapter uploads and waits; a loop closer with its keyframes resident calls plf_sim3_optimize on all candidates at once.
    template <class KeyFrameT, class MapPointT, class Sim3T>
    static int OptimizeSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches1, Sim3T &g2oS12, const float th2, const bool bFixScale, int device = 0)
    {
        const std::vector<MapPointT *> vpMapPoints1 = pKF1->GetMapPointMatches();
        KeyFrameT *kf[2] = {pKF1, pKF2};
        const int n1 = (int)pKF1->mvKeysUn.size(), n2 = (int)pKF2->mvKeysUn.size(), N = (int)vpMatches1.size();
        const int S = std::max(n1, 1);
        std::vector<plf_keypoint> keys[2];
        std::vector<int32_t> mps[2], match(S, -1), slots = {n1, n2};
        plf_frustum_pose pose[2];
        std::vector<float> world;
        std::vector<uint8_t> bad;
        std::unordered_map<MapPointT *, int32_t> ids;
        auto id_of = [&](MapPointT *p) {
            auto it = ids.find(p);
            if (it != ids.end()) return it->second;
            const int32_t id = (int32_t)ids.size();
            ids.emplace(p, id);
            detail::put3(world, p->GetWorldPos());
            bad.push_back(p->isBad() ? 1 : 0);
            return id;
        };
        for (int s = 0; s < 2; s++) {
            const int n = slots[s];
            keys[s].resize(std::max(n, 1));
            if (n) std::memcpy((void *)keys[s].data(), kf[s]->mvKeysUn.data(), (size_t)n * sizeof(plf_keypoint));
            mps[s].assign(std::max(n, 1), -1);
            pose[s] = detail::frustum_pose(kf[s]->GetRotation(), kf[s]->GetTranslation());
        }
        for (int i = 0; i < N && i < n1; i++) {
            MapPointT *pMP2 = vpMatches1[i];
            if (!pMP2) continue;
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
            MapPointT *pMP1 = i < (int)vpMapPoints1.size() ? vpMapPoints1[i] : nullptr;
            if (!pMP1 || i2 < 0 || i2 >= n2) continue;
            mps[0][i] = id_of(pMP1);
            mps[1][i2] = id_of(pMP2);
            match[i] = i2;
        }
        if (world.empty()) { world.assign(3, 0.0f); bad.assign(1, 1); }
        // the start, narrowed to the floats of the C ABI
        const double qx = g2oS12.rotation().x(), qy = g2oS12.rotation().y(), qz = g2oS12.rotation().z(), qw = g2oS12.rotation().w();
        const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
        const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
        const std::vector<float> sim3_in = {(float)(1.0 - (tyy + tzz)), (float)(txy - twz), (float)(txz + twy), (float)(txy + twz), (float)(1.0 - (txx + tzz)),
                                            (float)(tyz - twx), (float)(txz - twy), (float)(tyz + twx), (float)(1.0 - (txx + tyy)), (float)g2oS12.translation()[0],
                                            (float)g2oS12.translation()[1], (float)g2oS12.translation()[2], (float)g2oS12.scale()};
        const std::vector<float> inv_sigma2(pKF1->mvInvLevelSigma2.begin(), pKF1->mvInvLevelSigma2.end());
        plf::DeviceArray<plf_keypoint> dk0(keys[0], device), dk1(keys[1], device);
        plf::DeviceArray<int32_t> dm0(mps[0], device), dm1(mps[1], device), dn(slots, device), dmatch(match, device), dkf1(std::vector<int32_t>(1, 0), device),
            dkf2(std::vector<int32_t>(1, 1), device), dnin(1, device), dst(1, device);
        const std::vector<const plf_keypoint *> t_keys = {dk0.get(), dk1.get()};
        const std::vector<const int32_t *> t_mps = {dm0.get(), dm1.get()};
        plf::DeviceArray<const plf_keypoint *> dt_keys(t_keys, device);
        plf::DeviceArray<const int32_t *> dt_mps(t_mps, device);
        plf::DeviceArray<plf_frustum_pose> dpose(std::vector<plf_frustum_pose>(pose, pose + 2), device);
        plf::DeviceArray<float> dworld(world, device), dsig(inv_sigma2, device), din(sim3_in, device);
        plf::DeviceArray<uint8_t> dbad(bad, device), dfix(std::vector<uint8_t>(1, bFixScale ? 1 : 0), device);
        plf::DeviceArray<double> dout(8, device);
        plf_sim3_view v = {};
        v.n_kf = 2; v.kf_keys = dt_keys.get(); v.kf_n = dn.get(); v.kf_pose = dpose.get(); v.kf_mappoints = dt_mps.get(); v.kf_obs_index = nullptr;
        v.world_pos = dworld.get(); v.point_bad = dbad.get(); v.n_points = (int32_t)bad.size(); v.level_sigma2 = nullptr; v.nlevels = (int32_t)inv_sigma2.size();
        plf_camera cam = {};
        cam.fx = pKF1->fx; cam.fy = pKF1->fy; cam.cx = pKF1->cx; cam.cy = pKF1->cy;
        const plf_sim3opt_jobs jobs = {1, S, dkf1.get(), dkf2.get(), din.get(), dfix.get(), dsig.get(), th2};
        plf::check(plf_sim3_optimize(&v, &cam, &jobs, dmatch.get(), dout.get(), nullptr, dnin.get(), dst.get(), device, nullptr), "OptimizeSim3");
        const std::vector<int32_t> after = dmatch.download();          // a NULL-stream download waits for the device first
        for (int i = 0; i < N && i < n1; i++)
            if (match[i] >= 0 && after[i] < 0) vpMatches1[i] = static_cast<MapPointT *>(nullptr);
        const int status = dst.download()[0];
        if (!(status & PLF_SIM3OPT_FEW)) {
            const std::vector<double> o = dout.download();
            g2oS12.rotation().x() = o[0]; g2oS12.rotation().y() = o[1]; g2oS12.rotation().z() = o[2]; g2oS12.rotation().w() = o[3];
            g2oS12.translation()[0] = o[4]; g2oS12.translation()[1] = o[5]; g2oS12.translation()[2] = o[6];
            g2oS12.scale() = o[7];
        }
        return dnin.download()[0];
    }
};

// Tracking::NeedNewKeyFrame (so@0x49750) and the point loops of Tracking::CreateNewKeyFrame (so@0x4e040) / Tracking::UpdateLastFrame (so@0x4e570) over the
// reference's own Tracking / Frame / KeyFrame / MapPoint.  Single-frame: each uploads, waits and writes back; a tracker with its frames resident calls the
// plf_track_* entry points on all of them at once and reads nothing back.  The MapPoints are made on the host, by the caller's `make(x3D, i)`, in the
// device's order (the order of the reference's walk), so that ids (MapPoint::nNextId) come out as the reference's.
struct Tracking {
    template <class TrackingT> static bool NeedNewKeyFrame(TrackingT *t, int device = 0)
    {
        auto &F = t->mCurrentFrame;
        const int N = std::max(F.N, 1);
        std::vector<float> depth(N, 0.0f);
        std::vector<int32_t> match(N, -1), n_obs, row_start(2, 0), row_item;
        std::vector<uint8_t> bad;
        std::unordered_map<const void *, int32_t> ids;
        auto id_of = [&](auto *pMP) {
            auto it = ids.find(pMP);
            if (it != ids.end()) return it->second;
            const int32_t id = (int32_t)n_obs.size();
            ids.emplace(pMP, id);
            n_obs.push_back(pMP->Observations());
            bad.push_back(pMP->isBad() ? 1 : 0);
            return id;
        };
        for (int i = 0; i < F.N; i++) {
            depth[i] = F.mvDepth[i];
            if (F.mvpMapPoints[i]) match[i] = id_of(F.mvpMapPoints[i]);
        }
        if (t->mpReferenceKF)
            for (auto *pMP : t->mpReferenceKF->GetMapPointMatches()) row_item.push_back(pMP ? id_of(pMP) : -1);
        row_start[1] = (int32_t)row_item.size();
        if (row_item.empty()) row_item.push_back(-1);
        if (n_obs.empty()) { n_obs.push_back(0); bad.push_back(0); }
        plf_track_kf_state s = {};
        s.frame_id = (int64_t)F.mnId; s.ref_kf = t->mpReferenceKF ? 0 : -1; s.n_matches_inliers = t->mnMatchesInliers;
        s.last_kf_id = (uint32_t)t->mnLastKeyFrameId; s.last_reloc_frame_id = (uint32_t)t->mnLastRelocFrameId;
        s.min_frames = t->mMinFrames; s.max_frames = t->mMaxFrames; s.n_kfs = (int32_t)t->mpMap->KeyFramesInMap();
        const bool stopped = t->mpLocalMapper->isStopped() || t->mpLocalMapper->stopRequested();
        const bool idle = t->mpLocalMapper->AcceptKeyFrames();
        s.flags = (t->mbOnlyTracking ? PLF_TRACK_ONLY_TRACKING : 0) | (stopped ? PLF_TRACK_MAPPER_STOPPED : 0) | (idle ? PLF_TRACK_MAPPER_IDLE : 0) |
                  (t->mSensor == 0 ? PLF_TRACK_MONO : 0);
        plf::DeviceArray<float> ddepth(depth, device);
        plf::DeviceArray<int32_t> dmatch(match, device), dobs(n_obs, device), dstart(row_start, device), ditem(row_item, device), dcounts(3, device), ddec(1, device);
        plf::DeviceArray<uint8_t> dbad(bad, device);
        plf::DeviceArray<plf_track_kf_state> dstate(std::vector<plf_track_kf_state>(1, s), device);
        plf_track_view v = {};
        v.n_frames = 1; v.kp_stride = N; v.depth = ddepth.get(); v.match_of_kp = dmatch.get(); v.n_host = F.N > 0 ? F.N : 0; v.n_obs = dobs.get();
        v.n_points = (int32_t)n_obs.size();
        const plf_track_kf_view kf = {dstart.get(), ditem.get(), 1, dbad.get()};
        plf::Tracking::NeedNewKeyFrame(v, kf, dstate.get(), nullptr, t->mThDepth, dcounts.get(), ddec.get(), device);
        const int decision = ddec.download()[0];                 // a NULL-stream download waits for the device first
        if (decision != 2) return decision == 1;
        t->mpLocalMapper->InterruptBA();                         // thread state: the host's (so@0x49a50-0x49aa5)
        return t->mSensor != 0 && t->mpLocalMapper->KeyframesInQueue() < 3;
    }

    // the loop of CreateNewKeyFrame after UpdatePoseMatrices: F.mvpMapPoints[i] = make(x3D, i) for the created key points, in order; returns their number
    template <class FrameT, class Make> static int CreateNewKeyFrame(FrameT &F, float mThDepth, Make make, int device = 0, int min_points = 100)
    {
        return ClosePoints(F, mThDepth, make, device, min_points);
    }
    // the loop of UpdateLastFrame over mLastFrame (the guard and SetPose(Tlr * pRef->GetPose()) are the caller's; make() also keeps mlpTemporalPoints)
    template <class FrameT, class Make> static int UpdateLastFrame(FrameT &F, float mThDepth, Make make, int device = 0, int min_points = 100)
    {
        return ClosePoints(F, mThDepth, make, device, min_points);
    }

private:
    template <class FrameT, class Make> static int ClosePoints(FrameT &F, float mThDepth, Make make, int device, int min_points)
    {
        const int N = F.N;
        if (N <= 0) return 0;
        if (N > 16384) throw std::invalid_argument("Tracking: more than 16384 key points");
        std::vector<plf_keypoint> keys(N);
        std::vector<float> depth(N);
        std::vector<int32_t> match(N, -1), n_obs(N, 0);
        for (int i = 0; i < N; i++) {
            const cv::KeyPoint &kp = F.mvKeysUn[i];
            keys[i] = plf_keypoint{kp.pt.x, kp.pt.y, kp.size, kp.angle, kp.response, kp.octave, kp.class_id};
            depth[i] = F.mvDepth[i];
            if (F.mvpMapPoints[i]) { match[i] = i; n_obs[i] = F.mvpMapPoints[i]->Observations(); }
        }
        const cv::Mat Rwc = F.GetRotationInverse();
        cv::Mat Rcw(3, 3, CV_32F);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rcw.template at<float>(r, c) = Rwc.template at<float>(c, r);
        const plf_frustum_pose fp = detail::frustum_pose(Rcw, cv::Mat(), F.GetCameraCenter());   // tcw is not read
        plf_camera cam = {};
        cam.fx = F.fx; cam.fy = F.fy; cam.cx = F.cx; cam.cy = F.cy; cam.bf = F.mbf;
        plf::DeviceArray<plf_keypoint> dkeys(keys, device);
        plf::DeviceArray<float> ddepth(depth, device), dpos((size_t)N * 3, device);
        plf::DeviceArray<int32_t> dmatch(match, device), dobs(n_obs, device), dkp(N, device), dn(3, device);
        plf::DeviceArray<plf_frustum_pose> dfp(std::vector<plf_frustum_pose>(1, fp), device);
        plf_track_view v = {};
        v.n_frames = 1; v.kp_stride = N; v.keys_un = dkeys.get(); v.depth = ddepth.get(); v.match_of_kp = dmatch.get(); v.n_host = N; v.n_obs = dobs.get();
        v.n_points = N; v.pose = dfp.get();
        plf::Tracking::CreateNewKeyFrame(v, cam, mThDepth, nullptr, N, dkp.get(), dpos.get(), dn.get(), dn.get() + 1, dn.get() + 2, device, nullptr, min_points);
        const int n_new = dn.download()[0];                      // a NULL-stream download waits for the device first
        const std::vector<int32_t> kp = dkp.download();
        const std::vector<float> pos = dpos.download();
        for (int k = 0; k < n_new; k++) {
            F.mvpMapPoints[kp[k]] = make(detail::mat31(&pos[3 * (size_t)k]), kp[k]);
        }
        return n_new;
    }
};

// void LocalMapping::CreateNewMapPoints() (so@0x5ce60) over the reference's own KeyFrame / MapPoint, in the reference's order: GetBestCovisibilityKeyFrames(nn),
// and per neighbour the caller's ComputeF12, plf_match_triangulation and plf_triangulate_points (which holds the baseline test) with the has_mp marks on, so that
// neighbour r + 1 is searched over what neighbour r's pairs created; then, on the host and in the order of the reference's `new MapPoint` calls (neighbour by
// neighbour, ascending idx1), make(x3D, pKF1, pKF2, idx1, idx2), which does new MapPoint / AddObservation x2 / AddMapPoint x2 / ComputeDistinctiveDescriptors /
// UpdateNormalAndDepth / mpMap->AddMapPoint / mlpRecentAddedMapPoints.push_back and so hands out MapPoint::nNextId as the reference would.  No ids cross the
// device: they are given after the last neighbour.  computeF12(pKF1, pKF2) returns the 3x3 CV_32F matrix.  Single-keyframe form: it uploads the keyframes, and
// waits after each call because the matcher handle enqueues on a stream of its own; a mapper with its keyframes resident passes one stream to both calls and
// waits once.  The monocular CheckNewKeyFrames() exit and ComputeSceneMedianDepth test are thread state and out of scope: RGB-D and stereo only.
struct LocalMapping {
    template <class KeyFrameT, class ComputeF12, class Make>
    static int CreateNewMapPoints(KeyFrameT *mpCurrentKeyFrame, ComputeF12 computeF12, Make make, int device = 0, int nn = 10)
    {
        const std::vector<KeyFrameT *> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
        if (vpNeighKFs.empty()) return 0;
        std::vector<KeyFrameT *> kfs(1, mpCurrentKeyFrame);
        kfs.insert(kfs.end(), vpNeighKFs.begin(), vpNeighKFs.end());
        const int K = (int)kfs.size(), J = K - 1;
        struct Dev {
            plf::DeviceArray<plf_keypoint> keys;
            plf::DeviceArray<float> uright, depth;
            plf::DeviceArray<uint8_t> desc, has_mp;
            plf::DeviceArray<uint32_t> node_id;
            plf::DeviceArray<int32_t> node_start, feat;
            int n = 0, nodes = 0;
        };
        std::vector<Dev> d(K);
        std::vector<plf_frustum_pose> poses(K);
        std::vector<const plf_keypoint *> t_keys(K);
        std::vector<const float *> t_ur(K), t_depth(K);
        std::vector<uint8_t *> t_has(K);
        std::vector<int32_t> t_n(K);
        int max_n = 1;
        for (int s = 0; s < K; s++) {
            KeyFrameT *kf = kfs[s];
            const int N = kf->N;
            const size_t cap = (size_t)std::max(N, 1);
            std::vector<plf_keypoint> keys(cap);
            std::vector<float> ur(cap, -1.0f), dep(cap, -1.0f);
            std::vector<uint8_t> desc(cap * 32, 0), has(cap, 0);
            for (int i = 0; i < N; i++) {
                const cv::KeyPoint &kp = kf->mvKeysUn[i];
                keys[i] = plf_keypoint{kp.pt.x, kp.pt.y, kp.size, kp.angle, kp.response, kp.octave, kp.class_id};
                ur[i] = kf->mvuRight[i];
                dep[i] = kf->mvDepth[i];
                has[i] = kf->GetMapPoint(i) ? 1 : 0;
                std::memcpy(&desc[(size_t)i * 32], kf->mDescriptors.data + (size_t)i * kf->mDescriptors.step, 32);
            }
            std::vector<uint32_t> node_id;
            std::vector<int32_t> node_start(1, 0), feat;
            for (const auto &node : kf->mFeatVec) {
                node_id.push_back((uint32_t)node.first);
                for (unsigned int f : node.second) feat.push_back((int32_t)f);
                node_start.push_back((int32_t)feat.size());
            }
            d[s].n = N; d[s].nodes = (int)node_id.size();
            if (node_id.empty()) node_id.push_back(0);
            if (feat.empty()) feat.push_back(0);
            d[s].keys.assign(keys, device); d[s].uright.assign(ur, device); d[s].depth.assign(dep, device); d[s].desc.assign(desc, device);
            d[s].has_mp.assign(has, device); d[s].node_id.assign(node_id, device); d[s].node_start.assign(node_start, device); d[s].feat.assign(feat, device);
            poses[s] = detail::frustum_pose(kf->GetRotation(), kf->GetTranslation(), kf->GetCameraCenter());
            t_keys[s] = d[s].keys.get(); t_ur[s] = d[s].uright.get(); t_depth[s] = d[s].depth.get(); t_has[s] = d[s].has_mp.get(); t_n[s] = N;
            max_n = std::max(max_n, N);
        }
        KeyFrameT *cur = mpCurrentKeyFrame;
        const int N1 = std::max(cur->N, 1);
        const std::vector<float> sf(cur->mvScaleFactors.begin(), cur->mvScaleFactors.end()), sg(cur->mvLevelSigma2.begin(), cur->mvLevelSigma2.end());
        plf::DeviceArray<float> d_sf(sf, device), d_sg(sg, device);
        plf::DeviceArray<const plf_keypoint *> d_keys(t_keys, device);
        plf::DeviceArray<const float *> d_ur(t_ur, device), d_depth(t_depth, device);
        plf::DeviceArray<uint8_t *> d_has(t_has, device);
        plf::DeviceArray<int32_t> d_n(t_n, device), d_match((size_t)J * N1, device), d_cnt(1, device), d_i1((size_t)J * N1, device), d_i2((size_t)J * N1, device),
            d_nnew(J, device), d_status(J, device);
        plf::DeviceArray<plf_frustum_pose> d_pose(poses, device);
        plf::DeviceArray<float> d_pos((size_t)J * N1 * 3, device);
        plf::DeviceArray<uint8_t> d_reason((size_t)J * N1, device);
        std::vector<int32_t> kf1(J, 0), kf2(J);
        for (int j = 0; j < J; j++) kf2[j] = j + 1;
        plf::DeviceArray<int32_t> d_kf1(kf1, device), d_kf2(kf2, device);
        plf_matcher *m = nullptr;
        plf::check(plf_matcher_create(device, max_n, 1024, 64, 1, &m), "plf_matcher_create");
        struct Free { plf_matcher *m; ~Free() { plf_matcher_destroy(m); } } free_m{m};
        plf_triangulate_view tv = {};
        tv.n_kf = K; tv.kf_keys = d_keys.get(); tv.kf_uright = d_ur.get(); tv.kf_depth = d_depth.get(); tv.kf_n = d_n.get(); tv.kf_pose = d_pose.get();
        tv.scale_factors = d_sf.get(); tv.level_sigma2 = d_sg.get(); tv.nlevels = (int32_t)sf.size(); tv.scale_factor = cur->mfScaleFactor;
        tv.mb = cur->mb; tv.mbf = cur->mbf;
        plf_camera cam = {};
        cam.fx = cur->fx; cam.fy = cur->fy; cam.cx = cur->cx; cam.cy = cur->cy; cam.bf = cur->mbf;
        plf_triangulate_marks marks = {d_has.get(), nullptr, nullptr};
        float Cw1[3];
        detail::put3(Cw1, cur->GetCameraCenter());
        for (int j = 0; j < J; j++) {
            KeyFrameT *pKF2 = kfs[j + 1];
            const cv::Mat F12 = computeF12(cur, pKF2);
            float F[9];
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) F[3 * r + c] = F12.template at<float>(r, c);
            plf_tri_view v = {};
            v.n1 = d[0].n; v.n2 = d[j + 1].n;
            v.keys1 = d[0].keys.get(); v.keys2 = d[j + 1].keys.get(); v.uright1 = d[0].uright.get(); v.uright2 = d[j + 1].uright.get();
            v.desc1 = d[0].desc.get(); v.desc2 = d[j + 1].desc.get(); v.has_mp1 = d[0].has_mp.get(); v.has_mp2 = d[j + 1].has_mp.get();
            v.nodes1 = d[0].nodes; v.nodes2 = d[j + 1].nodes; v.node_id1 = d[0].node_id.get(); v.node_id2 = d[j + 1].node_id.get();
            v.node_start1 = d[0].node_start.get(); v.node_start2 = d[j + 1].node_start.get(); v.feat1 = d[0].feat.get(); v.feat2 = d[j + 1].feat.get();
            v.scale_factors2 = d_sf.get(); v.level_sigma2_2 = d_sg.get();
            plf_kf_pose p2 = {};
            std::memcpy(p2.Rcw, poses[j + 1].Rcw, sizeof(p2.Rcw)); std::memcpy(p2.tcw, poses[j + 1].tcw, sizeof(p2.tcw)); std::memcpy(p2.Ow, poses[j + 1].Ow, sizeof(p2.Ow));
            p2.fx = pKF2->fx; p2.fy = pKF2->fy; p2.cx = pKF2->cx; p2.cy = pKF2->cy; p2.bf = pKF2->mbf; p2.log_scale_factor = pKF2->mfLogScaleFactor;
            p2.inv_level_sigma2 = pKF2->mvInvLevelSigma2.data();
            // ORBmatcher matcher(0.6, false); matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, false)
            plf::check(plf_match_triangulation(m, &v, F, Cw1, &p2, 0, 0, d_match.get() + (size_t)j * N1, d_cnt.get(), nullptr), "SearchForTriangulation");
            (void)d_cnt.download();                                  // waits: the handle's stream is its own
            plf_triangulate_jobs jobs = {1, N1, N1, d_kf1.get() + j, d_kf2.get() + j, d_match.get() + (size_t)j * N1};
            plf::Triangulator::CreateNewMapPoints(tv, cam, jobs, &marks, d_i1.get() + (size_t)j * N1, d_i2.get() + (size_t)j * N1, d_pos.get() + (size_t)j * N1 * 3,
                                                  d_nnew.get() + j, d_status.get() + j, d_reason.get() + (size_t)j * N1, device, nullptr);
            (void)d_cnt.download();                                  // waits: the next search reads the marks
        }
        const std::vector<int32_t> n_new = d_nnew.download(), i1 = d_i1.download(), i2 = d_i2.download();
        const std::vector<float> pos = d_pos.download();
        int nnew = 0;
        for (int j = 0; j < J; j++)
            for (int k = 0; k < n_new[j]; k++) {
                const size_t o = (size_t)j * N1 + k;
                make(detail::mat31(&pos[o * 3]), cur, kfs[j + 1], i1[o], i2[o]);
                nnew++;
            }
        return nnew;
    }
};

// class Sim3Solver include/Sim3Solver.h with its reference signatures, over the reference's own KeyFrame / MapPoint classes (the members the reference's
// constructor reads: GetMapPointMatches, GetRotation, GetTranslation, mvKeysUn, mvLevelSigma2, fx .. cy; isBad, GetIndexInKeyFrame, GetWorldPos).
// The constructor flattens what the reference's reads and, like the reference's (so@0x110a06), sets the default parameters; it draws NOTHING from rand().
// SetRansacParameters draws the solver's 3 * maxIterations raw values from rand() -- for one solver driven by find() exactly the values the reference
// would consume up to the returning iteration; a solver left at the constructor's defaults draws at its first iterate() / Prepare().  iterate() is one
// plf_sim3_iterate.  Prepare() + Step() step a vector of solvers with ONE device call per round: the loop of LoopClosing::ComputeSim3.  The camera and
// mvLevelSigma2 are taken from pKF1 for both keyframes (the reference projects into keyframe 2 with pKF2's mK and reads pKF2->mvLevelSigma2): the same
// values for one sensor, which is all plf_sim3_view holds.  The reference
// interleaves one global rand() stream across its solvers and an early return shifts every later draw; a call that runs solvers side by side cannot
// reproduce that and does not claim it: given the same triples the result is the reference's, which triples a solver gets is the caller's.
template <class KeyFrameT, class MapPointT> class Sim3Solver {
public:
    Sim3Solver(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatched12, const bool bFixScale = true, int device = 0)
        : mbFixScale(bFixScale), device_(device)
    {
        const std::vector<MapPointT *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        std::unordered_map<MapPointT *, int32_t> ids;
        auto id_of = [&](MapPointT *p) {
            auto it = ids.find(p);
            if (it != ids.end()) return it->second;
            const int32_t id = (int32_t)ids.size();
            ids.emplace(p, id);
            detail::put3(world_, p->GetWorldPos());
            bad_.push_back(p->isBad() ? 1 : 0);
            return id;
        };
        KeyFrameT *kf[2] = {pKF1, pKF2};
        for (int s = 0; s < 2; s++) {
            const int n = (int)kf[s]->mvKeysUn.size();
            n_[s] = n;
            keys_[s].resize(std::max(n, 1));
            if (n) std::memcpy((void *)keys_[s].data(), kf[s]->mvKeysUn.data(), (size_t)n * sizeof(plf_keypoint));
            mps_[s].assign(std::max(n, 1), -1);
            obs_[s].assign(std::max(n, 1), -1);
            pose_[s] = detail::frustum_pose(kf[s]->GetRotation(), kf[s]->GetTranslation());
        }
        sigma2_.assign(pKF1->mvLevelSigma2.begin(), pKF1->mvLevelSigma2.end());
        cam_ = plf_camera{};
        cam_.fx = pKF1->fx; cam_.fy = pKF1->fy; cam_.cx = pKF1->cx; cam_.cy = pKF1->cy;
        match_.assign(std::max(n_[0], 1), -1);
        // a key point of keyframe 2 that stands for each matched point: its GetIndexInKeyFrame when that is a key point, else none (the reference skips it)
        for (int i1 = 0; i1 < mN1 && i1 < n_[0]; i1++) {
            MapPointT *pMP2 = vpMatched12[i1];
            if (!pMP2) continue;
            MapPointT *pMP1 = i1 < (int)vpKeyFrameMP1.size() ? vpKeyFrameMP1[i1] : nullptr;
            if (!pMP1) continue;
            const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (i2 < 0 || i2 >= n_[1]) continue;
            mps_[0][i1] = id_of(pMP1); obs_[0][i1] = pMP1->GetIndexInKeyFrame(pKF1);
            mps_[1][i2] = id_of(pMP2); obs_[1][i2] = i2;
            match_[i1] = i2;
        }
        if (world_.empty()) { world_.assign(3, 0.0f); bad_.assign(1, 1); }
    }
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        prob_ = probability; min_inliers_ = minInliers; max_iterations_ = maxIterations;
        Draw();
        batch_.reset();
        own_.clear();
    }
    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        std::vector<Sim3Solver *> me(1, this);
        std::vector<cv::Mat> T;
        std::vector<bool> no_more;
        if (!batch_) { own_ = me; Prepare(own_, batch_, held_); }
        Step(own_, *batch_, nIterations, T, no_more);
        bNoMore = no_more[0];
        vbInliers = vbInliers_; nInliers = nInliers_;
        return T[0];
    }
    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers)
    {
        bool bFlag;
        return iterate(max_iterations_, bFlag, vbInliers12, nInliers);
    }
    cv::Mat GetEstimatedRotation() { return best_R_; }
    cv::Mat GetEstimatedTranslation() { return best_t_; }
    float GetEstimatedScale() { return best_s_; }
    // what the last Step() / iterate() left for this solver: vbInliers and nInliers of the reference's iterate()
    const std::vector<bool> &LastInliers() const { return vbInliers_; }
    int LastInlierCount() const { return nInliers_; }

    // everything a prepared vector of solvers keeps on the device
    struct Held {
        std::vector<std::unique_ptr<plf::DeviceArray<plf_keypoint>>> keys;
        std::vector<std::unique_ptr<plf::DeviceArray<int32_t>>> mps, obs;
        plf::DeviceArray<const plf_keypoint *> t_keys;
        plf::DeviceArray<const int32_t *> t_mps, t_obs;
        plf::DeviceArray<int32_t> kf_n, kf1, kf2, match;
        plf::DeviceArray<plf_frustum_pose> pose;
        plf::DeviceArray<float> world, sigma2;
        plf::DeviceArray<uint8_t> bad;
    };
    // the constructor of every solver in one launch (their SetRansacParameters must agree); then Step() is one round of LoopClosing::ComputeSim3
    static void Prepare(const std::vector<Sim3Solver *> &solvers, std::unique_ptr<plf::Sim3Batch> &batch, Held &h)
    {
        for (Sim3Solver *s : solvers) if (s->rand3_.empty()) s->Draw();
        const int J = (int)solvers.size(), device = solvers[0]->device_;
        int S = 1, RS = 1;
        for (Sim3Solver *s : solvers) { S = std::max(S, s->n_[0]); RS = std::max(RS, s->max_iterations_); }
        std::vector<const plf_keypoint *> t_keys;
        std::vector<const int32_t *> t_mps, t_obs;
        std::vector<int32_t> kf_n, kf1, kf2, match((size_t)J * S, -1), rand3((size_t)J * RS * 3, 0);
        std::vector<plf_frustum_pose> pose;
        std::vector<float> world;
        std::vector<uint8_t> bad, fix;
        h.keys.clear(); h.mps.clear(); h.obs.clear();
        for (int j = 0; j < J; j++) {
            Sim3Solver *s = solvers[j];
            const int32_t base = (int32_t)bad.size();
            for (int k = 0; k < 2; k++) {
                std::vector<int32_t> ids = s->mps_[k];
                for (int32_t &id : ids) if (id >= 0) id += base;
                h.keys.emplace_back(new plf::DeviceArray<plf_keypoint>(s->keys_[k], device));
                h.mps.emplace_back(new plf::DeviceArray<int32_t>(ids, device));
                h.obs.emplace_back(new plf::DeviceArray<int32_t>(s->obs_[k], device));
                t_keys.push_back(h.keys.back()->get()); t_mps.push_back(h.mps.back()->get()); t_obs.push_back(h.obs.back()->get());
                kf_n.push_back(s->n_[k]); pose.push_back(s->pose_[k]);
            }
            world.insert(world.end(), s->world_.begin(), s->world_.end());
            bad.insert(bad.end(), s->bad_.begin(), s->bad_.end());
            kf1.push_back(2 * j); kf2.push_back(2 * j + 1);
            fix.push_back(s->mbFixScale ? 1 : 0);
            std::copy(s->match_.begin(), s->match_.begin() + std::min<size_t>(s->match_.size(), (size_t)S), match.begin() + (size_t)j * S);
            std::copy(s->rand3_.begin(), s->rand3_.end(), rand3.begin() + (size_t)j * RS * 3);
        }
        h.t_keys.assign(t_keys, device); h.t_mps.assign(t_mps, device); h.t_obs.assign(t_obs, device);
        h.kf_n.assign(kf_n, device); h.kf1.assign(kf1, device); h.kf2.assign(kf2, device); h.match.assign(match, device); h.pose.assign(pose, device);
        h.world.assign(world, device); h.bad.assign(bad, device); h.sigma2.assign(solvers[0]->sigma2_, device);
        batch.reset(new plf::Sim3Batch(J, S, S, RS, 1, device));
        batch->fix_scale.upload(fix.data(), fix.size());
        batch->rand3.upload(rand3.data(), rand3.size());
        batch->SetRansacParameters(solvers[0]->prob_, solvers[0]->min_inliers_, solvers[0]->max_iterations_);
        plf_sim3_view v = {};
        v.n_kf = 2 * J; v.kf_keys = h.t_keys.get(); v.kf_n = h.kf_n.get(); v.kf_pose = h.pose.get(); v.kf_mappoints = h.t_mps.get(); v.kf_obs_index = h.t_obs.get();
        v.world_pos = h.world.get(); v.point_bad = h.bad.get(); v.n_points = (int32_t)bad.size(); v.level_sigma2 = h.sigma2.get();
        v.nlevels = (int32_t)solvers[0]->sigma2_.size();
        batch->Pairs(v, solvers[0]->cam_, h.kf1.get(), h.kf2.get(), h.match.get(), nullptr);
    }
    // iterate(nIterations) of every solver that has not said bNoMore, in one device call; T[j] is empty where solver j did not return a transform.  A
    // solver that hits is set back to its hit, where the reference's iterate() returned: its next call goes on from the iteration after.
    static void Step(const std::vector<Sim3Solver *> &solvers, plf::Sim3Batch &b, int nIterations, std::vector<cv::Mat> &T, std::vector<bool> &bNoMore)
    {
        const int J = (int)solvers.size();
        b.Iterate(nIterations, nullptr, nullptr);
        const std::vector<int32_t> n_hits = b.n_hits.download(), hit_iter = b.hit_iter.download(), hit_inliers = b.hit_inliers.download(), max_its = b.max_its.download();
        std::vector<int32_t> done = b.iterations_done.download(), best = b.best_inliers.download(), best_iter = b.best_iter.download();
        const std::vector<float> hit_sim3 = b.hit_sim3.download();
        std::vector<float> best_sim3 = b.best_sim3.download();
        std::vector<uint8_t> no_more = b.no_more.download();
        const std::vector<uint8_t> rows = b.hit_inlier12.download();
        T.assign(J, cv::Mat()); bNoMore.assign(J, false);
        bool patched = false;
        for (int j = 0; j < J; j++) {
            Sim3Solver *s = solvers[j];
            s->vbInliers_.assign(s->mN1, false); s->nInliers_ = 0;
            if (n_hits[j] > 0) {
                done[j] = hit_iter[j]; best[j] = hit_inliers[j]; best_iter[j] = hit_iter[j]; no_more[j] = hit_iter[j] >= max_its[j];
                std::copy(hit_sim3.begin() + (size_t)j * 13, hit_sim3.begin() + (size_t)(j + 1) * 13, best_sim3.begin() + (size_t)j * 13);
                patched = true;
                for (int i = 0; i < s->mN1 && i < b.S; i++) s->vbInliers_[i] = rows[(size_t)j * b.S + i] != 0;
                s->nInliers_ = hit_inliers[j];
            } else bNoMore[j] = no_more[j] != 0;
            const float *q = best_sim3.data() + (size_t)j * 13;
            s->best_R_ = cv::Mat(3, 3, CV_32F); s->best_t_ = detail::mat31(q + 9); s->best_s_ = q[12];
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) s->best_R_.template at<float>(r, c) = q[3 * r + c];
            if (n_hits[j] > 0) {
                plf_pose34 sRt;                                      // T12 = [s R | t]
                for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) sRt.Tcw[4 * r + c] = q[3 * r + c] * q[12] + 0.0f; sRt.Tcw[4 * r + 3] = q[9 + r]; }
                T[j] = detail::mat44(sRt);
            }
        }
        if (patched) {
            b.iterations_done.upload(done.data(), done.size()); b.best_inliers.upload(best.data(), best.size()); b.best_iter.upload(best_iter.data(), best_iter.size());
            b.best_sim3.upload(best_sim3.data(), best_sim3.size()); b.no_more.upload(no_more.data(), no_more.size());
        }
    }
private:
    void Draw()
    {
        rand3_.resize((size_t)max_iterations_ * 3);
        for (int32_t &r : rand3_) r = (int32_t)rand();
    }
    bool mbFixScale;
    int device_, mN1 = 0, n_[2] = {0, 0}, min_inliers_ = 6, max_iterations_ = 300, nInliers_ = 0;
    double prob_ = 0.99;
    std::vector<plf_keypoint> keys_[2];
    std::vector<int32_t> mps_[2], obs_[2], match_, rand3_;
    plf_frustum_pose pose_[2];
    std::vector<float> world_, sigma2_;
    std::vector<uint8_t> bad_;
    plf_camera cam_;
    std::vector<bool> vbInliers_;
    cv::Mat best_R_, best_t_;
    float best_s_ = 1.0f;
    std::unique_ptr<plf::Sim3Batch> batch_;
    std::vector<Sim3Solver *> own_;
    Held held_;
};

// The two loops of LoopClosing::CorrectLoop (so@0x67fb0) that follow the construction of mvpCurrentConnectedKFs, over the reference's own KeyFrame / MapPoint
// / g2o::Sim3 and the CALLER'S OWN std::map<KeyFrame*, g2o::Sim3> (KeyFrameAndPose): the maps are filled here, and their iteration order -- the pointer order
// the caller's allocator produced -- is the rank order of the walk, as in the reference.  Reads GetPose(), GetCameraCenter(), mnId, GetMapPointMatches(),
// isBad(), GetWorldPos(), mnCorrectedByKF, GetObservations(), GetReferenceKeyFrame(), mvKeysUn, mvScaleFactors, mnScaleLevels; writes SetWorldPos(),
// mnCorrectedByKF, mnCorrectedReference and SetPose(), and returns per moved point what UpdateNormalAndDepth() leaves (mNormalVector / mfMinDistance /
// mfMaxDistance are protected in the reference: the forwarder inside MapPoint.cc assigns them).  UpdateConnections() per keyframe stays
// with the caller.  Uploads and waits: for one loop closure of a map that lives in host objects; a resident map calls plf::LoopCorrection.
struct LoopClosing {
    template <class MapPointT> struct Corrected {
        std::vector<MapPointT *> points;            // every point met in the rows, in order of first occurrence
        std::vector<int32_t> owner_rank, n;         // the rank that moved it (-1: left alone); observations counted (-1: leave the three members alone)
        std::vector<float> normal, minDistance, maxDistance;
    };
    template <class KeyFrameT, class MapPointT, class Sim3T, class KeyFrameAndPoseT>
    static Corrected<MapPointT> CorrectLoop(KeyFrameT *mpCurrentKF, const std::vector<KeyFrameT *> &mvpCurrentConnectedKFs, const Sim3T &mg2oScw,
                                            KeyFrameAndPoseT &CorrectedSim3, KeyFrameAndPoseT &NonCorrectedSim3, int device = 0)
    {
        Corrected<MapPointT> out;
        for (KeyFrameT *pKFi : mvpCurrentConnectedKFs) { CorrectedSim3[pKFi]; NonCorrectedSim3[pKFi]; }
        CorrectedSim3[mpCurrentKF]; NonCorrectedSim3[mpCurrentKF];
        std::vector<plf_pose34> tcw;
        std::vector<float> ow, scale, pos;
        std::vector<int64_t> kf_id, by;
        std::vector<int32_t> ref, level;
        auto g = detail::map_gather<KeyFrameT, MapPointT>(
            [&](KeyFrameT *pKF) { tcw.push_back(detail::pose34(pKF->GetPose())); detail::put3(ow, pKF->GetCameraCenter()); kf_id.push_back((int64_t)pKF->mnId); },
            [&](auto &gather, MapPointT *pMP, const auto &observations) {
                detail::put3(pos, pMP->GetWorldPos());
                by.push_back((int64_t)pMP->mnCorrectedByKF);
                ref.push_back(-1); level.push_back(0);
                detail::ref_level(gather, pMP->GetReferenceKeyFrame(), observations, scale, ref.back(), level.back());
            });
        std::vector<int32_t> rank_kf;               // slots: the K ranks first, in the map's order, then every other keyframe that observes a point
        for (auto &e : CorrectedSim3) rank_kf.push_back(g.slot(e.first));
        const int K = (int)rank_kf.size();
        for (auto &e : CorrectedSim3) g.row(e.first->GetMapPointMatches());
        out.points = g.pts;                         // every point met in the rows, in order of first occurrence
        const int P = (int)out.points.size(), S = (int)g.kfs.size();
        out.owner_rank.assign(P, -1); out.n.assign(P, -1);
        out.normal.assign((size_t)P * 3, 0.0f); out.minDistance.assign(P, 0.0f); out.maxDistance.assign(P, 0.0f);
        if (scale.empty()) scale.assign(1, 1.0f);
        const std::vector<double> scw8 = {mg2oScw.rotation().x(), mg2oScw.rotation().y(), mg2oScw.rotation().z(), mg2oScw.rotation().w(), mg2oScw.translation()[0],
                                          mg2oScw.translation()[1], mg2oScw.translation()[2], mg2oScw.scale()};
        plf::LoopCorrection lc(K, P, S, device);
        lc.scw.upload(scw8.data(), 8);
        const typename decltype(g)::Device d(g, device);
        plf::DeviceArray<plf_pose34> dtcw(tcw, device);
        plf::DeviceArray<float> dow(ow, device), dscale(scale, device), dpos(pos, device), dnormal(out.normal, device), dmin(out.minDistance, device),
            dmax(out.maxDistance, device);
        plf::DeviceArray<int32_t> drank(rank_kf, device), dref(ref, device), dlevel(level, device);
        plf::DeviceArray<int64_t> did(kf_id, device), dby(by, device), dcref(P, device);
        dcref.fill(0);
        const plf_loop_view rows = {K, drank.get(), d.row_start.get(), d.row_point.get(), P, d.point_bad.get(), S, did.get()};
        plf_map_geom_view geom = {};
        geom.n_points = P; geom.obs_start = d.obs_start.get(); geom.obs_kf = d.obs_kf.get(); geom.kf_ow = dow.get(); geom.n_kf = S; geom.ref_kf = dref.get();
        geom.ref_level = dlevel.get(); geom.scale_factors = dscale.get(); geom.nlevels = (int32_t)scale.size(); geom.point_bad = d.point_bad.get(); geom.pos_floats = 3;
        lc.Run(rows, g.slot(mpCurrentKF), (int64_t)mpCurrentKF->mnId, dtcw.get(), dow.get(), geom, dpos.get(), dby.get(), dcref.get(), dnormal.get(), dmin.get(),
               dmax.get(), rank_kf);
        // ---- back into the caller's objects (a NULL-stream download waits for the device first)
        const std::vector<double> cor = lc.corrected.download(), non = lc.noncorrected.download();
        auto put = [](Sim3T &S3, const double *o) {
            S3.rotation().x() = o[0]; S3.rotation().y() = o[1]; S3.rotation().z() = o[2]; S3.rotation().w() = o[3];
            S3.translation()[0] = o[4]; S3.translation()[1] = o[5]; S3.translation()[2] = o[6]; S3.scale() = o[7];
        };
        int r = 0;
        for (auto &e : CorrectedSim3) { put(e.second, &cor[8 * (size_t)r]); put(NonCorrectedSim3[e.first], &non[8 * (size_t)r]); r++; }
        if (P) {
            const std::vector<float> npos = dpos.download();
            const std::vector<int64_t> nby = dby.download(), ncref = dcref.download();
            out.owner_rank = lc.owner_rank.download(); out.n = lc.n_obs_used.download();
            out.owner_rank.resize(P); out.n.resize(P);
            out.normal = dnormal.download(); out.minDistance = dmin.download(); out.maxDistance = dmax.download();
            for (int p = 0; p < P; p++) {
                if (out.owner_rank[p] < 0) continue;
                out.points[p]->SetWorldPos(detail::mat31(&npos[(size_t)p * 3]));
                out.points[p]->mnCorrectedByKF = (decltype(out.points[p]->mnCorrectedByKF))nby[p];
                out.points[p]->mnCorrectedReference = (decltype(out.points[p]->mnCorrectedReference))ncref[p];
            }
        }
        const std::vector<plf_pose34> tn = lc.tcw_new.download();
        r = 0;
        for (auto &e : CorrectedSim3) e.first->SetPose(detail::mat44(tn[r++]));
        return out;
    }
};
}  // namespace ORB_SLAM2_PLF
#endif
#endif
