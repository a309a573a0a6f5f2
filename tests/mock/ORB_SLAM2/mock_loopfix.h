// MOCK of the members of ORB_SLAM2::KeyFrame / MapPoint (include/KeyFrame.h, MapPoint.h of the reference) and of g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h)
// that the adapter ORB_SLAM2_PLF::LoopClosing::CorrectLoop of include/plf.hpp reads and writes -- same names, same types where the adapter sees them.  (The
// two tails have no adapter, so their members are not mocked.)  Test infrastructure only; not to be included together with the other mocks (same class names).
#pragma once
#include <map>
#include <vector>
#include <opencv2/core.hpp>
namespace g2o {
struct MockQuaterniond {
    double c[4] = {0, 0, 0, 1};
    double &x() { return c[0]; } double &y() { return c[1]; } double &z() { return c[2]; } double &w() { return c[3]; }
    const double &x() const { return c[0]; } const double &y() const { return c[1]; } const double &z() const { return c[2]; } const double &w() const { return c[3]; }
};
struct MockVector3d {
    double v[3] = {0, 0, 0};
    double &operator[](int i) { return v[i]; }
    const double &operator[](int i) const { return v[i]; }
};
struct Sim3 {
    MockQuaterniond r;
    MockVector3d t;
    double s = 1.0;
    const MockVector3d &translation() const { return t; }
    MockVector3d &translation() { return t; }
    const MockQuaterniond &rotation() const { return r; }
    MockQuaterniond &rotation() { return r; }
    const double &scale() const { return s; }
    double &scale() { return s; }
};
}  // namespace g2o
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    cv::Mat GetWorldPos() { return mWorldPos; }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = cv::Mat(3, 1, CV_32F); for (int k = 0; k < 3; k++) mWorldPos.at<float>(k, 0) = Pos.at<float>(k, 0); }
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    cv::Mat mWorldPos;                                               // 3 x 1 CV_32F (protected in the reference)
    bool mbBad = false;
    KeyFrame *mpRefKF = nullptr;
    std::map<KeyFrame *, size_t> mObservations;
};
class KeyFrame {
public:
    cv::Mat GetPose() { return Tcw; }
    cv::Mat GetCameraCenter() { return Ow; }
    void SetPose(const cv::Mat &T) { Tcw = cv::Mat(4, 4, CV_32F); for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw.at<float>(r, c) = T.at<float>(r, c); nSetPose++; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    long unsigned int mnId = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Tcw, Ow;                                                 // 4 x 4, 3 x 1 CV_32F (behind the getters in the reference)
    int nSetPose = 0;
};
}  // namespace ORB_SLAM2
