// MOCK of the members of ORB_SLAM2::KeyFrame / MapPoint (include/KeyFrame.h, MapPoint.h of the reference) and of g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h)
// that the adapter ORB_SLAM2_PLF::Optimizer::OptimizeSim3 of include/plf.hpp reads and writes -- same names, same types where the adapter sees them.  Test
// infrastructure only; not to be included together with the other mocks (same class names).
#pragma once
#include <map>
#include <vector>
#include <opencv2/core.hpp>
namespace g2o {
// the accessors of Eigen::Quaterniond / Eigen::Vector3d that the adapter uses
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
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame *pKF) { auto it = mObservations.find(pKF); return it != mObservations.end() ? (int)it->second : -1; }
    cv::Mat mWorldPos;                                               // 3 x 1 CV_32F
    bool mbBad = false;
    std::map<KeyFrame *, size_t> mObservations;
};
class KeyFrame {
public:
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    cv::Mat GetRotation() { return Rcw; }
    cv::Mat GetTranslation() { return tcw; }
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<float> mvInvLevelSigma2;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Rcw, tcw;                                                // 3 x 3, 3 x 1 CV_32F (behind the getters in the reference)
};
}  // namespace ORB_SLAM2
