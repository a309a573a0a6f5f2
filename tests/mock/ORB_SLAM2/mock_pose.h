// MOCK of the members of ORB_SLAM2::Frame / MapPoint (include/Frame.h, MapPoint.h of the reference) that the PoseOptimization adapter of include/plf.hpp
// reads and writes -- same names, same types (fx, fy, cx, cy static as there).  Test infrastructure only; not to be included together with the other mocks
// (same class names).
#pragma once
#include <vector>
#include <opencv2/core.hpp>
namespace ORB_SLAM2 {
class MapPoint {
public:
    cv::Mat GetWorldPos() { return mWorldPos; }
    cv::Mat mWorldPos;           // 3 x 1 CV_32F (protected in the reference; public here so that the driver can place the point)
};
class Frame {
public:
    void SetPose(cv::Mat Tcw) { mTcw = Tcw; }
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvInvLevelSigma2;
    inline static float fx = 0, fy = 0, cx = 0, cy = 0;
    float mbf = 0;
    cv::Mat mTcw;                // 4 x 4 CV_32F
};
}  // namespace ORB_SLAM2
