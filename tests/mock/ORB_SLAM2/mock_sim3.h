// MOCK of the members of ORB_SLAM2::KeyFrame / MapPoint (include/KeyFrame.h, MapPoint.h of the reference) that the adapter
// ORB_SLAM2_PLF::Sim3Solver of include/plf.hpp reads -- same names, same types.  Test infrastructure only; not to be included together with the other
// mocks (same class names).
#pragma once
#include <map>
#include <vector>
#include <opencv2/core.hpp>
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
    std::vector<float> mvLevelSigma2;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat Rcw, tcw;                                                // 3 x 3, 3 x 1 CV_32F (behind the getters in the reference)
};
}  // namespace ORB_SLAM2
