// MOCK of the members of ORB_SLAM2::MapPoint / KeyFrame (include/MapPoint.h, KeyFrame.h of the reference) that the UpdateNormalAndDepth adapter of
// include/plf.hpp reads -- same names, same types, mNormalVector / mfMinDistance / mfMaxDistance protected as there.
// Test infrastructure only; not to be included together with the other mocks (same class names).
#pragma once
#include <map>
#include <vector>
#include <opencv2/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame {
public:
    cv::Mat GetCameraCenter() { return Ow; }
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    cv::Mat Ow;                  // 3 x 1 CV_32F (protected in the reference; the adapter goes through GetCameraCenter())
};
class MapPoint {
public:
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    cv::Mat GetWorldPos() { return mWorldPos; }
    void AddObservation(KeyFrame *pKF, size_t idx) { mObservations[pKF] = idx; }
    void UpdateNormalAndDepth();                                // the forwarder: defined by the program that uses the mock, as MapPoint.cc would
    cv::Mat GetNormal() { return mNormalVector; }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    cv::Mat mWorldPos;           // protected in the reference; public here so that the driver can place the point
    KeyFrame *mpRefKF = nullptr;
    bool mbBad = false;
    float mfMinDistance = 0, mfMaxDistance = 0;
protected:
    std::map<KeyFrame *, size_t> mObservations;
    cv::Mat mNormalVector;
};
}  // namespace ORB_SLAM2
