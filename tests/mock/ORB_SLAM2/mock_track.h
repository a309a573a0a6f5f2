// MOCK of the members of ORB_SLAM2::Tracking / Frame / KeyFrame / MapPoint / Map / LocalMapping (include/Tracking.h, Frame.h, KeyFrame.h, MapPoint.h, Map.h,
// LocalMapping.h of the reference) that the tracking-tail adapters of include/plf.hpp read and write -- same names, same types (fx, fy, cx, cy static as
// there).  Test infrastructure only; not to be included together with the other mocks (same class names).
#pragma once
#include <vector>
#include <opencv2/core.hpp>
namespace ORB_SLAM2 {
class MapPoint {
public:
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    int nObs = 0;
    bool mbBad = false;
    cv::Mat mWorldPos;           // what the driver's make() stores
    int made_for = -1;           // and the key point it was made for
};
class KeyFrame {
public:
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<MapPoint *> mvpMapPoints;
};
class Frame {
public:
    cv::Mat GetRotationInverse() { return mRwc; }
    cv::Mat GetCameraCenter() { return mOw; }
    long unsigned int mnId = 0;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvDepth;
    std::vector<MapPoint *> mvpMapPoints;
    inline static float fx = 0, fy = 0, cx = 0, cy = 0;
    float mbf = 0;
    cv::Mat mRwc, mOw;           // 3 x 3, 3 x 1 CV_32F (private in the reference, read through the two getters)
};
class Map {
public:
    long unsigned int KeyFramesInMap() { return nKFs; }
    long unsigned int nKFs = 0;
};
class LocalMapping {
public:
    bool isStopped() { return stopped; }
    bool stopRequested() { return stop_requested; }
    bool AcceptKeyFrames() { return accept; }
    void InterruptBA() { interrupted++; }
    int KeyframesInQueue() { return queue; }
    bool stopped = false, stop_requested = false, accept = true;
    int interrupted = 0, queue = 0;
};
class Tracking {
public:
    int mSensor = 2;             // System::RGBD; 0 = MONOCULAR
    bool mbOnlyTracking = false;
    Frame mCurrentFrame;
    KeyFrame *mpReferenceKF = nullptr;
    LocalMapping *mpLocalMapper = nullptr;
    Map *mpMap = nullptr;
    int mnMatchesInliers = 0, mMinFrames = 0, mMaxFrames = 30;
    unsigned int mnLastKeyFrameId = 0, mnLastRelocFrameId = 0;
    float mThDepth = 0;
};
}  // namespace ORB_SLAM2
