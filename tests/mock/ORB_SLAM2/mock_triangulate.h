// MOCK of the members of ORB_SLAM2::KeyFrame / MapPoint (include/KeyFrame.h, MapPoint.h of the reference) that the adapter
// ORB_SLAM2_PLF::LocalMapping::CreateNewMapPoints of include/plf.hpp reads and writes -- same names, same types.  Test infrastructure only; not to be
// included together with the other mocks (same class names).
#pragma once
#include <vector>
#include <DBoW2/mock_dbow2.h>
#include <opencv2/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF) : mnId(nNextId++), mWorldPos(Pos), mpRefKF(pRefKF) {}
    void AddObservation(KeyFrame *pKF, size_t idx) { obs.push_back({pKF, idx}); }
    long unsigned int mnId;
    inline static long unsigned int nNextId = 0;
    cv::Mat mWorldPos;
    KeyFrame *mpRefKF;
    std::vector<std::pair<KeyFrame *, size_t>> obs;
};
class KeyFrame {
public:
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    cv::Mat GetRotation() { return Rcw; }
    cv::Mat GetTranslation() { return tcw; }
    cv::Mat GetCameraCenter() { return Ow; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    long unsigned int mnId = 0;
    int N = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0, mb = 0, mfScaleFactor = 0, mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors;                                            // N x 32 CV_8U
    DBoW2::FeatureVector mFeatVec;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    cv::Mat Rcw, tcw, Ow;                                            // 3 x 3, 3 x 1, 3 x 1 CV_32F (behind the three getters in the reference)
    cv::Mat F12_from_current;                                        // what the driver's ComputeF12 returns for (current, this)
};
}  // namespace ORB_SLAM2
