// MOCK of the members of ORB_SLAM2::MapPoint / MapLine / KeyFrame (include/MapPoint.h:53,75,146, MapLine.h:71,93,168, KeyFrame.h:231 of the reference)
// that the ComputeDistinctiveDescriptors adapter of include/plf.hpp reads -- same names, same types, mDescriptor / mLDescriptor protected as there.
// Test infrastructure only; not to be included together with mock_slam.h (same class names).
#pragma once
#include <map>
#include <vector>
#include <opencv2/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame {
public:
    bool isBad() { return mbBad; }
    cv::Mat mDescriptors;        // ORB, N x 32
    cv::Mat mLineDescriptors;    // LBD, NL x 32
    bool mbBad = false;
};
class MapPoint {
public:
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    void AddObservation(KeyFrame *pKF, size_t idx) { mObservations[pKF] = idx; }
    void ComputeDistinctiveDescriptors();                       // the forwarder: defined by the program that uses the mock, as MapPoint.cc would
    cv::Mat GetDescriptor() { return mDescriptor; }
protected:
    std::map<KeyFrame *, size_t> mObservations;
    cv::Mat mDescriptor;
};
class MapLine {
public:
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    void AddObservation(KeyFrame *pKF, size_t idx) { mObservations[pKF] = idx; }
    void ComputeDistinctiveDescriptors();
    cv::Mat GetDescriptor() { return mLDescriptor; }
protected:
    std::map<KeyFrame *, size_t> mObservations;
    cv::Mat mLDescriptor;
};
}  // namespace ORB_SLAM2
