// MOCK of the members of ORB_SLAM2::KeyFrame / MapPoint / Frame (include/KeyFrame.h, MapPoint.h, Frame.h of the reference) that the covisibility adapter of
// include/plf.hpp reads -- same names, same types.  Test infrastructure only; not to be included together with the other mocks (same class names).
#pragma once
#include <map>
#include <vector>
namespace ORB_SLAM2 {
class MapPoint;
class KeyFrame {
public:
    bool isBad() { return mbBad; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    long unsigned int mnId = 0;
    std::vector<MapPoint *> mvpMapPoints;
    bool mbBad = false;
};
class MapPoint {
public:
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    void AddObservation(KeyFrame *pKF, size_t idx) { mObservations[pKF] = idx; }
    bool mbBad = false;
protected:
    std::map<KeyFrame *, size_t> mObservations;
};
class Frame {
public:
    int N = 0;
    std::vector<MapPoint *> mvpMapPoints;
};
}  // namespace ORB_SLAM2
