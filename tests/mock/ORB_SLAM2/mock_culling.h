// MOCK of the members of ORB_SLAM2::KeyFrame / MapPoint (include/KeyFrame.h, MapPoint.h of the reference) that the KeyFrameCulling adapter of
// include/plf.hpp reads -- same names, same types -- and of what the caller runs on its result: KeyFrame::SetBadFlag -> MapPoint::EraseObservation ->
// MapPoint::SetBadFlag -> KeyFrame::EraseMapPointMatch, restated from the rule in include/plf.h ("Culling").  mbNotErase is public here so that the driver
// can set it.  Test infrastructure only; not to be included together with the other mocks (same class names).
#pragma once
#include <map>
#include <vector>
#include <opencv2/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
public:
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    int Observations() { return nObs; }
    inline void AddObservation(KeyFrame *pKF, size_t idx);
    inline void EraseObservation(KeyFrame *pKF);
    inline void SetBadFlag();
    long unsigned int mnId = 0;
    bool mbBad = false;
    int nObs = 0;
protected:
    std::map<KeyFrame *, size_t> mObservations;
};
class KeyFrame {
public:
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    bool isBad() { return mbBad; }
    void EraseMapPointMatch(const size_t &idx) { if (idx < mvpMapPoints.size()) mvpMapPoints[idx] = nullptr; }
    void SetBadFlag()
    {
        if (mnId == 0) return;
        if (mbNotErase) { mbToBeErased = true; return; }
        for (MapPoint *pMP : mvpMapPoints) if (pMP) pMP->EraseObservation(this);
        mbBad = true;
    }
    long unsigned int mnId = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    float mThDepth = 0;
    std::vector<MapPoint *> mvpMapPoints;
    bool mbNotErase = false, mbToBeErased = false, mbBad = false;
};
inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx)
{
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs += idx < pKF->mvuRight.size() && pKF->mvuRight[idx] >= 0 ? 2 : 1;
}
inline void MapPoint::EraseObservation(KeyFrame *pKF)
{
    const auto it = mObservations.find(pKF);
    if (it == mObservations.end()) return;
    const size_t idx = it->second;
    nObs -= idx < pKF->mvuRight.size() && pKF->mvuRight[idx] >= 0 ? 2 : 1;
    mObservations.erase(it);
    if (nObs <= 2) SetBadFlag();
}
inline void MapPoint::SetBadFlag()
{
    const std::map<KeyFrame *, size_t> obs = mObservations;
    mbBad = true;
    mObservations.clear();
    for (const auto &ob : obs) ob.first->EraseMapPointMatch(ob.second);
}
}  // namespace ORB_SLAM2
