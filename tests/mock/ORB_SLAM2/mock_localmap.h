// MOCK of the members of ORB_SLAM2::KeyFrame / MapPoint / Frame / Tracking (include/KeyFrame.h, MapPoint.h, Frame.h, Tracking.h of the reference) that the
// local-map adapter of include/plf.hpp reads and writes -- same names, same types -- and a restatement of Tracking::UpdateLocalKeyFrames,
// Tracking::UpdateLocalPoints and the head of Tracking::SearchLocalPoints over them, as include/plf.h ("Local map") states the rules: real std::map,
// std::set and std::vector with pointer keys, a mark per frame.  Test infrastructure only; not to be included together with the other mocks (same
// class names).
#pragma once
#include <map>
#include <set>
#include <vector>
namespace ORB_SLAM2 {
class MapPoint;
class KeyFrame {
public:
    bool isBad() { return mbBad; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::set<KeyFrame *> GetChilds() { return mspChildrens; }
    KeyFrame *GetParent() { return mpParent; }
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = (long unsigned int)-1;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame *> mspChildrens;
    KeyFrame *mpParent = nullptr;
    bool mbBad = false;
};
class MapPoint {
public:
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    void AddObservation(KeyFrame *pKF, size_t idx) { mObservations[pKF] = idx; }
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = (long unsigned int)-1;
    long unsigned int mnLastFrameSeen = (long unsigned int)-1;
    bool mbTrackInView = false;
    int mnVisible = 1;
    bool mbBad = false;
protected:
    std::map<KeyFrame *, size_t> mObservations;
};
class Frame {
public:
    long unsigned int mnId = 0;
    int N = 0;
    std::vector<MapPoint *> mvpMapPoints;
};

// the three functions, restated
class Tracking {
public:
    Frame mCurrentFrame;
    std::vector<KeyFrame *> mvpLocalKeyFrames;
    std::vector<MapPoint *> mvpLocalMapPoints;
    KeyFrame *mpReferenceKF = nullptr;

    void UpdateLocalKeyFrames()
    {
        std::map<KeyFrame *, int> keyframeCounter;
        for (int i = 0; i < mCurrentFrame.N; i++) {
            MapPoint *pMP = mCurrentFrame.mvpMapPoints[i];
            if (!pMP) continue;
            if (pMP->isBad()) { mCurrentFrame.mvpMapPoints[i] = nullptr; continue; }
            const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
            for (const auto &ob : observations) keyframeCounter[ob.first]++;
        }
        if (keyframeCounter.empty()) return;
        int max = 0;
        KeyFrame *pKFmax = nullptr;
        mvpLocalKeyFrames.clear();
        for (const auto &kc : keyframeCounter) {
            KeyFrame *pKF = kc.first;
            if (pKF->isBad()) continue;
            if (kc.second > max) { max = kc.second; pKFmax = pKF; }
            mvpLocalKeyFrames.push_back(pKF);
            pKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
        }
        // begin() and end() are read once: indices over the seed count say the same without dangling when the vector grows
        const size_t seeds = mvpLocalKeyFrames.size();
        for (size_t s = 0; s < seeds; s++) {
            if (mvpLocalKeyFrames.size() > 80) break;
            KeyFrame *pKF = mvpLocalKeyFrames[s];
            const std::vector<KeyFrame *> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
            for (KeyFrame *pNeighKF : vNeighs)
                if (!pNeighKF->isBad() && pNeighKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pNeighKF);
                    pNeighKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;
                }
            const std::set<KeyFrame *> spChilds = pKF->GetChilds();
            for (KeyFrame *pChildKF : spChilds)
                if (!pChildKF->isBad() && pChildKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pChildKF);
                    pChildKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;
                }
            KeyFrame *pParent = pKF->GetParent();
            if (pParent && pParent->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                mvpLocalKeyFrames.push_back(pParent);
                pParent->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                break;
            }
        }
        if (pKFmax) mpReferenceKF = pKFmax;
    }

    void UpdateLocalPoints()
    {
        mvpLocalMapPoints.clear();
        for (KeyFrame *pKF : mvpLocalKeyFrames) {
            const std::vector<MapPoint *> vpMPs = pKF->GetMapPointMatches();
            for (MapPoint *pMP : vpMPs) {
                if (!pMP) continue;
                if (pMP->mnTrackReferenceForFrame == mCurrentFrame.mnId) continue;
                if (pMP->isBad()) continue;
                mvpLocalMapPoints.push_back(pMP);
                pMP->mnTrackReferenceForFrame = mCurrentFrame.mnId;
            }
        }
    }

    // isInFrustum(pMP) is the caller's: the head has no geometry of its own.  Returns nToMatch.
    template <class InFrustum> int SearchLocalPointsHead(InFrustum isInFrustum)
    {
        for (MapPoint *&pMP : mCurrentFrame.mvpMapPoints) {
            if (!pMP) continue;
            if (pMP->isBad()) { pMP = nullptr; continue; }
            pMP->IncreaseVisible();
            pMP->mnLastFrameSeen = mCurrentFrame.mnId;
            pMP->mbTrackInView = false;
        }
        int nToMatch = 0;
        for (MapPoint *pMP : mvpLocalMapPoints) {
            if (pMP->mnLastFrameSeen == mCurrentFrame.mnId) continue;
            if (pMP->isBad()) continue;
            if (isInFrustum(pMP)) { pMP->IncreaseVisible(); pMP->mbTrackInView = true; nToMatch++; }
        }
        return nToMatch;
    }
};
}  // namespace ORB_SLAM2
