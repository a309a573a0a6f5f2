// MOCK of the members of ORB_SLAM2::KeyFrame / Frame (include/KeyFrame.h:77-92,145,211, include/Frame.h:135,185 of the reference) that the KeyFrameDatabase
// adapter of include/plf.hpp reads -- same names, same types.  Test infrastructure only; not to be included together with mock_slam.h / mock_map.h
// (same class names).
#pragma once
#include <set>
#include <vector>
#include "DBoW2/mock_dbow2.h"
namespace ORB_SLAM2 {
class KeyFrame {
public:
    std::set<KeyFrame *> GetConnectedKeyFrames() { return std::set<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.end()); }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
};
class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};
}  // namespace ORB_SLAM2
