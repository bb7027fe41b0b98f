// Stand-in ORB_SLAM::KeyFrame for the KeyFrameDatabase drop-in harness: the public members the database reads and writes,
// with the reference's names and types (include/KeyFrame.h:160-165), and the two covisibility queries it calls.
#pragma once
#include <set>
#include <vector>

#include "ORBVocabulary.h"

namespace ORB_SLAM {

class KeyFrame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;

    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;

    // covisibility: the connected key frames, best first (the harness sets both)
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;

    std::set<KeyFrame*> GetConnectedKeyFrames() {
        return std::set<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.end());
    }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
};

}  // namespace ORB_SLAM
