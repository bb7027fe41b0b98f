// Stand-in ORB_SLAM::Frame for the KeyFrameDatabase drop-in harness: the two members DetectRelocalisationCandidates reads.
#pragma once
#include "ORBVocabulary.h"

namespace ORB_SLAM {

class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};

}  // namespace ORB_SLAM
