// Stand-in ORB_SLAM::KeyFrame: only what ORBmatcherAccess.h's key-frame overloads name (LocalMapPoints.cc never calls them).
#pragma once
#include <vector>

#include "cvmini.h"

namespace ORB_SLAM {

class KeyFrame {
public:
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::vector<cv::KeyPoint> GetKeyPointsUn() const { return std::vector<cv::KeyPoint>(); }
    std::vector<float> GetVectorScaleSigma2() const { return std::vector<float>(); }
};

}  // namespace ORB_SLAM
