// Stand-in ORB_SLAM::Frame: the members of the reference's include/Frame.h that PnPsolver.cc reads, over the stand-in OpenCV types of
// tests/mappoints_dropin/cvmini.h.  MapPoint.h is that of tests/mappoints_dropin.
#pragma once
#include <vector>

#include "cvmini.h"

namespace ORB_SLAM {

class Frame {
public:
    std::vector<cv::KeyPoint> mvKeysUn;          // undistorted key points
    std::vector<float> mvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0;
};

}  // namespace ORB_SLAM
