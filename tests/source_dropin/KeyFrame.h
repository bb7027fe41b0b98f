// Stand-in ORB_SLAM::KeyFrame: the accessors of the reference's include/KeyFrame.h that LocalMapPointsSource.cc and ORBmatcherAccess.h call.
#pragma once
#include <cstddef>
#include <vector>

#include "cvmini.h"

namespace ORB_SLAM {

class MapPoint;

class KeyFrame {
public:
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<cv::KeyPoint> GetKeyPointsUn() const { return mvKeysUn; }
    cv::KeyPoint GetKeyPointUn(const std::size_t& idx) const { return mvKeysUn[idx]; }
    std::vector<float> GetVectorScaleSigma2() const { return std::vector<float>(); }

    // set by the harness
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint*> mvpMapPoints;
};

}  // namespace ORB_SLAM
