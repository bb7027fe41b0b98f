// Stand-in ORB_SLAM::Frame for the culling harness (the one of tests/localmap_dropin, here so that this directory's MapPoint.h is the one it meets): the public members of the reference's include/Frame.h that LocalMapPoints.cc,
// LocalMapPointsLocalMap.cc and ORBmatcherAccess.h read, under the reference's names and types.
#pragma once
#include <cstddef>
#include <vector>

#include "cvmini.h"

#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

namespace ORB_SLAM {

class MapPoint;
class KeyFrame;

class Frame {
public:
    static float fx, fy, cx, cy;
    static int mnMinX, mnMaxX, mnMinY, mnMaxY;
    static float mfGridElementWidthInv, mfGridElementHeightInv;
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
    cv::Mat mTcw;
    long unsigned int mnId = 0;
    int mnScaleLevels = 0;
    std::vector<float> mvScaleFactors;
};

}  // namespace ORB_SLAM
