// Stand-in ORB_SLAM::Frame for the LocalMapPoints::SearchByBoW harness: tests/mappoints_dropin/Frame.h and, under the reference's names
// (include/Frame.h), mvKeys and mFeatVec, which LocalMapPointsBoW.cc uploads per call.
#pragma once
#include <cstddef>
#include <vector>

#include <map>

#include "cvmini.h"

#ifndef BOW_DROPIN_FEATURE_VECTOR
#define BOW_DROPIN_FEATURE_VECTOR
namespace DBoW2 {
typedef unsigned int NodeId;
class FeatureVector : public std::map<NodeId, std::vector<unsigned int> > {};
}  // namespace DBoW2
#endif

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
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    DBoW2::FeatureVector mFeatVec;
    cv::Mat mDescriptors;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
    cv::Mat mTcw;
    long unsigned int mnId = 0;
    int mnScaleLevels = 0;
    std::vector<float> mvScaleFactors;
};

}  // namespace ORB_SLAM
