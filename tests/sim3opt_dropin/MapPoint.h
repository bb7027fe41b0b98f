// Stand-in ORB_SLAM::MapPoint for the Sim3Optimizer drop-in harness (include/MapPoint.h): the position, the bad flag and the observations keyed by
// the key frame's pointer, as Optimizer::OptimizeSim3 reads them.
#pragma once
#include <cstddef>
#include <map>

#include "KeyFrame.h"
#include "cvmini.h"

namespace ORB_SLAM {

class MapPoint {
public:
    long unsigned int mnId = 0;
    cv::Mat mWorldPos = cv::Mat(3, 1, CV_32F);
    std::map<KeyFrame*, size_t> mObservations;
    bool mbBad = false;

    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
};

}  // namespace ORB_SLAM
