// Stand-in ORB_SLAM::MapPoint for the local-map harness: the members of the reference's include/MapPoint.h that LocalMapPoints.cc,
// LocalMapPointsRefresh.cc and LocalMapPointsLocalMap.cc touch, under the reference's names, and mnTrackReferenceForFrame, which the drop-in
// deliberately leaves alone (the harness prints it to show that).
#pragma once
#include <cstddef>
#include <map>

#include "cvmini.h"

namespace ORB_SLAM {

class KeyFrame;

class MapPoint {
public:
    MapPoint() : mWorldPos(3, 1, CV_32F), mNormalVector(3, 1, CV_32F), mDescriptor(1, 32, CV_8U) {}
    long unsigned int mnId = 0;
    // variables used by the tracking
    float mTrackProjX = 0, mTrackProjY = 0;
    bool mbTrackInView = false;
    int mnTrackScaleLevel = 0;
    float mTrackViewCos = 0;
    long unsigned int mnTrackReferenceForFrame = 0;      // src/MapPoint.cc:32
    long unsigned int mnLastFrameSeen = 0;

    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMinDistanceInvariance() { return mfMinDistance; }
    float GetMaxDistanceInvariance() { return mfMaxDistance; }
    bool isBad() { return mbBad; }
    void IncreaseVisible() { mnVisible++; }
    std::map<KeyFrame*, std::size_t> GetObservations() { return mObservations; }
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }

    // set by the harness
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    bool mbBad = false;
    int mnVisible = 1;
    std::map<KeyFrame*, std::size_t> mObservations;
    KeyFrame* mpRefKF = nullptr;
};

}  // namespace ORB_SLAM
