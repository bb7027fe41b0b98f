// Stand-in ORB_SLAM::MapPoint for the culling harness: what LocalMapPoints.cc, LocalMapPointsRefresh.cc, LocalMapPointsLocalMap.cc and
// LocalMapPointsCull.cc touch of a map point, under the reference's names, and the two functions through which a culled key frame changes the map:
// EraseObservation and SetBadFlag (defined behind KeyFrame in KeyFrame.h, which they need complete).  Written for this harness: the observation
// map is a plain std::map in pointer order, there are no locks, and the Map that the reference tells about a bad point does not exist here.
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
    long unsigned int mnTrackReferenceForFrame = 0;
    long unsigned int mnLastFrameSeen = 0;

    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMinDistanceInvariance() { return mfMinDistance; }
    float GetMaxDistanceInvariance() { return mfMaxDistance; }
    bool isBad() { return mbBad; }
    void IncreaseVisible() { mnVisible++; }
    std::map<KeyFrame*, std::size_t> GetObservations() { return mObservations; }
    int Observations() { return (int)mObservations.size(); }
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    // the key frame no longer observes this point; with two observers or fewer left the point is given up
    void EraseObservation(KeyFrame* pKF);
    // the point leaves the map: every key frame that still observes it drops its match
    void SetBadFlag();

    // set by the harness
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 1.f, mfMaxDistance = 4.f;
    bool mbBad = false;
    int mnVisible = 1;
    std::map<KeyFrame*, std::size_t> mObservations;
    KeyFrame* mpRefKF = nullptr;
};

}  // namespace ORB_SLAM
