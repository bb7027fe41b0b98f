// Stand-in ORB_SLAM::MapPoint for the LocalMapPoints::Fuse / FuseInNeighbors harness: the members of tests/refresh_dropin/MapPoint.h and, under
// the reference's names (include/MapPoint.h), what Fuse and LocalMapping::SearchInNeighbors touch in addition: IsInKeyFrame, AddObservation,
// Replace (defined in KeyFrame.h of this directory, behind both classes) and mnFuseCandidateForKF.
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
    long unsigned int mnLastFrameSeen = 0;
    // variable used by the local mapping
    long unsigned int mnFuseCandidateForKF = (long unsigned int)-1;

    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMinDistanceInvariance() { return mfMinDistance; }
    float GetMaxDistanceInvariance() { return mfMaxDistance; }
    bool isBad() { return mbBad; }
    void IncreaseVisible() { mnVisible++; }
    std::map<KeyFrame*, std::size_t> GetObservations() { return mObservations; }
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    void AddObservation(KeyFrame* pKF, std::size_t idx) { mObservations[pKF] = idx; }                  // src/MapPoint.cc:79-86
    void Replace(MapPoint* pMP);                                                                       // src/MapPoint.cc:141-176

    // set by the harness
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    bool mbBad = false;
    int mnVisible = 1;
    std::map<KeyFrame*, std::size_t> mObservations;
    KeyFrame* mpRefKF = nullptr;
    static int nReplaced;                    // how often Replace ran
};

}  // namespace ORB_SLAM
