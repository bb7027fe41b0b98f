// Stand-in ORB_SLAM::MapPoint for the LocalMapPoints::SearchBySim3 harness: the members of tests/fuse_dropin/MapPoint.h and, under the reference's
// name (include/MapPoint.h), MapPoint::GetIndexInKeyFrame, which LocalMapPointsSim3.cc asks of the points that are in vpMatches12 on entry.  Found
// ahead of tests/fuse_dropin's by the include order; KeyFrame.h is that of tests/loop_dropin, Frame.h and cvmini.h those of tests/mappoints_dropin.
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
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }   // src/MapPoint.cc:258-265
    void AddObservation(KeyFrame* pKF, std::size_t idx) { mObservations[pKF] = idx; }
    void Replace(MapPoint* pMP);

    // set by the harness
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    bool mbBad = false;
    int mnVisible = 1;
    std::map<KeyFrame*, std::size_t> mObservations;
    KeyFrame* mpRefKF = nullptr;
    static int nReplaced;
};

}  // namespace ORB_SLAM
