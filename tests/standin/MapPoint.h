// Stand-in ORB_SLAM::MapPoint for every drop-in harness (tests/*_dropin/harness.cpp, tests/kfdb_dropin aside): the members of the reference's
// include/MapPoint.h that the drop-in classes of orb_slam_amd/cpp touch, under the reference's names.  Written for the harnesses: the members the
// reference protects are public and set by the harness, the observation map is a plain std::map in pointer order, there are no locks and no Map.
//
// Who reads what:
//   LocalMapPoints.cc, LocalMapPointsSource.cc      GetWorldPos, GetNormal, GetDescriptor, GetMin/MaxDistanceInvariance, isBad, IncreaseVisible,
//                                                   mnId, mnLastFrameSeen; write mTrackProjX/Y, mbTrackInView, mnTrackScaleLevel, mTrackViewCos
//   PnPsolver.cc                                    GetWorldPos, isBad
//   LocalMapPointsRefresh.cc                        GetObservations, GetReferenceKeyFrame, GetWorldPos
//   LocalMapPointsFuse.cc, LocalMapPointsLoop.cc    GetObservations, IsInKeyFrame, AddObservation, Replace, mnFuseCandidateForKF
//   LocalMapPointsSim3.cc                           GetIndexInKeyFrame
//   LocalMapPointsLocalMap.cc                       the tracking members; mnTrackReferenceForFrame is there to show that it is left alone
//   LocalMapPointsCull.cc                           nothing of its own: a culled KeyFrame::SetBadFlag calls EraseObservation, that SetBadFlag
// Replace, EraseObservation and SetBadFlag need KeyFrame complete and are defined in harness_io.h.
//
// -DSTANDIN_TRACKING_ONLY leaves what LocalMapPoints.cc, LocalMapPointsSource.cc and ORBmatcherAccess.h name: those two files must compile for a
// build that only wants the tracking searches (the Makefile checks it).
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

    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMinDistanceInvariance() { return mfMinDistance; }
    float GetMaxDistanceInvariance() { return mfMaxDistance; }
    bool isBad() { return mbBad; }
    void IncreaseVisible() { mnVisible++; }

    // set by the harness
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    bool mbBad = false;
    int mnVisible = 1;

#ifndef STANDIN_TRACKING_ONLY
    long unsigned int mnTrackReferenceForFrame = 0;                          // src/MapPoint.cc:32
    // variable used by the local mapping
    long unsigned int mnFuseCandidateForKF = (long unsigned int)-1;

    std::map<KeyFrame*, std::size_t> GetObservations() { return mObservations; }
    int Observations() { return (int)mObservations.size(); }
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }   // src/MapPoint.cc:258-265
    void AddObservation(KeyFrame* pKF, std::size_t idx) { mObservations[pKF] = idx; }                            // src/MapPoint.cc:79-86
    void Replace(MapPoint* pMP);                                                                                 // src/MapPoint.cc:141-176
    // the key frame no longer observes this point; with two observers or fewer left the point is given up
    void EraseObservation(KeyFrame* pKF);
    // the point leaves the map: every key frame that still observes it drops its match
    void SetBadFlag();

    // set by the harness
    std::map<KeyFrame*, std::size_t> mObservations;
    KeyFrame* mpRefKF = nullptr;
    static int nReplaced;                    // how often Replace ran
#endif
};

}  // namespace ORB_SLAM
