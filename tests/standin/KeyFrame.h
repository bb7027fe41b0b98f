// Stand-in ORB_SLAM::KeyFrame for every drop-in harness (tests/*_dropin/harness.cpp, tests/kfdb_dropin aside): the members of the reference's
// include/KeyFrame.h that the drop-in classes of orb_slam_amd/cpp touch, under the reference's names.  Written for the harnesses: the members the
// reference protects are public and set by the harness (the pose as Rcw, tcw and Ow), connections and the spanning tree do not exist, and
// SetBadFlag does to the map points what a culled key frame does to them and sets the flag.  The n<Accessor> counters say how often an accessor
// was called: the drop-ins promise to fetch key points, matches and the FeatureVector once per upload.
//
// Who reads what:
//   ORBmatcherAccess.h                              GetKeyPointsUn, mfGridElementWidthInv/HeightInv, GetVectorScaleSigma2
//   LocalMapPointsSource.cc                         GetMapPointMatches, GetKeyPointsUn
//   NewMapPoints.cc, LocalMapPointsNewPoints.cc     GetRotation, GetTranslation, GetCameraCenter, fx, fy, cx, cy, GetScaleFactor(s), GetVectorScaleSigma2;
//                                                   the latter also GetMapPointMatches, isBad
//   LocalMapPointsRefresh.cc                        GetKeyPointsUn, GetDescriptors, GetDescriptor, GetCameraCenter, GetScaleFactors, isBad
//   LocalMapPointsFuse.cc, LocalMapPointsLoop.cc    the pose and camera, GetScaleFactors, GetScaleLevels, GetMapPointMatches, GetMapPoint(s), AddMapPoint,
//                                                   mnId; through MapPoint::Replace also ReplaceMapPointMatch, EraseMapPointMatch
//   LocalMapPointsSim3.cc                           GetRotation, GetTranslation, fx, fy, cx, cy, GetScaleFactors, GetScaleLevels, GetMapPointMatches
//   LocalMapPointsBoW.cc                            GetFeatureVector, GetMapPointMatches, isBad
//   LocalMapPointsLocalMap.cc                       GetMapPointMatches, GetKeyPointsUn, GetBestCovisibilityKeyFrames, isBad, mnId, mnTrackReferenceForFrame
//   LocalMapPointsCull.cc                           GetVectorCovisibleKeyFrames, GetMapPointMatches, GetScaleLevels, SetBadFlag, isBad, mnId
//
// -DSTANDIN_TRACKING_ONLY leaves what LocalMapPoints.cc, LocalMapPointsSource.cc and ORBmatcherAccess.h name: those two files must compile for a
// build that only wants the tracking searches (the Makefile checks it).
#pragma once
#include <cstddef>
#include <cstring>
#include <set>
#include <vector>

#include "Frame.h"              // DBoW2::FeatureVector
#include "MapPoint.h"
#include "cvmini.h"

namespace ORB_SLAM {

class KeyFrame {
public:
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::vector<MapPoint*> GetMapPointMatches() { nGetMapPointMatches++; return mvpMapPoints; }
    std::vector<cv::KeyPoint> GetKeyPointsUn() const { nGetKeyPointsUn++; return mvKeysUn; }
    cv::KeyPoint GetKeyPointUn(const std::size_t& idx) const { return mvKeysUn[idx]; }
    std::vector<float> GetVectorScaleSigma2() const { return mvLevelSigma2; }

    // set by the harness
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<float> mvLevelSigma2;
    mutable int nGetKeyPointsUn = 0;         // mutable: the reference's accessor is const
    int nGetMapPointMatches = 0;

#ifndef STANDIN_TRACKING_ONLY
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;                          // src/KeyFrame.cc:32
    float fx = 0, fy = 0, cx = 0, cy = 0;
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    float GetScaleFactor(int nLevel = 1) const { return mvScaleFactors[nLevel]; }
    std::vector<float> GetScaleFactors() const { return mvScaleFactors; }
    float GetSigma2(int nLevel = 1) const { return mvLevelSigma2[nLevel]; }
    int GetScaleLevels() const { return mnScaleLevels; }
    cv::Mat GetDescriptors() { return mDescriptors.clone(); }
    cv::Mat GetDescriptor(const std::size_t& idx) {
        cv::Mat d(1, 32, CV_8U);
        std::memcpy(d.ptr<unsigned char>(0), mDescriptors.ptr<unsigned char>((int)idx), 32);
        return d;
    }
    DBoW2::FeatureVector GetFeatureVector() { nGetFeatureVector++; return mFeatVec; }
    bool isBad() { return mbBad; }
    MapPoint* GetMapPoint(const std::size_t& idx) { return mvpMapPoints[idx]; }
    std::set<MapPoint*> GetMapPoints() {                                      // src/KeyFrame.cc:238-251: the good points the key frame holds
        std::set<MapPoint*> s;
        for (std::size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i] && !mvpMapPoints[i]->isBad()) s.insert(mvpMapPoints[i]);
        return s;
    }
    void AddMapPoint(MapPoint* pMP, const std::size_t& idx) { mvpMapPoints[idx] = pMP; }
    void ReplaceMapPointMatch(const std::size_t& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const std::size_t& idx) { mvpMapPoints[idx] = nullptr; }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {       // src/KeyFrame.cc:189-197: the first N of the ordered list
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    void SetNotErase() { mbNotErase = true; }
    // The first key frame is never given up and a protected one only remembers that it was asked; any other takes its observation away from every
    // point it holds and is bad from then on.
    void SetBadFlag() {
        if (mnId == 0) return;
        if (mbNotErase) { mbToBeErased = true; return; }
        for (std::size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
        mbBad = true;
    }

    // set by the harness
    int mnScaleLevels = 0;
    std::vector<float> mvScaleFactors;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    cv::Mat mDescriptors, Rcw, tcw, Ow;
    bool mbBad = false, mbNotErase = false, mbToBeErased = false;
    DBoW2::FeatureVector mFeatVec;
    int nGetFeatureVector = 0;
#endif
};

}  // namespace ORB_SLAM
