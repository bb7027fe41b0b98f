// Stand-in ORB_SLAM::KeyFrame for the culling harness: what LocalMapPointsRefresh.cc and LocalMapPointsLocalMap.cc read of a key frame and, under the
// reference's names (include/KeyFrame.h), what LocalMapPointsCull.cc calls: GetVectorCovisibleKeyFrames, GetKeyPointsUn, GetScaleLevels, SetBadFlag,
// isBad; beside them SetNotErase and EraseMapPointMatch, through which the harness protects a key frame and a bad point leaves its observers.
// Written for this harness: SetBadFlag does to the map points what a culled key frame does to them and sets the flag; connections and the
// spanning tree do not exist here.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

#include "MapPoint.h"
#include "cvmini.h"

namespace ORB_SLAM {

class KeyFrame {
public:
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    std::vector<cv::KeyPoint> GetKeyPointsUn() const { keysRead++; return mvKeysUn; }
    std::vector<float> GetScaleFactors() { return mvScaleFactors; }
    int GetScaleLevels() { return mnScaleLevels; }
    cv::Mat GetDescriptors() { return mDescriptors.clone(); }
    cv::Mat GetDescriptor(const std::size_t& idx) {
        cv::Mat d(1, 32, CV_8U);
        std::memcpy(d.ptr<unsigned char>(0), mDescriptors.ptr<unsigned char>((int)idx), 32);
        return d;
    }
    std::vector<float> GetVectorScaleSigma2() const { return std::vector<float>(); }     // ORBmatcherAccess.h names these three; nothing here reads them
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    bool isBad() { return mbBad; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int&) { return std::vector<KeyFrame*>(); }   // no neighbours: the local key frames are those with votes
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    void EraseMapPointMatch(const std::size_t& idx) { mvpMapPoints[idx] = nullptr; }
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
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 8;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    cv::Mat mDescriptors, Ow;
    bool mbBad = false, mbNotErase = false, mbToBeErased = false;
    mutable int keysRead = 0;                // how often the key points were fetched
};

inline void MapPoint::EraseObservation(KeyFrame* pKF) {
    if (mObservations.erase(pKF) == 0) return;
    if (mObservations.size() <= 2) SetBadFlag();
}

inline void MapPoint::SetBadFlag() {
    mbBad = true;
    std::map<KeyFrame*, std::size_t> obs;
    obs.swap(mObservations);
    for (std::map<KeyFrame*, std::size_t>::iterator it = obs.begin(); it != obs.end(); ++it) it->first->EraseMapPointMatch(it->second);
}

}  // namespace ORB_SLAM
