// Stand-in ORB_SLAM::KeyFrame for the LocalMapPoints::CreateNewMapPoints harness: tests/bow_dropin/KeyFrame.h and, under the reference's names
// (include/KeyFrame.h), the level tables and GetScaleFactor that LocalMapPointsNewPoints.cc and NewMapPoints.cc read.  Frame.h (DBoW2::FeatureVector) is
// that of tests/bow_dropin, MapPoint.h that of tests/fuse_dropin, cvmini.h that of tests/mappoints_dropin.
#pragma once
#include <cstddef>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "Frame.h"              // DBoW2::FeatureVector
#include "MapPoint.h"
#include "cvmini.h"

namespace ORB_SLAM {

class KeyFrame {
public:
    long unsigned int mnId = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    cv::Mat GetRotation() { return Rcw.clone(); }
    cv::Mat GetTranslation() { return tcw.clone(); }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    std::vector<cv::KeyPoint> GetKeyPointsUn() const { getKeys++; return mvKeysUn; }
    std::vector<float> GetVectorScaleSigma2() const { return mvLevelSigma2; }
    float GetScaleFactor(int nLevel = 1) const { return mvScaleFactors[nLevel]; }
    float GetSigma2(int nLevel = 1) const { return mvLevelSigma2[nLevel]; }
    std::vector<float> GetScaleFactors() { return mvScaleFactors; }
    int GetScaleLevels() { return (int)mvScaleFactors.size(); }
    cv::Mat GetDescriptors() { return mDescriptors.clone(); }
    cv::Mat GetDescriptor(const std::size_t& idx) {
        cv::Mat d(1, 32, CV_8U);
        std::memcpy(d.ptr<unsigned char>(0), mDescriptors.ptr<unsigned char>((int)idx), 32);
        return d;
    }
    bool isBad() { return mbBad; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    DBoW2::FeatureVector GetFeatureVector() { getFeatVec++; return mFeatVec; }
    MapPoint* GetMapPoint(const std::size_t& idx) { return mvpMapPoints[idx]; }
    std::set<MapPoint*> GetMapPoints() {                                      // the good points the key frame holds
        std::set<MapPoint*> s;
        for (std::size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i] && !mvpMapPoints[i]->isBad()) s.insert(mvpMapPoints[i]);
        return s;
    }
    void AddMapPoint(MapPoint* pMP, const std::size_t& idx) { mvpMapPoints[idx] = pMP; }
    void ReplaceMapPointMatch(const std::size_t& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const std::size_t& idx) { mvpMapPoints[idx] = nullptr; }

    // set by the harness
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors, mvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;
    cv::Mat mDescriptors, Rcw, tcw, Ow;
    bool mbBad = false;
    DBoW2::FeatureVector mFeatVec;
    mutable int getKeys = 0;                 // how often the key points were fetched
    int getFeatVec = 0;                      // how often the FeatureVector was fetched
};

// src/MapPoint.cc:141-176 without the descriptor update and the map's bookkeeping
inline void MapPoint::Replace(MapPoint* pMP) {
    if (pMP->mnId == mnId) return;
    nReplaced++;
    const std::map<KeyFrame*, std::size_t> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    for (std::map<KeyFrame*, std::size_t>::const_iterator mit = obs.begin(); mit != obs.end(); ++mit) {
        KeyFrame* pKF = mit->first;
        if (!pMP->IsInKeyFrame(pKF)) {
            pKF->ReplaceMapPointMatch(mit->second, pMP);
            pMP->AddObservation(pKF, mit->second);
        } else {
            pKF->EraseMapPointMatch(mit->second);
        }
    }
}

}  // namespace ORB_SLAM
