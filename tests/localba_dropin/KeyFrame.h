// Stand-in ORB_SLAM::KeyFrame for the BundleAdjuster drop-in harness: the members Optimizer::LocalBundleAdjustment and BundleAdjustment touch, under
// the reference's names (include/KeyFrame.h).  tests/standin lacks SetPose, GetInvSigma2 and the mnBA* marks, so this directory has its own.  Every
// EraseMapPointMatch is logged in call order (ErasedLog), which is what the test compares.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "cvmini.h"

namespace ORB_SLAM {

class MapPoint;

class KeyFrame {
public:
    long unsigned int mnId = 0;
    long unsigned int mnBALocalForKF = 0, mnBAFixedForKF = 0;         // KeyFrame.cc:43-44 initialise both to 0
    float fx = 0, fy = 0, cx = 0, cy = 0;
    bool mbBad = false;
    cv::Mat Tcw;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2, mvInvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    int nSetPose = 0;

    cv::Mat GetPose() { return Tcw.clone(); }
    void SetPose(const cv::Mat& T) { Tcw = T.clone(); nSetPose++; }
    bool isBad() { return mbBad; }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    cv::KeyPoint GetKeyPointUn(const size_t& idx) const { return mvKeysUn[idx]; }
    float GetSigma2(int nLevel) const { return mvLevelSigma2[nLevel]; }
    float GetInvSigma2(int nLevel) const { return mvInvLevelSigma2[nLevel]; }
    // KeyFrame.cc:219-230
    void EraseMapPointMatch(const size_t& idx) {
        ErasedLog().push_back(std::make_pair(mnId, (long)idx));
        mvpMapPoints[idx] = NULL;
    }
    void EraseMapPointMatch(MapPoint* pMP);                            // defined in MapPoint.h

    static std::vector<std::pair<long unsigned int, long> >& ErasedLog() {
        static std::vector<std::pair<long unsigned int, long> > log;
        return log;
    }
};

}  // namespace ORB_SLAM
