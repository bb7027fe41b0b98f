// Stand-in ORB_SLAM::KeyFrame for the Sim3Optimizer drop-in harness: the members Optimizer::OptimizeSim3 touches, under the reference's names
// (include/KeyFrame.h).  tests/standin lacks GetInvSigma2 and GetCalibrationMatrix, so this directory has its own, over tests/standin/cvmini.h.
#pragma once
#include <cstddef>
#include <vector>

#include "cvmini.h"

namespace ORB_SLAM {

class MapPoint;

class KeyFrame {
public:
    long unsigned int mnId = 0;
    cv::Mat mK = cv::Mat(3, 3, CV_32F), Tcw = cv::Mat(4, 4, CV_32F);
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2, mvInvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;

    cv::Mat GetCalibrationMatrix() const { return mK.clone(); }
    // KeyFrame.cc:114-124: Tcw.rowRange(0,3).colRange(0,3) and .col(3)
    cv::Mat GetRotation() const {
        cv::Mat R(3, 3, CV_32F);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R.at<float>(r, c) = Tcw.at<float>(r, c);
        return R;
    }
    cv::Mat GetTranslation() const {
        cv::Mat t(3, 1, CV_32F);
        for (int r = 0; r < 3; r++) t.at<float>(r) = Tcw.at<float>(r, 3);
        return t;
    }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    cv::KeyPoint GetKeyPointUn(const size_t& idx) const { return mvKeysUn[idx]; }
    float GetSigma2(int nLevel) const { return mvLevelSigma2[nLevel]; }
    float GetInvSigma2(int nLevel) const { return mvInvLevelSigma2[nLevel]; }
};

}  // namespace ORB_SLAM
