// Stand-in ORB_SLAM::KeyFrame: the accessors of the reference's include/KeyFrame.h that NewMapPoints.cc calls.
#pragma once
#include <cstddef>
#include <vector>

#include "cvmini.h"

namespace ORB_SLAM {

class KeyFrame {
public:
    cv::Mat GetRotation() { return mRcw.clone(); }
    cv::Mat GetTranslation() { return mtcw.clone(); }
    cv::Mat GetCameraCenter() { return mOw.clone(); }
    float GetScaleFactor(int nLevel = 1) const { return mvScaleFactors[nLevel]; }
    std::vector<float> GetScaleFactors() const { return mvScaleFactors; }
    std::vector<float> GetVectorScaleSigma2() const { return mvLevelSigma2; }
    float GetSigma2(int nLevel = 1) const { return mvLevelSigma2[nLevel]; }
    int GetScaleLevels() const { return (int)mvScaleFactors.size(); }
    float fx = 0, fy = 0, cx = 0, cy = 0;

    // set by the harness
    cv::Mat mRcw = cv::Mat(3, 3, CV_32F), mtcw = cv::Mat(3, 1, CV_32F), mOw = cv::Mat(3, 1, CV_32F);
    std::vector<float> mvScaleFactors, mvLevelSigma2;
};

}  // namespace ORB_SLAM
