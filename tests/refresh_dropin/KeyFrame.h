// Stand-in ORB_SLAM::KeyFrame for the LocalMapPoints::Refresh harness: the accessors of the reference's include/KeyFrame.h that
// LocalMapPointsRefresh.cc and ORBmatcherAccess.h call.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

#include "cvmini.h"

namespace ORB_SLAM {

class KeyFrame {
public:
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::vector<cv::KeyPoint> GetKeyPointsUn() const { getKeys++; return mvKeysUn; }
    std::vector<float> GetVectorScaleSigma2() const { return std::vector<float>(); }
    std::vector<float> GetScaleFactors() { return mvScaleFactors; }
    cv::Mat GetDescriptors() { return mDescriptors.clone(); }
    cv::Mat GetDescriptor(const std::size_t& idx) {
        cv::Mat d(1, 32, CV_8U);
        std::memcpy(d.ptr<unsigned char>(0), mDescriptors.ptr<unsigned char>((int)idx), 32);
        return d;
    }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    bool isBad() { return mbBad; }

    // set by the harness
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    cv::Mat mDescriptors, Ow;
    bool mbBad = false;
    mutable int getKeys = 0;                 // how often the key points were fetched: once per upload
};

}  // namespace ORB_SLAM
