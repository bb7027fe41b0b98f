// Stand-in ORB_SLAM::KeyFrame for the local-map harness: what LocalMapPointsRefresh.cc reads of a key frame (it owns the rows of the key-frame
// store) and, under the reference's names (include/KeyFrame.h), what LocalMapPointsLocalMap.cc reads and writes: GetMapPointMatches,
// GetBestCovisibilityKeyFrames (src/KeyFrame.cc:189-197: the first N of the ordered list), isBad, mnId and mnTrackReferenceForFrame.
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
    long unsigned int mnTrackReferenceForFrame = 0;      // src/KeyFrame.cc:32
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    std::vector<cv::KeyPoint> GetKeyPointsUn() const { return mvKeysUn; }
    std::vector<float> GetScaleFactors() { return mvScaleFactors; }
    cv::Mat GetDescriptors() { return mDescriptors.clone(); }
    cv::Mat GetDescriptor(const std::size_t& idx) {
        cv::Mat d(1, 32, CV_8U);
        std::memcpy(d.ptr<unsigned char>(0), mDescriptors.ptr<unsigned char>((int)idx), 32);
        return d;
    }
    std::vector<float> GetVectorScaleSigma2() const { return std::vector<float>(); }     // ORBmatcherAccess.h names these three; nothing here reads them
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    bool isBad() { return mbBad; }
    std::vector<MapPoint*> GetMapPointMatches() { getMatches++; return mvpMapPoints; }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }

    // set by the harness
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    cv::Mat mDescriptors, Ow;
    bool mbBad = false;
    int getMatches = 0;                      // how often the matches were fetched
};

}  // namespace ORB_SLAM
