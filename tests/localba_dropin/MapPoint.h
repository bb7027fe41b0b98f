// Stand-in ORB_SLAM::MapPoint for the BundleAdjuster drop-in harness (include/MapPoint.h): the observations as the reference keeps them, a
// std::map keyed by the key frame's POINTER (the harness allocates the key frames in one array, so the order is their index), and
// EraseObservation / SetBadFlag as src/MapPoint.cc:71-122 has them: bad at two observations or fewer.
#pragma once
#include <cstddef>
#include <map>

#include "KeyFrame.h"
#include "cvmini.h"

namespace ORB_SLAM {

class MapPoint {
public:
    long unsigned int mnId = 0;
    long unsigned int mnBALocalForKF = 0;
    cv::Mat mWorldPos = cv::Mat(3, 1, CV_32F);
    std::map<KeyFrame*, size_t> mObservations;
    KeyFrame* mpRefKF = NULL;
    bool mbBad = false;
    int nUpdateNormalAndDepth = 0, nSetWorldPos = 0;

    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat& Pos) { mWorldPos = Pos.clone(); nSetWorldPos++; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    bool isBad() { return mbBad; }
    void UpdateNormalAndDepth() { nUpdateNormalAndDepth++; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) ? (int)mObservations[pKF] : -1; }
    void EraseObservation(KeyFrame* pKF) {
        bool bBad = false;
        if (mObservations.count(pKF)) {
            mObservations.erase(pKF);
            if (mpRefKF == pKF) mpRefKF = mObservations.begin()->first;
            if (mObservations.size() <= 2) bBad = true;                // If only 2 observations or less, discard point
        }
        if (bBad) SetBadFlag();
    }
    void SetBadFlag() {
        mbBad = true;
        const std::map<KeyFrame*, size_t> obs = mObservations;
        mObservations.clear();
        for (std::map<KeyFrame*, size_t>::const_iterator mit = obs.begin(); mit != obs.end(); mit++) mit->first->EraseMapPointMatch(mit->second);
    }
};

// KeyFrame.cc:225-230
inline void KeyFrame::EraseMapPointMatch(MapPoint* pMP) {
    const int idx = pMP->GetIndexInKeyFrame(this);
    if (idx >= 0) EraseMapPointMatch((size_t)idx);
}

}  // namespace ORB_SLAM
