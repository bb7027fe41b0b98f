// ORB_SLAM::LocalMapPoints: the last-frame and key-frame projection searches (LocalMapPoints.h).  A translation unit of its own because
// it names Frame::mvKeys / mvbOutlier and KeyFrame's accessors, which a build that only wants SearchReferencePointsInFrustum need not have.
#include <algorithm>
#include <cstring>

#include "LocalMapPoints.h"
#include "KeyFrame.h"
#include "orbf.h"
#include "orbs.h"
#include "orbx.h"

namespace ORB_SLAM {

int LocalMapPoints::searchSource(Frame& C, int mode, const std::vector<MapPoint*>& vpSource, const cv::KeyPoint* srcKeys,
                                 const unsigned char* srcDesc, float th, int ORBdist, bool checkOrientation) {
    const int n = (int)vpSource.size();
    list_.assign(std::max(n, 1), -1);
    for (int i = 0; i < n; i++) {
        MapPoint* pMP = vpSource[i];
        if (!pMP || skip_[i]) continue;
        list_[i] = slotOf(pMP);
    }
    flush();
    orbp_view V;
    orbf_bounds b;
    viewOf(C, V, b);
    V.th = th;
    V.mode = mode;
    const int nt = (int)C.mvKeysUn.size();
    claimed_.resize(std::max(nt, 1));
    for (int i = 0; i < nt; i++) claimed_[i] = C.mvpMapPoints[i] ? 1 : 0;
    cell_feat_.resize(std::max(nt, 1));
    t2pos_.assign(std::max(nt, 1), -1);
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint and orbx_keypoint share one layout");
    const orbs_params prm = {ORBS_RULE_BEST, ORBdist, 0.0f, checkOrientation ? 1 : 0};
    int nmatches = 0, nvisible = 0;
    const int qcap = std::max(1, std::min(n, ORBF_MAX_FEATURES));
    const int rc = orbp_track_source(map_, &V, C.mvScaleFactors.data(), C.mnScaleLevels, list_.data(), n, skip_.data(),
                                     reinterpret_cast<const orbx_keypoint*>(srcKeys), srcDesc, 0, &b, &prm,
                                     reinterpret_cast<const orbx_keypoint*>(C.mvKeysUn.data()), C.mDescriptors.ptr<unsigned char>(0), cell_off_.data(),
                                     cell_feat_.data(), claimed_.data(), nt, 0, qcap, t2pos_.data(), nullptr, &nmatches, &nvisible, nullptr);
    if (rc != ORBX_OK) fail("orbp_track_source", rc);
    for (int idx = 0; idx < nt; idx++)
        if (t2pos_[idx] >= 0) C.mvpMapPoints[idx] = vpSource[t2pos_[idx]];         // src/ORBmatcher.cc:1578, :1703
    return nmatches;
}

// src/ORBmatcher.cc:1507-1620
int LocalMapPoints::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, float th, bool checkOrientation) {
    const int n = (int)LastFrame.mvpMapPoints.size();
    skip_.assign(std::max(n, 1), 0);
    for (int i = 0; i < n; i++) skip_[i] = LastFrame.mvbOutlier[i] ? 1 : 0;         // :1526
    // the octave is read from mvKeys and the angle from mvKeysUn (:1544, :1583); undistortion leaves both as they are
    return searchSource(CurrentFrame, ORBP_MODE_LAST_FRAME, LastFrame.mvpMapPoints, LastFrame.mvKeysUn.data(),
                        LastFrame.mDescriptors.ptr<unsigned char>(0), th, ORBS_TH_HIGH, checkOrientation);
}

// src/ORBmatcher.cc:1622-1746
int LocalMapPoints::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound, float th, int ORBdist,
                                       bool checkOrientation) {
    const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
    const std::vector<cv::KeyPoint> keys = pKF->GetKeyPointsUn();
    const int n = (int)vpMPs.size();
    skip_.assign(std::max(n, 1), 0);
    for (int i = 0; i < n; i++) {
        MapPoint* pMP = vpMPs[i];
        skip_[i] = pMP && (pMP->isBad() || sAlreadyFound.count(pMP)) ? 1 : 0;       // :1644
    }
    return searchSource(CurrentFrame, ORBP_MODE_KEYFRAME, vpMPs, keys.data(), nullptr, th, ORBdist, checkOrientation);
}

}  // namespace ORB_SLAM
