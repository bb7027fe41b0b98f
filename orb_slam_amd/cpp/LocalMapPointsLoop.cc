// ORB_SLAM::LocalMapPoints::SearchByProjection(pKF, Scw, ...) / SearchAndFuse (LocalMapPoints.h): the two searches LoopClosing makes once a Sim3
// is accepted (reference src/LoopClosing.cc:370 and :557-570), through orbp_loop_search and orbp_fuse over the resident key frames of
// LocalMapPointsRefresh.cc.  A translation unit of its own because it names KeyFrame::GetMapPoints and MapPoint::Replace, which a build that only
// wants the tracking searches need not have; it needs LocalMapPointsRefresh.cc (the key-frame store) and LocalMapPointsFuse.cc (searchFuse) built in.
#include <algorithm>
#include <map>
#include <cstring>
#include <set>

#include "LocalMapPoints.h"
#include "KeyFrame.h"
#include "orbf.h"
#include "orbs.h"
#include "orbx.h"

#ifndef ORBMATCHER_ACCESS_HEADER
#define ORBMATCHER_ACCESS_HEADER "ORBmatcherAccess.h"
#endif
#include ORBMATCHER_ACCESS_HEADER

namespace ORB_SLAM {

namespace {
// src/ORBmatcher.cc:1152-1261 over a search that is already done: the key frame's points are read as its turn begins, isBad() as of each
// iteration, because a Replace of an earlier iteration (or of an earlier key frame's turn) changes both
// touched: the key frames whose mvpMapPoints this changes
int loopFuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpPoints, const std::vector<int32_t>& best, std::vector<KeyFrame*>& touched) {
    const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();
    int nFused = 0;
    for (size_t i = 0; i < vpPoints.size(); i++) {
        MapPoint* pMP = vpPoints[i];
        if (!pMP || pMP->isBad() || spAlreadyFound.count(pMP)) continue;
        const int bestIdx = best[i];
        if (bestIdx < 0) continue;
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
        if (pMPinKF) {
            if (!pMPinKF->isBad()) {
                const std::map<KeyFrame*, size_t> obs = pMPinKF->GetObservations();
                for (std::map<KeyFrame*, size_t>::const_iterator mit = obs.begin(); mit != obs.end(); ++mit) touched.push_back(mit->first);
                pMPinKF->Replace(pMP);
            }
        } else {
            pMP->AddObservation(pKF, bestIdx);
            pKF->AddMapPoint(pMP, bestIdx);
            touched.push_back(pKF);
        }
        nFused++;
    }
    return nFused;
}
}  // namespace

int LocalMapPoints::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th) {
    const int n = (int)vpPoints.size();
    std::set<MapPoint*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase((MapPoint*)0);
    list_.assign(std::max(n, 1), -1);
    skip_.assign(std::max(n, 1), 1);
    for (int i = 0; i < n; i++) {
        MapPoint* pMP = vpPoints[i];
        if (!pMP || pMP->isBad() || spAlreadyFound.count(pMP)) continue;
        list_[i] = slotOf(pMP);
        skip_[i] = 0;
    }
    flush();                                                                     // a table that grew keeps its slots
    residentForFuse(std::vector<KeyFrame*>(1, pKF));
    const int row = kf_row_[pKF], nt = kf_nt_[row];
    if ((int)vpMatched.size() < nt) fail("SearchByProjection (vpMatched is shorter than the key frame)", ORBX_ERR_ARG);

    const orbf_bounds b = orbm_access::CameraBounds();
    const orbp_view V = keyFrameView(pKF, &Scw, b, (float)th, ORBP_MODE_LOOP);

    claimed_.assign(std::max(nt, 1), 0);
    for (int idx = 0; idx < nt; idx++) claimed_[idx] = vpMatched[idx] ? 1 : 0;
    t2pos_.assign(std::max(nt, 1), -1);
    const std::vector<float> factors = pKF->GetScaleFactors();
    int nmatches = 0, nvisible = 0;
    // pKF's row of the store, in place
    const int rc = orbp_loop_search(map_, &V, factors.data(), pKF->GetScaleLevels(), list_.data(), n, skip_.data(), &b, ORBS_TH_LOW,
                                    static_cast<const orbx_keypoint*>(d_kf_kps_) + (size_t)row * feat_cap_, static_cast<const uint8_t*>(d_kf_desc_) + (size_t)row * feat_cap_ * 32,
                                    static_cast<const int32_t*>(d_kf_cell_off_) + (size_t)row * (ORBF_GRID_CELLS + 1), static_cast<const int32_t*>(d_kf_cell_feat_) + (size_t)row * feat_cap_,
                                    claimed_.data(), nt, 1, std::min(std::max(n, 1), ORBF_MAX_FEATURES), nullptr, t2pos_.data(), nullptr, &nmatches, &nvisible, nullptr);
    if (rc != ORBX_OK) fail("orbp_loop_search", rc);
    for (int idx = 0; idx < nt; idx++)
        if (t2pos_[idx] >= 0) vpMatched[idx] = vpPoints[t2pos_[idx]];
    return nmatches;
}

void LocalMapPoints::SearchAndFuse(const std::vector<std::pair<KeyFrame*, cv::Mat> >& vCorrectedScw, const std::vector<MapPoint*>& vpLoopMapPoints, float th,
                                   std::vector<int>* nFused) {
    if (nFused) nFused->clear();
    std::vector<KeyFrame*> targets(vCorrectedScw.size());
    std::vector<cv::Mat> vScw(vCorrectedScw.size());
    for (size_t k = 0; k < vCorrectedScw.size(); k++) {
        targets[k] = vCorrectedScw[k].first;
        vScw[k] = vCorrectedScw[k].second;
    }
    std::vector<std::vector<int32_t> > best;
    searchFuse(targets, std::vector<const std::vector<MapPoint*>*>(targets.size(), &vpLoopMapPoints), th, best, &vScw);
    std::vector<KeyFrame*> touched;
    for (size_t k = 0; k < targets.size(); k++) {
        const int n = loopFuse(targets[k], vpLoopMapPoints, best[k], touched);
        if (nFused) nFused->push_back(n);
    }
    columnsChanged(touched);
}

}  // namespace ORB_SLAM
