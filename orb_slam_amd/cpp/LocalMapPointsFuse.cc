// ORB_SLAM::LocalMapPoints::Fuse / FuseInNeighbors (LocalMapPoints.h): ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th) as
// LocalMapping::SearchInNeighbors calls it, the search through orbp_fuse over the resident key frames of LocalMapPointsRefresh.cc.  A
// translation unit of its own because it names MapPoint::Replace / AddObservation and KeyFrame::AddMapPoint, which a build that only wants the
// searches need not have; it needs LocalMapPointsRefresh.cc (the key-frame store) built in.
#include <algorithm>
#include <map>
#include <cstring>

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
// the loop of src/ORBmatcher.cc:1033-1131 over a search that is already done: isBad() and IsInKeyFrame() are read as of NOW, because a
// Replace or an AddMapPoint of an earlier iteration (or of an earlier key frame's loop) changes them
// touched: the key frames whose mvpMapPoints this changes (Replace rewrites the match in every key frame that observes the replaced point)
int fuseLoop(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const std::vector<int32_t>& best, std::vector<KeyFrame*>& touched) {
    int nFused = 0;
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
        MapPoint* pMP = vpMapPoints[i];
        if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        const int bestIdx = best[i];
        if (bestIdx < 0) continue;
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
        if (pMPinKF) {
            if (!pMPinKF->isBad()) {
                const std::map<KeyFrame*, size_t> obs = pMP->GetObservations();
                for (std::map<KeyFrame*, size_t>::const_iterator mit = obs.begin(); mit != obs.end(); ++mit) touched.push_back(mit->first);
                pMP->Replace(pMPinKF);
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

// every listed key frame gets a row, and its features and grid are on the device when this returns
void LocalMapPoints::residentForFuse(const std::vector<KeyFrame*>& kfs) {
    for (size_t k = 0; k < kfs.size(); k++) keyFrameRow(kfs[k]);                 // may drop the store: rows first, uploads after
    std::vector<std::vector<cv::KeyPoint> > keys(kfs.size());
    int feats = feat_cap_;
    for (size_t k = 0; k < kfs.size(); k++)
        if (!kf_resident_[kf_row_[kfs[k]]]) {
            keys[k] = kfs[k]->GetKeyPointsUn();
            feats = std::max(feats, (int)keys[k].size());
        }
    if (feats > feat_cap_) {                                                     // a wider store: every row goes up again when it is next needed
        growKeyFrames(kf_rows_, feats);
        for (size_t k = 0; k < kfs.size(); k++)
            if (keys[k].empty()) keys[k] = kfs[k]->GetKeyPointsUn();
    }
    std::vector<int32_t> cell_off, cell_feat;
    orbf_bounds b;
    for (size_t k = 0; k < kfs.size(); k++) {
        KeyFrame* pKF = kfs[k];
        const int row = kf_row_[pKF];
        int rc = ORBX_OK;
        if (!kf_resident_[row]) {
            const cv::Mat D = pKF->GetDescriptors();                             // a clone: its rows are contiguous
            const size_t nf = keys[k].size();
            if (nf > 0) {
                rc = orbx_device_upload(device_, static_cast<char*>(d_kf_kps_) + (size_t)row * feat_cap_ * sizeof(orbx_keypoint), keys[k].data(), nf * sizeof(orbx_keypoint));
                if (rc == ORBX_OK) rc = orbx_device_upload(device_, static_cast<char*>(d_kf_desc_) + (size_t)row * feat_cap_ * 32, D.ptr<unsigned char>(0), nf * 32);
            }
            if (rc != ORBX_OK) fail("orbx_device_upload (key frame)", rc);
            kf_resident_[row] = 1;
            kf_nt_[row] = (int32_t)nf;
        }
        if (!kf_grid_resident_[row]) {
            orbm_access::GridOf(pKF, b, cell_off, cell_feat);
            rc = orbx_device_upload(device_, static_cast<char*>(d_kf_cell_off_) + (size_t)row * (ORBF_GRID_CELLS + 1) * 4, cell_off.data(), cell_off.size() * 4);
            if (rc == ORBX_OK && !cell_feat.empty())
                rc = orbx_device_upload(device_, static_cast<char*>(d_kf_cell_feat_) + (size_t)row * feat_cap_ * 4, cell_feat.data(), cell_feat.size() * 4);
            if (rc != ORBX_OK) fail("orbx_device_upload (key frame grid)", rc);
            kf_grid_resident_[row] = 1;
        }
    }
}

orbp_view LocalMapPoints::keyFrameView(KeyFrame* pKF, const cv::Mat* Scw, const orbf_bounds& b, float th, int mode) {
    orbp_view V;
    std::memset(&V, 0, sizeof(V));
    if (Scw) {
        float S[12];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) S[r * 4 + c] = Scw->at<float>(r, c);
        const int rc = orbp_view_from_sim3(S, &V);
        if (rc != ORBX_OK) fail("orbp_view_from_sim3", rc);
    } else {
        const cv::Mat Rcw = pKF->GetRotation(), tcw = pKF->GetTranslation(), Ow = pKF->GetCameraCenter();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) V.Rcw[r * 3 + c] = Rcw.at<float>(r, c);
            V.tcw[r] = tcw.at<float>(r);
            V.Ow[r] = Ow.at<float>(r);
        }
    }
    V.fx = pKF->fx; V.fy = pKF->fy; V.cx = pKF->cx; V.cy = pKF->cy;
    V.min_x = b.min_x; V.max_x = b.max_x; V.min_y = b.min_y; V.max_y = b.max_y;
    V.th = th;
    V.mode = mode;
    return V;
}

// vScw (loop closing, LocalMapPointsLoop.cc): view p is the decomposition of (*vScw)[p] instead of the key frame's own pose, and a point that is
// in the key frame is searched like any other: that overload passes over the members of pKF->GetMapPoints(), which its caller reads when the
// key frame's turn comes
void LocalMapPoints::searchFuse(const std::vector<KeyFrame*>& targets, const std::vector<const std::vector<MapPoint*>*>& lists, float th,
                                std::vector<std::vector<int32_t> >& best, const std::vector<cv::Mat>* vScw) {
    const int nviews = (int)targets.size();
    best.assign(nviews, std::vector<int32_t>());
    if (nviews == 0) return;
    size_t lcap = 1;
    for (int p = 0; p < nviews; p++) lcap = std::max(lcap, lists[p]->size());
    std::vector<int32_t> list((size_t)nviews * lcap, -1), nlist(nviews), frame(nviews), best_idx((size_t)nviews * lcap, -1), best_dist((size_t)nviews * lcap);
    std::vector<uint8_t> skip((size_t)nviews * lcap, 1);
    for (int p = 0; p < nviews; p++) {
        const std::vector<MapPoint*>& v = *lists[p];
        nlist[p] = (int32_t)v.size();
        for (size_t i = 0; i < v.size(); i++) {
            MapPoint* pMP = v[i];
            // what the loop would pass over already is not searched: both conditions can only turn ON later, and the loop asks again
            if (!pMP || pMP->isBad() || (!vScw && pMP->IsInKeyFrame(targets[p]))) continue;
            list[p * lcap + i] = slotOf(pMP);
            skip[p * lcap + i] = 0;
        }
    }
    flush();                                                                     // a table that grew keeps its slots
    residentForFuse(targets);
    std::vector<orbp_view> views(nviews);
    const orbf_bounds b = orbm_access::CameraBounds();
    for (int p = 0; p < nviews; p++) {
        views[p] = keyFrameView(targets[p], vScw ? &(*vScw)[p] : 0, b, th, ORBP_MODE_FUSE);
        frame[p] = kf_row_[targets[p]];
    }
    const std::vector<float> factors = targets[0]->GetScaleFactors();
    const int rc = orbp_fuse(map_, views.data(), nviews, factors.data(), targets[0]->GetScaleLevels(), list.data(), nlist.data(), (int)lcap, skip.data(), &b,
                             ORBS_TH_LOW, static_cast<const orbx_keypoint*>(d_kf_kps_), static_cast<const uint8_t*>(d_kf_desc_),
                             static_cast<const int32_t*>(d_kf_cell_off_), static_cast<const int32_t*>(d_kf_cell_feat_), kf_nt_.data(), kf_rows_, feat_cap_, 1,
                             frame.data(), best_idx.data(), best_dist.data(), nullptr, nullptr);
    if (rc != ORBX_OK) fail("orbp_fuse", rc);
    for (int p = 0; p < nviews; p++) best[p].assign(best_idx.begin() + p * lcap, best_idx.begin() + p * lcap + nlist[p]);
}

int LocalMapPoints::Fuse(KeyFrame* pKF, std::vector<MapPoint*>& vpMapPoints, float th) {
    std::vector<std::vector<int32_t> > best;
    searchFuse(std::vector<KeyFrame*>(1, pKF), std::vector<const std::vector<MapPoint*>*>(1, &vpMapPoints), th, best);
    std::vector<KeyFrame*> touched;
    const int n = fuseLoop(pKF, vpMapPoints, best[0], touched);
    columnsChanged(touched);
    return n;
}

void LocalMapPoints::FuseInNeighbors(KeyFrame* pCurrent, const std::vector<KeyFrame*>& vpTargetKFs, float th, std::vector<int>* nFused) {
    if (nFused) nFused->clear();
    // src/LocalMapping.cc:398-406: the current key frame's points into every target, searched in one call, fused target by target
    const std::vector<MapPoint*> vpMapPointMatches = pCurrent->GetMapPointMatches();
    std::vector<std::vector<int32_t> > best;
    searchFuse(vpTargetKFs, std::vector<const std::vector<MapPoint*>*>(vpTargetKFs.size(), &vpMapPointMatches), th, best);
    std::vector<KeyFrame*> touched;
    for (size_t k = 0; k < vpTargetKFs.size(); k++) {
        const int n = fuseLoop(vpTargetKFs[k], vpMapPointMatches, best[k], touched);
        if (nFused) nFused->push_back(n);
    }
    columnsChanged(touched);
    // :408-428: the targets' points, each once, as they are after the forward pass
    std::vector<MapPoint*> vpFuseCandidates;
    vpFuseCandidates.reserve(vpTargetKFs.size() * vpMapPointMatches.size());
    for (size_t k = 0; k < vpTargetKFs.size(); k++) {
        const std::vector<MapPoint*> vpMapPointsKFi = vpTargetKFs[k]->GetMapPointMatches();
        for (size_t i = 0; i < vpMapPointsKFi.size(); i++) {
            MapPoint* pMP = vpMapPointsKFi[i];
            if (!pMP) continue;
            if (pMP->isBad() || pMP->mnFuseCandidateForKF == pCurrent->mnId) continue;
            pMP->mnFuseCandidateForKF = pCurrent->mnId;
            vpFuseCandidates.push_back(pMP);
        }
    }
    // :430
    const int n = Fuse(pCurrent, vpFuseCandidates, th);
    if (nFused) nFused->push_back(n);
}

}  // namespace ORB_SLAM
