// ORB_SLAM::LocalMapPoints::SearchBySim3 (LocalMapPoints.h): ORBmatcher::SearchBySim3 as LoopClosing::ComputeSim3 calls it (reference
// src/ORBmatcher.cc:1267-1505), through orbp_sim3_search over the map-point table and the resident key frames of LocalMapPointsRefresh.cc.  A
// translation unit of its own because it names KeyFrame::GetMapPointMatches and MapPoint::GetIndexInKeyFrame, which a build that only wants the
// tracking searches need not have; it needs LocalMapPointsRefresh.cc (the key-frame store) and LocalMapPointsFuse.cc (residentForFuse) built in.
#include <algorithm>
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
void floats(const cv::Mat& M, int rows, int cols, float* out) {
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) out[r * cols + c] = cols == 1 ? M.at<float>(r) : M.at<float>(r, c);
}
}  // namespace

int LocalMapPoints::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const cv::Mat& R12, const cv::Mat& t12,
                                 float th) {
    std::vector<int> nFound;
    SearchBySim3(pKF1, std::vector<Sim3Candidate>(1, Sim3Candidate{pKF2, s12, R12, t12, &vpMatches12}), th, &nFound);
    return nFound[0];
}

void LocalMapPoints::SearchBySim3(KeyFrame* pKF1, const std::vector<Sim3Candidate>& vCandidates, float th, std::vector<int>* nFound) {
    const int npairs = (int)vCandidates.size();
    if (nFound) nFound->assign(npairs, 0);
    if (npairs == 0) return;
    const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
    const size_t N1 = vpMapPoints1.size();
    std::vector<std::vector<MapPoint*> > vpMapPoints2(npairs);
    size_t lcap = std::max<size_t>(N1, 1);
    for (int p = 0; p < npairs; p++) {
        vpMapPoints2[p] = vCandidates[p].pKF2->GetMapPointMatches();
        lcap = std::max(lcap, vpMapPoints2[p].size());
        if (vCandidates[p].vpMatches12->size() < N1) fail("SearchBySim3 (vpMatches12 is shorter than key frame 1)", ORBX_ERR_ARG);
    }
    // rows 2p (pKF1's points into pKF2) and 2p + 1 (pKF2's into pKF1); an entry is searched unless lines :1323-1327 / :1406-1410 pass it over
    std::vector<int32_t> list((size_t)2 * npairs * lcap, -1), nlist(2 * npairs), frame(2 * npairs);
    std::vector<uint8_t> skip((size_t)2 * npairs * lcap, 1);
    std::vector<char> already1, already2;
    for (int p = 0; p < npairs; p++) {
        KeyFrame* pKF2 = vCandidates[p].pKF2;
        const std::vector<MapPoint*>& vpMatches12 = *vCandidates[p].vpMatches12;
        const size_t N2 = vpMapPoints2[p].size();
        already1.assign(N1, 0);
        already2.assign(N2, 0);
        for (size_t i = 0; i < N1; i++) {                                        // :1303-1313
            MapPoint* pMP = vpMatches12[i];
            if (!pMP) continue;
            already1[i] = 1;
            const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
            if (idx2 >= 0 && idx2 < (int)N2) already2[idx2] = 1;
        }
        for (int s = 0; s < 2; s++) {
            const std::vector<MapPoint*>& v = s ? vpMapPoints2[p] : vpMapPoints1;
            const std::vector<char>& already = s ? already2 : already1;
            const size_t e = (size_t)(2 * p + s) * lcap;
            nlist[2 * p + s] = (int32_t)v.size();
            for (size_t i = 0; i < v.size(); i++) {
                MapPoint* pMP = v[i];
                if (!pMP || already[i] || pMP->isBad()) continue;
                list[e + i] = slotOf(pMP);
                skip[e + i] = 0;
            }
        }
    }
    flush();                                                                     // a table that grew keeps its slots
    std::vector<KeyFrame*> kfs(1, pKF1);
    for (int p = 0; p < npairs; p++) kfs.push_back(vCandidates[p].pKF2);
    residentForFuse(kfs);

    const orbf_bounds b = orbm_access::CameraBounds();
    std::vector<orbp_sim3_dir> dirs(2 * npairs);
    float R1w[9], t1w[3], R2w[9], t2w[3], R[9], t[3];
    floats(pKF1->GetRotation(), 3, 3, R1w);
    floats(pKF1->GetTranslation(), 3, 1, t1w);
    for (int p = 0; p < npairs; p++) {
        KeyFrame* pKF2 = vCandidates[p].pKF2;
        floats(pKF2->GetRotation(), 3, 3, R2w);
        floats(pKF2->GetTranslation(), 3, 1, t2w);
        floats(vCandidates[p].R12, 3, 3, R);
        floats(vCandidates[p].t12, 3, 1, t);
        // the reference projects into both key frames with pKF1's camera (:1270-1273)
        const int rc = orbp_sim3_from_pair(vCandidates[p].s12, R, t, R1w, t1w, R2w, t2w, pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy, &b, th, &dirs[2 * p]);
        if (rc != ORBX_OK) fail("orbp_sim3_from_pair", rc);
        frame[2 * p] = kf_row_[pKF2];
        frame[2 * p + 1] = kf_row_[pKF1];
    }
    std::vector<int32_t> match12((size_t)npairs * lcap, -1), found(npairs, 0);
    const std::vector<float> factors = pKF1->GetScaleFactors();
    const int rc = orbp_sim3_search(map_, dirs.data(), npairs, factors.data(), pKF1->GetScaleLevels(), list.data(), nlist.data(), (int)lcap, skip.data(), frame.data(),
                                    static_cast<const orbx_keypoint*>(d_kf_kps_), static_cast<const uint8_t*>(d_kf_desc_), static_cast<const int32_t*>(d_kf_cell_off_),
                                    static_cast<const int32_t*>(d_kf_cell_feat_), kf_nt_.data(), kf_rows_, feat_cap_, 1, &b, ORBS_TH_HIGH, nullptr, nullptr, nullptr,
                                    match12.data(), found.data(), nullptr);
    if (rc != ORBX_OK) fail("orbp_sim3_search", rc);
    for (int p = 0; p < npairs; p++) {                                           // :1498
        std::vector<MapPoint*>& vpMatches12 = *vCandidates[p].vpMatches12;
        for (size_t i1 = 0; i1 < N1; i1++) {
            const int32_t idx2 = match12[(size_t)p * lcap + i1];
            if (idx2 >= 0) vpMatches12[i1] = vpMapPoints2[p][idx2];
        }
        if (nFound) (*nFound)[p] = found[p];
    }
}

}  // namespace ORB_SLAM
