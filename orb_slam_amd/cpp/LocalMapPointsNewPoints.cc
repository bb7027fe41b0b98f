// ORB_SLAM::LocalMapPoints::CreateNewMapPoints (LocalMapPoints.h): the neighbour loop of LocalMapping::CreateNewMapPoints (reference
// src/LocalMapping.cc:205-370) between ComputeF12 and `new MapPoint`: ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:852-1014) and the match loop
// (:269-353) for every neighbour, through ONE orbt_new_points_rows over the resident key frames of LocalMapPointsRefresh.cc.  A translation unit of
// its own because it names KeyFrame::GetFeatureVector and the pose accessors; it needs LocalMapPointsBoW.cc (residentForBoW) and what that needs.
#include <algorithm>

#include "LocalMapPoints.h"
#include "KeyFrame.h"
#include "NewMapPoints.h"
#include "NewPointsPacking.h"
#include "orbt.h"
#include "orbx.h"

namespace ORB_SLAM {

namespace {
orbt_camera cameraOf(KeyFrame* pKF) {
    orbt_camera c;
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) c.Rcw[r * 3 + k] = R.at<float>(r, k);
        c.tcw[r] = t.at<float>(r);
        c.Ow[r] = O.at<float>(r);
    }
    c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy;
    return c;
}
}  // namespace

void LocalMapPoints::CreateNewMapPoints(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpNeighKFs, const std::vector<cv::Mat>& vF12,
                                        std::vector<std::vector<NewMapPoint> >& vvNew, bool checkOrientation) {
    const size_t nn = vpNeighKFs.size();
    vvNew.assign(nn, std::vector<NewMapPoint>());
    if (vF12.size() != nn) fail("CreateNewMapPoints (one F12 per neighbour)", ORBX_ERR_ARG);
    std::vector<KeyFrame*> kfs(1, pKF1);                   // the current key frame, then the neighbours searched, each once
    std::vector<size_t> which;                             // per pair: its neighbour
    std::vector<float> F12;
    for (size_t i = 0; i < nn; i++) {
        KeyFrame* pKF2 = vpNeighKFs[i];
        float F[9];
        if (!pKF2 || pKF2->isBad() || std::find(kfs.begin(), kfs.end(), pKF2) != kfs.end() || !PackF12(vF12[i], F)) continue;
        which.push_back(i);
        kfs.push_back(pKF2);
        F12.insert(F12.end(), F, F + 9);
    }
    if (which.empty()) return;
    residentForBoW(kfs, 0);

    const int npairs = (int)which.size(), cap = feat_cap_;
    std::vector<int32_t> pairs(2 * (size_t)npairs);
    std::vector<orbt_pair> poses(npairs);
    std::vector<uint8_t> qvalid(cap), claimed((size_t)npairs * cap);
    PackPointFlags(pKF1->GetMapPointMatches(), false, cap, qvalid.data());                       // `if(pMP1) continue;`
    const orbt_camera c1 = cameraOf(pKF1);
    for (int p = 0; p < npairs; p++) {
        KeyFrame* pKF2 = kfs[p + 1];
        pairs[2 * p] = kf_row_[pKF1];
        pairs[2 * p + 1] = kf_row_[pKF2];
        poses[p].kf1 = c1;
        poses[p].kf2 = cameraOf(pKF2);
        poses[p].scale_factor = pKF1->GetScaleFactor();
        poses[p].reserved = 0;
        PackPointFlags(pKF2->GetMapPointMatches(), true, cap, &claimed[(size_t)p * cap]);         // `if(vbMatched2[idx2] || pMP2) continue;`
    }
    // the level tables: the key frames of one map share their extractor's, so the first neighbour's stand for every neighbour's
    const std::vector<float> f1 = pKF1->GetScaleFactors(), s1 = pKF1->GetVectorScaleSigma2(), f2 = kfs[1]->GetScaleFactors(), s2 = kfs[1]->GetVectorScaleSigma2();
    const int nlevels = (int)std::min(std::min(f1.size(), s1.size()), std::min(f2.size(), s2.size()));

    const size_t nent = (size_t)npairs * cap;
    std::vector<int32_t> q2t(nent), found(npairs), match12(nent), acc_idx(2 * nent), count(npairs), overflow(npairs);
    std::vector<uint8_t> status(nent);
    std::vector<float> x3d(3 * nent), acc_x3d(3 * nent);
    const orbs_params prm = {ORBS_RULE_TRIANGULATION, ORBS_TH_LOW, 0.0f, checkOrientation ? 1 : 0};
    const int rc = orbt_new_points_rows(&prm, pairs.data(), npairs, poses.data(), F12.data(), f1.data(), s1.data(), f2.data(), s2.data(), nlevels,
                                        static_cast<const orbx_keypoint*>(d_kf_kps_), static_cast<const uint8_t*>(d_kf_desc_), kf_nt_.data(),
                                        static_cast<const uint32_t*>(d_kf_fv_node_), static_cast<const int32_t*>(d_kf_fv_off_),
                                        static_cast<const uint32_t*>(d_kf_fv_feat_), kf_nfv_.data(), kf_rows_, cap, 1, qvalid.data(), claimed.data(),
                                        q2t.data(), nullptr, found.data(), status.data(), x3d.data(), nullptr, match12.data(), acc_idx.data(),
                                        acc_x3d.data(), count.data(), overflow.data(), cap, nullptr);
    if (rc != ORBX_OK) fail("orbt_new_points_rows", rc);
    for (int p = 0; p < npairs; p++) {
        std::vector<NewMapPoint>& out = vvNew[which[p]];
        out.resize(count[p]);                              // at most cap: the compacted list holds them all
        for (int k = 0; k < count[p]; k++) {
            const size_t e = (size_t)p * cap + k;
            out[k].idx1 = (size_t)acc_idx[2 * e];
            out[k].idx2 = (size_t)acc_idx[2 * e + 1];
            out[k].x3D = cv::Mat(3, 1, CV_32F);
            for (int i = 0; i < 3; i++) out[k].x3D.at<float>(i) = acc_x3d[3 * e + i];
        }
    }
    // the caller makes a map point of every accepted pair and adds it to both key frames (src/LocalMapping.cc:355-362): their map-point columns
    // are read again at the next local-map call, when that has happened
    columnsChanged(kfs);
}

}  // namespace ORB_SLAM
