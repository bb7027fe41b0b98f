// ORB_SLAM::LocalMapPoints::SearchByBoW (LocalMapPoints.h): both ORBmatcher::SearchByBoW overloads (reference src/ORBmatcher.cc:155-281 and
// :715-850) as Tracking::Relocalisation and LoopClosing::ComputeSim3 call them for every candidate, through ONE orbs_bow_rows_search over the
// resident key frames of LocalMapPointsRefresh.cc.  A translation unit of its own because it names KeyFrame::GetFeatureVector and Frame::mFeatVec,
// which a build that only wants the projection searches need not have; it needs LocalMapPointsRefresh.cc (the key-frame store) and
// LocalMapPointsFuse.cc (residentForFuse) built in.
#include <algorithm>
#include <cstring>

#include "LocalMapPoints.h"
#include "KeyFrame.h"
#include "FeatureVectorCSR.h"
#include "orbs.h"
#include "orbx.h"

namespace ORB_SLAM {

namespace {
// flag[i] = the feature holds a good map point (with `invert`: it does not)
void goodPoints(const std::vector<MapPoint*>& v, uint8_t* flag, bool invert) {
    for (size_t i = 0; i < v.size(); i++) {
        const bool good = v[i] && !v[i]->isBad();
        flag[i] = (good != invert) ? 1 : 0;
    }
}
}  // namespace

// Every listed key frame has its features and its FeatureVector on the device when this returns, and the store is wide enough for a frame of
// frameFeatures features in its extra row.  The FeatureVector arrays follow the store's dimensions: a store that grew drops them whole.
void LocalMapPoints::residentForBoW(const std::vector<KeyFrame*>& kfs, int frameFeatures) {
    for (size_t k = 0; k < kfs.size(); k++) keyFrameRow(kfs[k]);
    if (frameFeatures > feat_cap_) growKeyFrames(kf_rows_, frameFeatures);
    residentForFuse(kfs);
    if (fv_rows_ != kf_rows_ || fv_cap_ != feat_cap_) {
        if (d_kf_fv_node_) orbx_device_free(device_, d_kf_fv_node_);
        if (d_kf_fv_off_) orbx_device_free(device_, d_kf_fv_off_);
        if (d_kf_fv_feat_) orbx_device_free(device_, d_kf_fv_feat_);
        d_kf_fv_node_ = d_kf_fv_off_ = d_kf_fv_feat_ = nullptr;
        fv_rows_ = fv_cap_ = 0;
        const size_t rows = (size_t)kf_rows_ + 1;
        int rc = orbx_device_alloc(device_, rows * feat_cap_ * 4, &d_kf_fv_node_);
        if (rc == ORBX_OK) rc = orbx_device_alloc(device_, rows * (feat_cap_ + 1) * 4, &d_kf_fv_off_);
        if (rc == ORBX_OK) rc = orbx_device_alloc(device_, rows * feat_cap_ * 4, &d_kf_fv_feat_);
        if (rc != ORBX_OK) fail("orbx_device_alloc (FeatureVectors)", rc);
        fv_rows_ = kf_rows_;
        fv_cap_ = feat_cap_;
        kf_fv_resident_.assign(kf_rows_, 0);
        kf_nfv_.assign(kf_rows_, 0);
    }
    std::vector<uint32_t> node(feat_cap_), feat(feat_cap_);
    std::vector<int32_t> off(feat_cap_ + 1);
    for (size_t k = 0; k < kfs.size(); k++) {
        const int row = kf_row_[kfs[k]];
        if (kf_fv_resident_[row]) continue;
        const int nn = PackFeatureVector(kfs[k]->GetFeatureVector(), kf_nt_[row], feat_cap_, node.data(), off.data(), feat.data());
        if (nn < 0) fail("SearchByBoW (a key frame's FeatureVector names features it does not have)", ORBX_ERR_ARG);
        int rc = orbx_device_upload(device_, static_cast<char*>(d_kf_fv_off_) + (size_t)row * (feat_cap_ + 1) * 4, off.data(), (size_t)(nn + 1) * 4);
        if (rc == ORBX_OK && nn > 0) rc = orbx_device_upload(device_, static_cast<char*>(d_kf_fv_node_) + (size_t)row * feat_cap_ * 4, node.data(), (size_t)nn * 4);
        if (rc == ORBX_OK && off[nn] > 0) rc = orbx_device_upload(device_, static_cast<char*>(d_kf_fv_feat_) + (size_t)row * feat_cap_ * 4, feat.data(), (size_t)off[nn] * 4);
        if (rc != ORBX_OK) fail("orbx_device_upload (FeatureVector)", rc);
        kf_fv_resident_[row] = 1;
        kf_nfv_[row] = nn;
    }
}

// pairs of rows over the store and its extra row, which holds frameFeatures features under frameNodes nodes (0, 0: not used by the call)
void LocalMapPoints::searchBoW(const std::vector<int32_t>& pairs, int frameFeatures, int frameNodes, int th, float nnratio, bool checkOrientation,
                               const std::vector<uint8_t>& qvalid, const std::vector<uint8_t>* claimed, std::vector<int32_t>* q2t, std::vector<int32_t>* t2q,
                               std::vector<int32_t>& found) {
    const int npairs = (int)pairs.size() / 2;
    found.assign(npairs, 0);
    if (q2t) q2t->assign((size_t)npairs * feat_cap_, -1);
    if (t2q) t2q->assign((size_t)npairs * feat_cap_, -1);
    std::vector<int32_t> nt(kf_nt_), nfv(kf_nfv_);         // the rows' counts stay on the host: the store's, then the extra row's
    nt.push_back(frameFeatures);
    nfv.push_back(frameNodes);
    const orbs_params prm = {ORBS_RULE_BOW, th, nnratio, checkOrientation ? 1 : 0};
    const int rc = orbs_bow_rows_search(&prm, pairs.data(), npairs, static_cast<const orbx_keypoint*>(d_kf_kps_), static_cast<const uint8_t*>(d_kf_desc_),
                                        nt.data(), static_cast<const uint32_t*>(d_kf_fv_node_), static_cast<const int32_t*>(d_kf_fv_off_),
                                        static_cast<const uint32_t*>(d_kf_fv_feat_), nfv.data(), kf_rows_ + 1, feat_cap_, 1, qvalid.data(),
                                        claimed ? claimed->data() : nullptr, q2t ? q2t->data() : nullptr, t2q ? t2q->data() : nullptr, nullptr, nullptr,
                                        found.data(), nullptr);
    if (rc != ORBX_OK) fail("orbs_bow_rows_search", rc);
}

int LocalMapPoints::SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches, float nnratio, bool checkOrientation) {
    std::vector<std::vector<MapPoint*> > vvp;
    std::vector<int> n;
    SearchByBoW(std::vector<KeyFrame*>(1, pKF), F, vvp, &n, nnratio, checkOrientation);
    vpMapPointMatches = vvp[0];
    return n[0];
}

void LocalMapPoints::SearchByBoW(const std::vector<KeyFrame*>& vpCandidates, Frame& F, std::vector<std::vector<MapPoint*> >& vvpMatches, std::vector<int>* nmatches,
                                 float nnratio, bool checkOrientation) {
    const size_t nc = vpCandidates.size();
    vvpMatches.assign(nc, std::vector<MapPoint*>());
    if (nmatches) nmatches->assign(nc, 0);
    std::vector<KeyFrame*> kfs;                            // the candidates searched, each key frame once
    std::vector<size_t> which;                             // per pair: its candidate
    for (size_t i = 0; i < nc; i++) {
        KeyFrame* pKF = vpCandidates[i];
        if (!pKF || pKF->isBad()) continue;
        which.push_back(i);
        if (std::find(kfs.begin(), kfs.end(), pKF) == kfs.end()) kfs.push_back(pKF);
    }
    if (which.empty()) return;
    const int nF = (int)F.mvKeys.size();
    residentForBoW(kfs, nF);

    // the frame: one extra row, up once per call
    const int frow = kf_rows_;
    std::vector<uint32_t> node(feat_cap_), feat(feat_cap_);
    std::vector<int32_t> off(feat_cap_ + 1);
    const int nn = PackFeatureVector(F.mFeatVec, nF, feat_cap_, node.data(), off.data(), feat.data());
    if (nn < 0) fail("SearchByBoW (the frame's FeatureVector names features it does not have)", ORBX_ERR_ARG);
    int rc = orbx_device_upload(device_, static_cast<char*>(d_kf_fv_off_) + (size_t)frow * (feat_cap_ + 1) * 4, off.data(), (size_t)(nn + 1) * 4);
    if (rc == ORBX_OK && nn > 0) rc = orbx_device_upload(device_, static_cast<char*>(d_kf_fv_node_) + (size_t)frow * feat_cap_ * 4, node.data(), (size_t)nn * 4);
    if (rc == ORBX_OK && off[nn] > 0) rc = orbx_device_upload(device_, static_cast<char*>(d_kf_fv_feat_) + (size_t)frow * feat_cap_ * 4, feat.data(), (size_t)off[nn] * 4);
    if (rc == ORBX_OK && nF > 0) {
        rc = orbx_device_upload(device_, static_cast<char*>(d_kf_kps_) + (size_t)frow * feat_cap_ * sizeof(orbx_keypoint), F.mvKeys.data(), (size_t)nF * sizeof(orbx_keypoint));
        if (rc == ORBX_OK) rc = orbx_device_upload(device_, static_cast<char*>(d_kf_desc_) + (size_t)frow * feat_cap_ * 32, F.mDescriptors.ptr<unsigned char>(0), (size_t)nF * 32);
    }
    if (rc != ORBX_OK) fail("orbx_device_upload (frame)", rc);

    const int npairs = (int)which.size();
    std::vector<int32_t> pairs(2 * (size_t)npairs), t2q, found;
    std::vector<uint8_t> qvalid((size_t)npairs * feat_cap_, 0);
    std::vector<std::vector<MapPoint*> > vpMapPointsKF(npairs);
    for (int p = 0; p < npairs; p++) {
        KeyFrame* pKF = vpCandidates[which[p]];
        pairs[2 * p] = kf_row_[pKF];
        pairs[2 * p + 1] = frow;
        vpMapPointsKF[p] = pKF->GetMapPointMatches();
        vpMapPointsKF[p].resize(std::min(vpMapPointsKF[p].size(), (size_t)feat_cap_));
        goodPoints(vpMapPointsKF[p], &qvalid[(size_t)p * feat_cap_], false);
    }
    searchBoW(pairs, nF, nn, ORBS_TH_LOW, nnratio, checkOrientation, qvalid, nullptr, nullptr, &t2q, found);
    for (int p = 0; p < npairs; p++) {
        std::vector<MapPoint*>& out = vvpMatches[which[p]];
        out.assign(F.mvpMapPoints.size(), static_cast<MapPoint*>(NULL));                 // :159
        for (size_t iF = 0; iF < out.size() && iF < (size_t)nF; iF++) {
            const int32_t iKF = t2q[(size_t)p * feat_cap_ + iF];
            if (iKF >= 0) out[iF] = vpMapPointsKF[p][iKF];                               // :227
        }
        if (nmatches) (*nmatches)[which[p]] = found[p];
    }
}

int LocalMapPoints::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, float nnratio, bool checkOrientation) {
    std::vector<std::vector<MapPoint*> > vvp;
    std::vector<int> n;
    SearchByBoW(pKF1, std::vector<KeyFrame*>(1, pKF2), vvp, &n, nnratio, checkOrientation);
    vpMatches12 = vvp[0];
    return n[0];
}

void LocalMapPoints::SearchByBoW(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpCandidates, std::vector<std::vector<MapPoint*> >& vvpMatches12,
                                 std::vector<int>* nmatches, float nnratio, bool checkOrientation) {
    const size_t nc = vpCandidates.size();
    vvpMatches12.assign(nc, std::vector<MapPoint*>());
    if (nmatches) nmatches->assign(nc, 0);
    std::vector<KeyFrame*> kfs(1, pKF1);
    std::vector<size_t> which;
    for (size_t i = 0; i < nc; i++) {
        KeyFrame* pKF = vpCandidates[i];
        if (!pKF || pKF->isBad()) continue;
        which.push_back(i);
        if (std::find(kfs.begin(), kfs.end(), pKF) == kfs.end()) kfs.push_back(pKF);
    }
    if (which.empty()) return;
    residentForBoW(kfs, 0);

    const int npairs = (int)which.size();
    std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
    const size_t N1 = vpMapPoints1.size();
    std::vector<int32_t> pairs(2 * (size_t)npairs), q2t, found;
    std::vector<uint8_t> qvalid((size_t)npairs * feat_cap_, 0), claimed((size_t)npairs * feat_cap_, 1);
    std::vector<std::vector<MapPoint*> > vpMapPoints2(npairs);
    for (int p = 0; p < npairs; p++) {
        KeyFrame* pKF2 = vpCandidates[which[p]];
        pairs[2 * p] = kf_row_[pKF1];
        pairs[2 * p + 1] = kf_row_[pKF2];
        vpMapPoints2[p] = pKF2->GetMapPointMatches();
        std::vector<MapPoint*> v1(vpMapPoints1.begin(), vpMapPoints1.begin() + std::min(N1, (size_t)feat_cap_));
        goodPoints(v1, &qvalid[(size_t)p * feat_cap_], false);
        std::vector<MapPoint*> v2(vpMapPoints2[p].begin(), vpMapPoints2[p].begin() + std::min(vpMapPoints2[p].size(), (size_t)feat_cap_));
        goodPoints(v2, &claimed[(size_t)p * feat_cap_], true);                           // "pMP2 is NULL or bad": never matched
    }
    searchBoW(pairs, 0, 0, ORBS_TH_LOW - 1, nnratio, checkOrientation, qvalid, &claimed, &q2t, nullptr, found);      // `bestDist1<TH_LOW` (:791)
    for (int p = 0; p < npairs; p++) {
        std::vector<MapPoint*>& out = vvpMatches12[which[p]];
        out.assign(N1, static_cast<MapPoint*>(NULL));                                    // :727
        for (size_t i1 = 0; i1 < N1 && i1 < (size_t)feat_cap_; i1++) {
            const int32_t idx2 = q2t[(size_t)p * feat_cap_ + i1];
            if (idx2 >= 0) out[i1] = vpMapPoints2[p][idx2];                              // :795
        }
        if (nmatches) (*nmatches)[which[p]] = found[p];
    }
}

}  // namespace ORB_SLAM
