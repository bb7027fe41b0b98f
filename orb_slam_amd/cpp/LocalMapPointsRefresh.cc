// ORB_SLAM::LocalMapPoints::Refresh (LocalMapPoints.h): MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors through
// orbp_refresh.  A translation unit of its own because it names MapPoint::GetObservations / GetReferenceKeyFrame and KeyFrame's accessors,
// which a build that only wants the searches need not have.
#include <algorithm>
#include <cstring>
#include <map>

#include "LocalMapPoints.h"
#include "KeyFrame.h"
#include "orbx.h"

namespace ORB_SLAM {

// A store of `rows` key frames of `feats` features.  The old one is dropped whole: every row is uploaded again when it is next needed.
void LocalMapPoints::growKeyFrames(int rows, int feats) {
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint and orbx_keypoint share one layout");
    if (d_kf_kps_) orbx_device_free(device_, d_kf_kps_);
    if (d_kf_desc_) orbx_device_free(device_, d_kf_desc_);
    if (d_kf_cell_off_) orbx_device_free(device_, d_kf_cell_off_);
    if (d_kf_cell_feat_) orbx_device_free(device_, d_kf_cell_feat_);
    d_kf_kps_ = d_kf_desc_ = d_kf_cell_off_ = d_kf_cell_feat_ = nullptr;
    // one row more than the key frames have: the frame of a SearchByBoW call (LocalMapPointsBoW.cc)
    int rc = orbx_device_alloc(device_, (size_t)(rows + 1) * feats * sizeof(orbx_keypoint), &d_kf_kps_);
    if (rc == ORBX_OK) rc = orbx_device_alloc(device_, (size_t)(rows + 1) * feats * 32, &d_kf_desc_);
    // the rows' grids, for Fuse (LocalMapPointsFuse.cc fills them): 12 KiB per row
    if (rc == ORBX_OK) rc = orbx_device_alloc(device_, (size_t)rows * (ORBF_GRID_CELLS + 1) * 4, &d_kf_cell_off_);
    if (rc == ORBX_OK) rc = orbx_device_alloc(device_, (size_t)rows * feats * 4, &d_kf_cell_feat_);
    if (rc != ORBX_OK) fail("orbx_device_alloc (key-frame store)", rc);
    for (int r = rows - 1; r >= kf_rows_; r--) kf_free_.push_back(r);
    kf_owner_.resize(rows, nullptr);
    kf_resident_.assign(rows, 0);
    kf_grid_resident_.assign(rows, 0);
    kf_fv_resident_.assign(rows, 0);
    kf_nfv_.assign(rows, 0);
    kf_nt_.assign(rows, 0);
    kf_rows_ = rows;
    feat_cap_ = feats;
}

int LocalMapPoints::keyFrameRow(KeyFrame* pKF) {
    std::unordered_map<KeyFrame*, int>::iterator it = kf_row_.find(pKF);
    if (it != kf_row_.end()) return it->second;
    if (kf_free_.empty()) growKeyFrames(std::max(16, kf_rows_ * 2), std::max(feat_cap_, 1));
    const int row = kf_free_.back();
    kf_free_.pop_back();
    kf_row_[pKF] = row;
    kf_owner_[row] = pKF;
    kf_resident_[row] = 0;
    kf_grid_resident_[row] = 0;
    kf_fv_resident_[row] = 0;
    return row;
}

void LocalMapPoints::ForgetKeyFrame(KeyFrame* pKF) {
    std::unordered_map<KeyFrame*, int>::iterator it = kf_row_.find(pKF);
    if (it == kf_row_.end()) return;
    kf_owner_[it->second] = nullptr;
    kf_resident_[it->second] = 0;
    kf_grid_resident_[it->second] = 0;
    kf_fv_resident_[it->second] = 0;                                  // its FeatureVector goes with it
    kf_nfv_[it->second] = 0;
    if ((size_t)it->second < kf_oct_up_.size()) kf_oct_up_[it->second] = 0;        // the row's next owner has octaves of its own
    if ((size_t)it->second < kf_col_put_.size() && kf_col_put_[it->second]) {      // its map-point column too (LocalMapPointsLocalMap.cc): the row's count becomes 0
        kf_col_put_[it->second] = 0;
        if (!kf_col_dirty_[it->second]) { kf_col_dirty_[it->second] = 1; col_pending_.push_back(it->second); }
    }
    kf_free_.push_back(it->second);
    kf_row_.erase(it);
}

std::vector<orbp_refreshed> LocalMapPoints::Refresh(const std::vector<MapPoint*>& vpMPs, bool descriptors) {
    const int nAll = (int)vpMPs.size();
    orbp_refreshed none;
    std::memset(&none, 0, sizeof(none));
    none.best_obs = -1; none.best_median = INT32_MAX; none.status = ORBP_REFRESH_SKIPPED;
    std::vector<orbp_refreshed> out(nAll, none);
    // the points of the call: not null, not bad, each once
    std::vector<int> first(nAll, -1);                    // per listed entry: the point of the call whose record it gets
    std::vector<int> entry;                              // per point of the call: its first entry
    std::unordered_map<MapPoint*, int> seen;
    for (int i = 0; i < nAll; i++) {
        MapPoint* pMP = vpMPs[i];
        if (!pMP || pMP->isBad()) continue;              // src/MapPoint.cc:194, :281
        std::unordered_map<MapPoint*, int>::iterator it = seen.find(pMP);
        if (it != seen.end()) { first[i] = it->second; continue; }
        seen[pMP] = first[i] = (int)entry.size();
        entry.push_back(i);
    }
    const int n = (int)entry.size();
    if (n == 0) return out;

    // the observation lists in the map's order, and the key frames they name
    std::vector<int32_t> obs_off(n + 1, 0), obs, ref(n, -1);
    std::vector<KeyFrame*> obs_kf;
    std::vector<float> pos((size_t)n * 3), factors;
    int feats = feat_cap_;
    for (int p = 0; p < n; p++) {
        MapPoint* pMP = vpMPs[entry[p]];
        const cv::Mat P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) pos[(size_t)p * 3 + k] = P.at<float>(k);
        const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
        KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
        int j = 0;
        for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit, ++j) {
            if (mit->first == pRefKF) ref[p] = j;
            obs.push_back(keyFrameRow(mit->first));
            obs.push_back((int32_t)mit->second);
            obs_kf.push_back(mit->first);
        }
        obs_off[p + 1] = obs_off[p] + j;
    }
    // every key frame of the call: camera centre and bad flag go up each time, its features once
    std::vector<KeyFrame*> rows_used;
    {
        std::vector<uint8_t> mark(kf_rows_, 0);
        for (size_t j = 0; j < obs_kf.size(); j++) {
            const int row = obs[j * 2];
            if (!mark[row]) { mark[row] = 1; rows_used.push_back(obs_kf[j]); }
        }
    }
    std::vector<std::vector<cv::KeyPoint> > keys(rows_used.size());           // of the key frames that are not resident, fetched once
    for (size_t k = 0; k < rows_used.size(); k++)
        if (!kf_resident_[kf_row_[rows_used[k]]]) {
            keys[k] = rows_used[k]->GetKeyPointsUn();
            feats = std::max(feats, (int)keys[k].size());
        }
    if (feats > feat_cap_) {                                                  // a wider store: every row of this call goes up again
        growKeyFrames(kf_rows_, feats);
        for (size_t k = 0; k < rows_used.size(); k++)
            if (keys[k].empty()) keys[k] = rows_used[k]->GetKeyPointsUn();
    }
    std::vector<float> kf_ow((size_t)kf_rows_ * 3, 0.f);
    std::vector<uint8_t> kf_bad(kf_rows_, 0);
    for (size_t k = 0; k < rows_used.size(); k++) {
        KeyFrame* pKF = rows_used[k];
        const int row = kf_row_[pKF];
        const cv::Mat Ow = pKF->GetCameraCenter();
        for (int c = 0; c < 3; c++) kf_ow[(size_t)row * 3 + c] = Ow.at<float>(c);
        kf_bad[row] = pKF->isBad() ? 1 : 0;
        if (factors.empty()) factors = pKF->GetScaleFactors();
        if (kf_resident_[row]) continue;
        const cv::Mat D = pKF->GetDescriptors();
        const size_t nf = keys[k].size();
        int rc = ORBX_OK;
        if (nf > 0) {
            // GetDescriptors() hands out a clone: its rows are contiguous
            rc = orbx_device_upload(device_, static_cast<char*>(d_kf_kps_) + (size_t)row * feat_cap_ * sizeof(orbx_keypoint), keys[k].data(), nf * sizeof(orbx_keypoint));
            if (rc == ORBX_OK) rc = orbx_device_upload(device_, static_cast<char*>(d_kf_desc_) + (size_t)row * feat_cap_ * 32, D.ptr<unsigned char>(0), nf * 32);
        }
        if (rc != ORBX_OK) fail("orbx_device_upload (key frame)", rc);
        kf_resident_[row] = 1;
        kf_nt_[row] = (int32_t)nf;
    }

    // slots: what is pending goes up first, then the new points take theirs (a table that has to grow is re-uploaded from the mirror)
    std::vector<int> fresh;                              // points of the call that are not mirrored yet
    for (int p = 0; p < n; p++)
        if (!slot_.count(vpMPs[entry[p]])) fresh.push_back(p);
    if (!descriptors) {
        for (size_t k = 0; k < fresh.size(); k++) Put(vpMPs[entry[fresh[k]]]);     // the descriptor comes from the map point
        fresh.clear();
    }
    while (free_.size() < fresh.size()) grow();
    flush();
    std::vector<int32_t> slots(n);
    for (size_t k = 0; k < fresh.size(); k++) {
        MapPoint* pMP = vpMPs[entry[fresh[k]]];
        const int slot = free_.back();
        free_.pop_back();
        slot_[pMP] = slot;
        owner_[slot] = pMP;
    }
    for (int p = 0; p < n; p++) slots[p] = slot_[vpMPs[entry[p]]];

    std::vector<orbp_refreshed> rec(n);
    const int what = ORBP_REFRESH_NORMAL_DEPTH | (descriptors ? ORBP_REFRESH_DESCRIPTOR : 0);
    if (obs.empty()) obs.resize(2, 0);
    const int rc = orbp_refresh(map_, slots.data(), n, pos.data(), obs_off.data(), obs.data(), ref.data(), nullptr, kf_ow.data(), kf_bad.data(),
                                static_cast<const orbx_keypoint*>(d_kf_kps_), static_cast<const uint8_t*>(d_kf_desc_), 1, kf_rows_, feat_cap_,
                                factors.data(), (int)factors.size(), what, rec.data(), nullptr);
    if (rc != ORBX_OK) fail("orbp_refresh", rc);

    // the mirror, and the slots of new points that could not be evaluated
    std::vector<uint8_t> is_fresh(n, 0);
    for (size_t k = 0; k < fresh.size(); k++) is_fresh[fresh[k]] = 1;
    for (int p = 0; p < n; p++) {
        const orbp_refreshed& r = rec[p];
        MapPoint* pMP = vpMPs[entry[p]];
        const size_t s = (size_t)slots[p];
        if (r.status != ORBP_REFRESH_OK) {
            if (is_fresh[p]) { slot_.erase(pMP); owner_[s] = nullptr; free_.push_back((int32_t)s); }
            continue;
        }
        std::memcpy(&pos_[s * 3], &pos[(size_t)p * 3], 12);
        std::memcpy(&nrm_[s * 3], r.normal, 12);
        dmin_[s] = r.min_dist;
        dmax_[s] = r.max_dist;
        if (descriptors) {
            if (r.best_obs >= 0) {
                const size_t j = (size_t)obs_off[p] + r.best_obs;
                const cv::Mat d = obs_kf[j]->GetDescriptor((size_t)obs[j * 2 + 1]);
                std::memcpy(&desc_[s * 32], d.ptr<unsigned char>(0), 32);
            } else if (is_fresh[p]) {
                std::memset(&desc_[s * 32], 0, 32);
            }
        }
    }
    for (int i = 0; i < nAll; i++)
        if (first[i] >= 0) out[i] = rec[first[i]];
    return out;
}

}  // namespace ORB_SLAM
