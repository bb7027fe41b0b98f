// ORB_SLAM::LocalMapPoints: see LocalMapPoints.h.  The frame's grid and bounds come through ORBmatcherAccess.h, as in ORBmatcher.cc.
#include "LocalMapPoints.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "KeyFrame.h"
#include "orbf.h"
#include "orbx.h"

#ifndef ORBMATCHER_ACCESS_HEADER
#define ORBMATCHER_ACCESS_HEADER "ORBmatcherAccess.h"
#endif
#include ORBMATCHER_ACCESS_HEADER

namespace ORB_SLAM {

void LocalMapPoints::fail(const char* what, int rc) {
    throw std::runtime_error(std::string("ORB_SLAM::LocalMapPoints: ") + what + " failed with status " + std::to_string(rc));
}

LocalMapPoints::LocalMapPoints(float nnratio, bool refresh_every_call, int capacity, int device)
    : ratio_(nnratio), refresh_(refresh_every_call), capacity_(std::max(capacity, 1)), device_(device) {
    const int rc = orbp_create(capacity_, device_, &map_);
    if (rc != ORBX_OK) fail("orbp_create", rc);
    owner_.assign(capacity_, nullptr);
    dirty_.assign(capacity_, 0); dead_.assign(capacity_, 0);
    pos_.assign((size_t)capacity_ * 3, 0.f); nrm_.assign((size_t)capacity_ * 3, 0.f);
    dmin_.assign(capacity_, 0.f); dmax_.assign(capacity_, 0.f); desc_.assign((size_t)capacity_ * 32, 0);
    for (int s = capacity_ - 1; s >= 0; s--) free_.push_back(s);
}

LocalMapPoints::~LocalMapPoints() {
    orbp_destroy(map_);
    if (d_kf_kps_) orbx_device_free(device_, d_kf_kps_);
    if (d_kf_desc_) orbx_device_free(device_, d_kf_desc_);
    if (d_kf_cell_off_) orbx_device_free(device_, d_kf_cell_off_);
    if (d_kf_cell_feat_) orbx_device_free(device_, d_kf_cell_feat_);
    if (d_kf_fv_node_) orbx_device_free(device_, d_kf_fv_node_);
    if (d_kf_fv_off_) orbx_device_free(device_, d_kf_fv_off_);
    if (d_kf_fv_feat_) orbx_device_free(device_, d_kf_fv_feat_);
    if (d_kf_slot_) orbx_device_free(device_, d_kf_slot_);
    if (d_kf_col_nt_) orbx_device_free(device_, d_kf_col_nt_);
    if (d_kf_oct_) orbx_device_free(device_, d_kf_oct_);
    if (d_local_) orbx_device_free(device_, d_local_);
}

void LocalMapPoints::grow() {
    const int old = capacity_;
    orbp_map* bigger = nullptr;
    const int rc = orbp_create(old * 2, device_, &bigger);
    if (rc != ORBX_OK) fail("orbp_create (growing)", rc);
    orbp_destroy(map_);
    map_ = bigger;
    capacity_ = old * 2;
    owner_.resize(capacity_, nullptr);
    dirty_.resize(capacity_, 0); dead_.assign(capacity_, 0);
    pos_.resize((size_t)capacity_ * 3, 0.f); nrm_.resize((size_t)capacity_ * 3, 0.f);
    dmin_.resize(capacity_, 0.f); dmax_.resize(capacity_, 0.f); desc_.resize((size_t)capacity_ * 32, 0);
    for (int s = capacity_ - 1; s >= old; s--) free_.push_back(s);
    // the new table is empty: every owned slot goes up again from the host copy, nothing is left to erase (the resident columns still forget
    // the slots that died)
    purgeColumns();
    dead_list_.clear();
    for (int s = 0; s < old; s++)
        if (owner_[s] && !dirty_[s]) { dirty_[s] = 1; dirty_list_.push_back(s); }
}

void LocalMapPoints::mirror(int slot, MapPoint* pMP) {
    const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal(), D = pMP->GetDescriptor();
    for (int k = 0; k < 3; k++) { pos_[(size_t)slot * 3 + k] = P.at<float>(k); nrm_[(size_t)slot * 3 + k] = Pn.at<float>(k); }
    dmin_[slot] = pMP->GetMinDistanceInvariance();
    dmax_[slot] = pMP->GetMaxDistanceInvariance();
    std::memcpy(&desc_[(size_t)slot * 32], D.ptr<unsigned char>(0), 32);
    if (!dirty_[slot]) { dirty_[slot] = 1; dirty_list_.push_back(slot); }
}

void LocalMapPoints::Put(MapPoint* pMP) {
    if (!pMP) return;
    std::unordered_map<MapPoint*, int>::iterator it = slot_.find(pMP);
    int slot;
    if (it != slot_.end()) {
        slot = it->second;
    } else {
        if (free_.empty()) grow();
        slot = free_.back();
        free_.pop_back();
        slot_[pMP] = slot;
        owner_[slot] = pMP;
    }
    mirror(slot, pMP);
}

int LocalMapPoints::slotOf(MapPoint* pMP) {
    std::unordered_map<MapPoint*, int>::iterator it = slot_.find(pMP);
    if (it != slot_.end() && !refresh_) return it->second;
    Put(pMP);
    return slot_[pMP];
}

void LocalMapPoints::Forget(MapPoint* pMP) {
    std::unordered_map<MapPoint*, int>::iterator it = slot_.find(pMP);
    if (it == slot_.end()) return;
    const int slot = it->second;
    slot_.erase(it);
    owner_[slot] = nullptr;
    free_.push_back(slot);
    if (!dead_[slot]) { dead_[slot] = 1; dead_list_.push_back(slot); }
}

// The key frames' columns (LocalMapPointsLocalMap.cc) must not name a slot that died: freed and assigned again, it would alias the stale entries.
// Every slot of dead_list_ goes, also one that has an owner again: the columns that name the new owner are uploaded after this.
void LocalMapPoints::purgeColumns() {
    if (!d_kf_slot_ || dead_list_.empty()) return;
    int rc = orbp_rows_purge_device(map_, dead_list_.data(), (int)dead_list_.size(), static_cast<int32_t*>(d_kf_slot_), col_rows_, col_cap_, nullptr);
    if (rc == ORBX_OK) rc = orbx_stream_synchronize(device_, nullptr);
    if (rc != ORBX_OK) fail("orbp_rows_purge_device", rc);
}

// one orbp_erase and one orbp_put for everything that changed since the last search
void LocalMapPoints::flush() {
    purgeColumns();
    std::vector<int32_t> gone;
    for (size_t i = 0; i < dead_list_.size(); i++) {
        const int s = dead_list_[i];
        dead_[s] = 0;
        if (!owner_[s]) gone.push_back(s);           // a slot that was reused since is simply overwritten
    }
    dead_list_.clear();
    if (!gone.empty()) {
        const int rc = orbp_erase(map_, gone.data(), (int)gone.size());
        if (rc != ORBX_OK) fail("orbp_erase", rc);
    }
    std::vector<int32_t> up;
    for (size_t i = 0; i < dirty_list_.size(); i++) {
        const int s = dirty_list_[i];
        dirty_[s] = 0;
        if (owner_[s]) up.push_back(s);
    }
    dirty_list_.clear();
    if (up.empty()) return;
    const size_t n = up.size();
    std::vector<float> p(n * 3), q(n * 3), a(n), b(n);
    std::vector<uint8_t> d(n * 32);
    for (size_t i = 0; i < n; i++) {
        const size_t s = (size_t)up[i];
        std::memcpy(&p[i * 3], &pos_[s * 3], 12); std::memcpy(&q[i * 3], &nrm_[s * 3], 12);
        a[i] = dmin_[s]; b[i] = dmax_[s];
        std::memcpy(&d[i * 32], &desc_[s * 32], 32);
    }
    const int rc = orbp_put(map_, up.data(), (int)n, p.data(), q.data(), a.data(), b.data(), d.data());
    if (rc != ORBX_OK) fail("orbp_put", rc);
}

// the view of F: mRcw, mtcw as UpdatePoseMatrices slices them from mTcw; mOw = -mRcw.t()*mtcw as the product of the negated transpose,
// a float sum per row started from 0; the camera and its bounds; F's grid goes into cell_off_ / cell_feat_
void LocalMapPoints::viewOf(Frame& F, orbp_view& V, orbf_bounds& b) {
    std::memset(&V, 0, sizeof(V));
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) V.Rcw[r * 3 + c] = F.mTcw.at<float>(r, c);
        V.tcw[r] = F.mTcw.at<float>(r, 3);
    }
    for (int r = 0; r < 3; r++) {
        float s = 0.0f;
        for (int k = 0; k < 3; k++) s += -V.Rcw[k * 3 + r] * V.tcw[k];
        V.Ow[r] = s;
    }
    V.fx = Frame::fx; V.fy = Frame::fy; V.cx = Frame::cx; V.cy = Frame::cy;
    orbm_access::GridOf(F, b, cell_off_, cell_feat_);
    V.min_x = b.min_x; V.max_x = b.max_x; V.min_y = b.min_y; V.max_y = b.max_y;
}

int LocalMapPoints::SearchReferencePointsInFrustum(Frame& F, const std::vector<MapPoint*>& vpLocalMapPoints, float th, int* nToMatch) {
    const int n = (int)vpLocalMapPoints.size();
    if (nToMatch) *nToMatch = 0;
    list_.assign(std::max(n, 1), -1);
    skip_.assign(std::max(n, 1), 1);
    for (int i = 0; i < n; i++) {
        MapPoint* pMP = vpLocalMapPoints[i];
        if (pMP->mnLastFrameSeen == F.mnId || pMP->isBad()) continue;             // :704-707
        list_[i] = slotOf(pMP);
        skip_[i] = 0;
    }
    flush();
    orbp_view V;
    orbf_bounds b;
    viewOf(F, V, b);
    V.view_cos_limit = 0.5f;                                                       // :709
    V.th = th;
    V.mode = ORBP_MODE_FRAME;
    const int nt = (int)F.mvKeysUn.size();
    claimed_.resize(std::max(nt, 1));
    for (int i = 0; i < nt; i++) claimed_[i] = F.mvpMapPoints[i] ? 1 : 0;
    cell_feat_.resize(std::max(nt, 1));
    t2slot_.assign(std::max(nt, 1), -1);
    rec_.resize(std::max(n, 1));
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint and orbx_keypoint share one layout");
    int nmatches = 0, nvisible = 0;
    const int qcap = std::max(1, std::min(n, ORBF_MAX_FEATURES));
    const int rc = orbp_track(map_, &V, F.mvScaleFactors.data(), F.mnScaleLevels, list_.data(), n, skip_.data(), &b, ratio_,
                              reinterpret_cast<const orbx_keypoint*>(F.mvKeysUn.data()), F.mDescriptors.ptr<unsigned char>(0),
                              cell_off_.data(), cell_feat_.data(), claimed_.data(), nt, 0, qcap, rec_.data(), t2slot_.data(), &nmatches,
                              &nvisible, nullptr);
    if (rc != ORBX_OK) fail("orbp_track", rc);
    for (int i = 0; i < n; i++) {
        if (skip_[i]) continue;
        MapPoint* pMP = vpLocalMapPoints[i];
        const orbp_record& r = rec_[i];
        pMP->mbTrackInView = r.in_view != 0;                                       // src/Frame.cc:139, :190
        if (!r.in_view) continue;
        pMP->mTrackProjX = r.u;
        pMP->mTrackProjY = r.v;
        pMP->mnTrackScaleLevel = r.level;
        pMP->mTrackViewCos = r.view_cos;
        pMP->IncreaseVisible();                                                    // :711
        if (nToMatch) ++*nToMatch;
    }
    for (int idx = 0; idx < nt; idx++)
        if (t2slot_[idx] >= 0) F.mvpMapPoints[idx] = owner_[t2slot_[idx]];         // src/ORBmatcher.cc:118
    return nmatches;
}

}  // namespace ORB_SLAM
