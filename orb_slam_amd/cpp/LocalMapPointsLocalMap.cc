// ORB_SLAM::LocalMapPoints::PutKeyFrame / UpdateReferenceKeyFrames / SearchLocalMap / ConnectionWeights (LocalMapPoints.h): the local map of Tracking
// (reference src/Tracking.cc:738-839, :675-726) and the counting half of KeyFrame::UpdateConnections (src/KeyFrame.cc:334-363) over a map-point
// column per row of the key-frame store (include/orbp.h: orbp_local_votes, orbp_local_points_batch_device, orbp_rows_purge_device).  A translation
// unit of its own because it names KeyFrame::GetMapPointMatches, GetBestCovisibilityKeyFrames and mnTrackReferenceForFrame, which a build that only
// wants the searches need not have; the rows are those of LocalMapPointsRefresh.cc (keyFrameRow, ForgetKeyFrame).
#include <algorithm>
#include <cstring>
#include <map>

#include "LocalMapPoints.h"
#include "KeyFrame.h"
#include "orbf.h"
#include "orbx.h"

namespace ORB_SLAM {

void LocalMapPoints::PutKeyFrame(KeyFrame* pKF) {
    if (!pKF) return;
    const int row = keyFrameRow(pKF);
    if ((int)kf_col_put_.size() < kf_rows_) { kf_col_put_.resize(kf_rows_, 0); kf_col_dirty_.resize(kf_rows_, 0); }
    kf_col_put_[row] = 1;
    if (!kf_col_dirty_[row]) { kf_col_dirty_[row] = 1; col_pending_.push_back(row); }
}

void LocalMapPoints::columnOf(KeyFrame* pKF, std::vector<int32_t>& col) {
    const std::vector<MapPoint*> v = pKF->GetMapPointMatches();
    col.resize(v.size());
    for (size_t i = 0; i < v.size(); i++) col[i] = v[i] && !v[i]->isBad() ? slotOf(v[i]) : -1;
}

// What PutKeyFrame, ForgetKeyFrame and columnsChanged left pending: the columns are read from their key frames (which may Put points), the table is
// flushed (which purges the slots that died from the resident columns, then erases and puts), and the columns go up behind that, so that a column
// never names a slot the table does not hold for the same point.
void LocalMapPoints::syncColumns() {
    std::vector<int> rows(col_pending_.begin(), col_pending_.end());
    col_pending_.clear();
    std::vector<std::vector<int32_t> > cols(rows.size());
    int need_cap = std::max(col_cap_, 1);
    for (size_t j = 0; j < rows.size(); j++) {
        const int r = rows[j];
        kf_col_dirty_[r] = 0;
        if (kf_col_put_[r] && kf_owner_[r]) columnOf(kf_owner_[r], cols[j]);
        need_cap = std::max(need_cap, (int)cols[j].size());
    }
    if (kf_rows_ > col_rows_ || need_cap > col_cap_) {
        // a bigger store, zero-initialised (every count 0); every column that was Put is read and uploaded again
        if (d_kf_slot_) orbx_device_free(device_, d_kf_slot_);
        if (d_kf_col_nt_) orbx_device_free(device_, d_kf_col_nt_);
        if (d_kf_oct_) orbx_device_free(device_, d_kf_oct_);
        d_kf_slot_ = d_kf_col_nt_ = d_kf_oct_ = nullptr;
        col_rows_ = kf_rows_;
        col_cap_ = need_cap > col_cap_ ? std::max(need_cap, 2 * col_cap_) : col_cap_;       // a longer row doubles the stride
        int rc = orbx_device_alloc(device_, (size_t)col_rows_ * col_cap_ * 4, &d_kf_slot_);
        if (rc == ORBX_OK) rc = orbx_device_alloc(device_, (size_t)col_rows_ * 4, &d_kf_col_nt_);
        if (rc == ORBX_OK) rc = orbx_device_alloc(device_, (size_t)col_rows_ * col_cap_, &d_kf_oct_);
        if (rc != ORBX_OK) fail("orbx_device_alloc (map-point columns)", rc);
        kf_col_n_.assign(col_rows_, 0);
        kf_oct_up_.assign(col_rows_, 0);
        std::vector<uint8_t> have(col_rows_, 0);
        for (size_t j = 0; j < rows.size(); j++) have[rows[j]] = 1;
        for (int r = 0; r < (int)kf_col_put_.size(); r++) {
            if (!kf_col_put_[r] || !kf_owner_[r] || have[r]) continue;
            rows.push_back(r);
            cols.push_back(std::vector<int32_t>());
            columnOf(kf_owner_[r], cols.back());
            if ((int)cols.back().size() > col_cap_) fail("map-point columns (a key frame grew while its column was read)", ORBX_ERR_ARG);
        }
    }
    flush();
    for (size_t j = 0; j < rows.size(); j++) {
        const int r = rows[j];
        const int32_t n = (int32_t)cols[j].size();
        int rc = n ? orbx_device_upload(device_, static_cast<int32_t*>(d_kf_slot_) + (size_t)r * col_cap_, cols[j].data(), (size_t)n * 4) : ORBX_OK;
        if (rc == ORBX_OK) rc = orbx_device_upload(device_, static_cast<int32_t*>(d_kf_col_nt_) + r, &n, 4);
        if (rc != ORBX_OK) fail("orbx_device_upload (map-point column)", rc);
        kf_col_n_[r] = n;
        // the octave column beside it: a key frame's octaves never change, so they are read once, when its column first goes up or the store is rebuilt
        if (n == 0 || kf_oct_up_[r] || !kf_owner_[r]) continue;
        const std::vector<cv::KeyPoint> keys = kf_owner_[r]->GetKeyPointsUn();
        std::vector<uint8_t> oct((size_t)n, 0);
        for (size_t i = 0; i < oct.size() && i < keys.size(); i++) oct[i] = (uint8_t)std::min(std::max(keys[i].octave, 0), 255);
        rc = orbx_device_upload(device_, static_cast<uint8_t*>(d_kf_oct_) + (size_t)r * col_cap_, oct.data(), oct.size());
        if (rc != ORBX_OK) fail("orbx_device_upload (octave column)", rc);
        kf_oct_up_[r] = 1;
    }
}

void LocalMapPoints::votesFor(const std::vector<int32_t>& query, const std::vector<int32_t>& nquery, int qcap, std::vector<int32_t>& votes) {
    const int np = (int)nquery.size();
    votes.assign((size_t)np * std::max(col_rows_, 1), 0);
    if (col_rows_ == 0 || np == 0) return;
    const int rc = orbp_local_votes(map_, query.data(), nquery.data(), qcap, np, static_cast<const int32_t*>(d_kf_slot_), static_cast<const int32_t*>(d_kf_col_nt_), 1,
                                    col_rows_, col_cap_, votes.data(), nullptr);
    if (rc != ORBX_OK) fail("orbp_local_votes", rc);
}

void LocalMapPoints::UpdateReferenceKeyFrames(Frame& F, std::vector<KeyFrame*>& vpLocalKeyFrames, KeyFrame*& pReferenceKF) {
    // :768-784 without the observation maps: the slots of the frame's points, one entry per feature
    std::vector<int32_t> query;
    for (size_t i = 0, iend = F.mvpMapPoints.size(); i < iend; i++) {
        MapPoint* pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (!pMP->isBad()) query.push_back(slotOf(pMP));
        else F.mvpMapPoints[i] = NULL;                                            // :781
    }
    syncColumns();
    std::map<KeyFrame*, int> keyframeCounter;                                      // :767, in pointer order as the reference's
    if (!query.empty()) {
        std::vector<int32_t> votes;
        votesFor(query, std::vector<int32_t>(1, (int32_t)query.size()), (int)query.size(), votes);
        for (int r = 0; r < col_rows_; r++)
            if (votes[r] > 0 && kf_owner_[r]) keyframeCounter[kf_owner_[r]] = votes[r];
    }
    int max = 0;                                                                   // :786-790
    KeyFrame* pKFmax = NULL;
    vpLocalKeyFrames.clear();
    vpLocalKeyFrames.reserve(3 * keyframeCounter.size());
    for (std::map<KeyFrame*, int>::iterator it = keyframeCounter.begin(), itEnd = keyframeCounter.end(); it != itEnd; it++) {      // :793-808
        KeyFrame* pKF = it->first;
        if (pKF->isBad()) continue;
        if (it->second > max) {
            max = it->second;
            pKFmax = pKF;
        }
        vpLocalKeyFrames.push_back(it->first);
        pKF->mnTrackReferenceForFrame = F.mnId;
    }
    // :812-836: the reference takes the end of the list once and has room reserved, so it walks the key frames listed so far and adds at most one
    // neighbour for each
    for (size_t j = 0, n0 = vpLocalKeyFrames.size(); j < n0; j++) {
        if (vpLocalKeyFrames.size() > 80) break;                                   // :815
        KeyFrame* pKF = vpLocalKeyFrames[j];
        const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
        for (std::vector<KeyFrame*>::const_iterator itNeighKF = vNeighs.begin(), itEndNeighKF = vNeighs.end(); itNeighKF != itEndNeighKF; itNeighKF++) {
            KeyFrame* pNeighKF = *itNeighKF;
            if (!pNeighKF->isBad()) {
                if (pNeighKF->mnTrackReferenceForFrame != F.mnId) {
                    vpLocalKeyFrames.push_back(pNeighKF);
                    pNeighKF->mnTrackReferenceForFrame = F.mnId;
                    break;
                }
            }
        }
    }
    pReferenceKF = pKFmax;                                                         // :838
}

namespace {
// the block of one SearchLocalMap call: slots at multiples of 256 bytes
struct Carve {
    size_t total = 0;
    size_t add(size_t bytes) {
        const size_t off = total;
        total = (off + std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
        return off;
    }
};
}  // namespace

int LocalMapPoints::SearchLocalMap(Frame& F, const std::vector<KeyFrame*>& vpLocalKeyFrames, float th, std::vector<MapPoint*>* vpLocalMapPoints, int* nToMatch) {
    if (nToMatch) *nToMatch = 0;
    if (vpLocalMapPoints) vpLocalMapPoints->clear();                               // :740
    // :678-694 on the host: a loop over the frame's features only
    const int nt = (int)F.mvKeysUn.size();
    std::vector<int32_t> query;
    for (std::vector<MapPoint*>::iterator vit = F.mvpMapPoints.begin(), vend = F.mvpMapPoints.end(); vit != vend; vit++) {
        MapPoint* pMP = *vit;
        if (!pMP) continue;
        if (pMP->isBad()) {
            *vit = NULL;
        } else {
            pMP->IncreaseVisible();
            pMP->mnLastFrameSeen = F.mnId;
            pMP->mbTrackInView = false;
            query.push_back(slotOf(pMP));
        }
    }
    // :752 with MapPoint::mnTrackReferenceForFrame at its initial 0: frame 0 lists nothing
    if (F.mnId == 0) return 0;
    std::vector<int32_t> rows(vpLocalKeyFrames.size(), -1);
    syncColumns();
    size_t listed = 0;
    for (size_t j = 0; j < rows.size(); j++) {
        std::unordered_map<KeyFrame*, int>::const_iterator it = kf_row_.find(vpLocalKeyFrames[j]);
        if (it == kf_row_.end() || it->second >= col_rows_ || (size_t)it->second >= kf_col_put_.size() || !kf_col_put_[it->second]) continue;      // never Put: lists no points
        rows[j] = it->second;
        listed += (size_t)kf_col_n_[it->second];
    }
    if (rows.empty() || listed == 0) return 0;
    const int lcap = (int)std::max<size_t>(1, std::min(listed, slot_.size())), cap = std::max(nt, 1);
    const int qcap = std::max(1, std::min(lcap, ORBF_MAX_FEATURES)), nq = (int)query.size(), nr = (int)rows.size();

    orbp_view V;
    orbf_bounds b;
    viewOf(F, V, b);
    V.view_cos_limit = 0.5f;                                                       // :709
    V.th = th;
    V.mode = ORBP_MODE_FRAME;
    static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint and orbx_keypoint share one layout");
    // up [view | counts | query | rows | kps | desc | cell_off | cell_feat | claimed], down [result | t2slot | list | rec], device only [skip]
    Carve L;
    const size_t o_view = L.add(sizeof(orbp_view)), o_counts = L.add(12), o_query = L.add((size_t)nq * 4), o_rows = L.add((size_t)nr * 4);
    const size_t o_kps = L.add((size_t)cap * sizeof(orbx_keypoint)), o_desc = L.add((size_t)cap * 32), o_off = L.add((size_t)(ORBF_GRID_CELLS + 1) * 4);
    const size_t o_feat = L.add((size_t)cap * 4), o_claimed = L.add(cap), up = L.total;
    const size_t o_res = L.add(5 * 4), o_t2slot = L.add((size_t)cap * 4), o_list = L.add((size_t)lcap * 4), o_rec = L.add((size_t)lcap * sizeof(orbp_record));
    const size_t down = L.total - up, o_skip = L.add(lcap);
    if (L.total > local_bytes_) {
        if (d_local_) orbx_device_free(device_, d_local_);
        d_local_ = nullptr;
        local_bytes_ = 0;
        size_t want = 1 << 16;
        while (want < L.total) want *= 2;
        const int rc = orbx_device_alloc(device_, want, &d_local_);
        if (rc != ORBX_OK) fail("orbx_device_alloc (local map block)", rc);
        local_bytes_ = want;
    }
    std::vector<uint8_t>& h = local_h_;
    if (h.size() < L.total) h.resize(L.total);
    std::memcpy(&h[o_view], &V, sizeof(V));
    const int32_t counts[3] = {nq, nr, nt};
    std::memcpy(&h[o_counts], counts, sizeof(counts));
    if (nq) std::memcpy(&h[o_query], query.data(), (size_t)nq * 4);
    std::memcpy(&h[o_rows], rows.data(), (size_t)nr * 4);
    if (nt) {
        std::memcpy(&h[o_kps], F.mvKeysUn.data(), (size_t)nt * sizeof(orbx_keypoint));
        std::memcpy(&h[o_desc], F.mDescriptors.ptr<unsigned char>(0), (size_t)nt * 32);
        std::memcpy(&h[o_feat], cell_feat_.data(), std::min(cell_feat_.size(), (size_t)nt) * 4);
        for (int i = 0; i < nt; i++) h[o_claimed + i] = F.mvpMapPoints[i] ? 1 : 0;
    }
    std::memcpy(&h[o_off], cell_off_.data(), (size_t)(ORBF_GRID_CELLS + 1) * 4);
    uint8_t* d = static_cast<uint8_t*>(d_local_);
    int rc = orbx_device_upload(device_, d, h.data(), up);
    if (rc != ORBX_OK) fail("orbx_device_upload (local map block)", rc);
    const int32_t* d_counts = reinterpret_cast<const int32_t*>(d + o_counts);
    int32_t* d_res = reinterpret_cast<int32_t*>(d + o_res);                       // nlist, overflow, nmatches, nq, query overflow
    int32_t* d_list = reinterpret_cast<int32_t*>(d + o_list);
    // the list is built on the device and handed to the search on the same stream (the map's own): it does not visit the host on the way
    rc = orbp_local_points_batch_device(map_, nq ? reinterpret_cast<const int32_t*>(d + o_query) : nullptr, nq ? d_counts : nullptr, std::max(nq, 1), 1,
                                        reinterpret_cast<const int32_t*>(d + o_rows), d_counts + 1, nr, static_cast<const int32_t*>(d_kf_slot_),
                                        static_cast<const int32_t*>(d_kf_col_nt_), col_rows_, col_cap_, d_list, d_res, d + o_skip, d_res + 1, lcap, nullptr);
    if (rc != ORBX_OK) fail("orbp_local_points_batch_device", rc);
    rc = orbp_track_batch_device(map_, reinterpret_cast<const orbp_view*>(d + o_view), 1, F.mvScaleFactors.data(), F.mnScaleLevels, d_list, d_res, lcap, d + o_skip, &b,
                                 ratio_, reinterpret_cast<const orbx_keypoint*>(d + o_kps), d + o_desc, reinterpret_cast<const int32_t*>(d + o_off),
                                 reinterpret_cast<const int32_t*>(d + o_feat), d_counts + 2, cap, d + o_claimed, qcap, reinterpret_cast<orbp_record*>(d + o_rec),
                                 reinterpret_cast<int32_t*>(d + o_t2slot), d_res + 2, d_res + 3, d_res + 4, nullptr);
    if (rc != ORBX_OK) fail("orbp_track_batch_device", rc);
    rc = orbx_device_download(device_, &h[up], d + up, down);                      // the list and the records come down once
    if (rc != ORBX_OK) fail("orbx_device_download (local map block)", rc);
    const int32_t* res = reinterpret_cast<const int32_t*>(&h[o_res]);
    if (res[1] || res[0] > lcap || res[0] < 0) fail("orbp_local_points_batch_device (more points than the table holds)", ORBX_ERR_CAPACITY);
    if (res[4]) fail("orbp_track_batch_device (more visible points than one search takes)", ORBX_ERR_CAPACITY);
    const int n = res[0];
    const int32_t* list = reinterpret_cast<const int32_t*>(&h[o_list]);
    const int32_t* t2slot = reinterpret_cast<const int32_t*>(&h[o_t2slot]);
    const orbp_record* rec = reinterpret_cast<const orbp_record*>(&h[o_rec]);
    if (vpLocalMapPoints) vpLocalMapPoints->reserve(n);
    for (int i = 0; i < n; i++) {
        MapPoint* pMP = owner_[list[i]];
        if (vpLocalMapPoints) vpLocalMapPoints->push_back(pMP);                    // :756
        if (!pMP || pMP->mnLastFrameSeen == F.mnId) continue;                      // :704 (the device's skip flag); a bad point is not live
        const orbp_record& r = rec[i];
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
        if (t2slot[idx] >= 0) F.mvpMapPoints[idx] = owner_[t2slot[idx]];           // src/ORBmatcher.cc:118
    return res[2];
}

void LocalMapPoints::ConnectionWeights(const std::vector<KeyFrame*>& vpKFs, std::vector<std::map<KeyFrame*, int> >& vKFcounter) {
    vKFcounter.assign(vpKFs.size(), std::map<KeyFrame*, int>());
    // the queries: each key frame's own column, read from the key frame (:340-353: NULL and bad points are passed over)
    std::vector<std::vector<int32_t> > cols(vpKFs.size());
    for (size_t k = 0; k < vpKFs.size(); k++)
        if (vpKFs[k]) columnOf(vpKFs[k], cols[k]);
    syncColumns();
    for (size_t k0 = 0; k0 < vpKFs.size(); k0 += ORBP_LOCAL_MAX_PROBLEMS) {
        const int np = (int)std::min<size_t>(ORBP_LOCAL_MAX_PROBLEMS, vpKFs.size() - k0);
        int qcap = 1;
        for (int p = 0; p < np; p++) qcap = std::max(qcap, (int)cols[k0 + p].size());
        std::vector<int32_t> query((size_t)np * qcap, -1), nquery(np), votes;
        for (int p = 0; p < np; p++) {
            nquery[p] = (int32_t)cols[k0 + p].size();
            std::copy(cols[k0 + p].begin(), cols[k0 + p].end(), query.begin() + (size_t)p * qcap);
        }
        votesFor(query, nquery, qcap, votes);
        for (int p = 0; p < np; p++) {
            KeyFrame* pKF = vpKFs[k0 + p];
            if (!pKF) continue;
            for (int r = 0; r < col_rows_; r++) {
                const int v = votes[(size_t)p * col_rows_ + r];
                if (v > 0 && kf_owner_[r] && kf_owner_[r]->mnId != pKF->mnId) vKFcounter[k0 + p][kf_owner_[r]] = v;      // :359-361
            }
        }
    }
}

void LocalMapPoints::ConnectionWeights(KeyFrame* pKF, std::map<KeyFrame*, int>& KFcounter) {
    std::vector<std::map<KeyFrame*, int> > v;
    ConnectionWeights(std::vector<KeyFrame*>(1, pKF), v);
    KFcounter.swap(v[0]);
}

}  // namespace ORB_SLAM
