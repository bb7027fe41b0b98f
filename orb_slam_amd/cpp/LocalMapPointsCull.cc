// ORB_SLAM::LocalMapPoints::KeyFrameCulling (LocalMapPoints.h): LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:524-578) over the slot and
// octave columns of the resident key-frame rows (include/orbp.h: orbp_cull).  The device judges every candidate on the map that the SetBadFlag calls
// of the candidates in front of it leave (src/KeyFrame.cc:497-515, src/MapPoint.cc:71-122); the SetBadFlag calls themselves, with the spanning tree
// and the connections, stay the caller's KeyFrame's.  A translation unit of its own because it names KeyFrame::GetVectorCovisibleKeyFrames,
// SetBadFlag and GetScaleLevels; the columns are those of LocalMapPointsLocalMap.cc (syncColumns), the rows those of LocalMapPointsRefresh.cc.
#include <algorithm>

#include "LocalMapPoints.h"
#include "KeyFrame.h"
#include "orbx.h"

namespace ORB_SLAM {

void LocalMapPoints::KeyFrameCulling(KeyFrame* pCurrentKF, std::vector<KeyFrame*>* vpCulled) {
    if (vpCulled) vpCulled->clear();
    cull_calls_ = 0;
    if (!pCurrentKF) return;
    const std::vector<KeyFrame*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();      // :529
    std::vector<KeyFrame*> pending;
    for (size_t j = 0; j < vpLocalKeyFrames.size(); j++) {
        KeyFrame* pKF = vpLocalKeyFrames[j];
        if (!pKF || pKF->mnId == 0 || pKF->isBad()) continue;                                       // :534; a bad key frame has no column
        std::unordered_map<KeyFrame*, int>::const_iterator it = kf_row_.find(pKF);
        if (it == kf_row_.end() || (size_t)it->second >= kf_col_put_.size() || !kf_col_put_[it->second]) continue;      // never Put
        pending.push_back(pKF);
    }
    while (!pending.empty()) {
        syncColumns();                                               // what is pending goes up, dead slots leave the table and the columns
        const int n = (int)std::min<size_t>(pending.size(), ORBP_CULL_MAX_CANDIDATES);
        std::vector<int32_t> rows(n), nmps(n), nred(n), cull(n);
        for (int c = 0; c < n; c++) rows[c] = kf_row_[pending[c]];
        const int nlevels = std::min(std::max(pending[0]->GetScaleLevels(), 1), ORBS_MAX_LEVELS);
        const int rc = orbp_cull(map_, rows.data(), n, static_cast<const int32_t*>(d_kf_slot_), static_cast<const uint8_t*>(d_kf_oct_),
                                 static_cast<const int32_t*>(d_kf_col_nt_), 1, col_rows_, col_cap_, nlevels, nmps.data(), nred.data(), cull.data(), nullptr);
        if (rc != ORBX_OK) fail("orbp_cull", rc);
        cull_calls_++;
        int done = n;                                                // the candidates this call settled
        for (int c = 0; c < n; c++) {
            if (!cull[c]) continue;
            KeyFrame* pKF = pending[c];
            pKF->SetBadFlag();                                       // :576
            if (!pKF->isBad()) {                                     // mbNotErase: it stays in the map, and the flags behind it assumed it gone
                done = c + 1;
                break;
            }
            // the mirror follows: the row and its column go, and so does every point of the row that went bad with it
            const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
            for (size_t i = 0; i < vpMapPoints.size(); i++)
                if (vpMapPoints[i] && vpMapPoints[i]->isBad()) Forget(vpMapPoints[i]);
            ForgetKeyFrame(pKF);
            if (vpCulled) vpCulled->push_back(pKF);
        }
        pending.erase(pending.begin(), pending.begin() + done);
    }
}

}  // namespace ORB_SLAM
