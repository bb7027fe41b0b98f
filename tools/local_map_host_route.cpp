// The host route tools/bench_local_map.py measures the local-map chain against, on one core: the three walks of Tracking in front of the local-map
// search (reference src/Tracking.cc:764-839, :738-761, and the list building of LocalMapPoints::SearchReferencePointsInFrustum) and the counting half
// of KeyFrame::UpdateConnections (src/KeyFrame.cc:334-363), written here over flat stand-in arrays: a map point is an index with an observation list
// (CSR of key frames), a bad flag and two stamps; a key frame is an index with its mvpMapPoints row, a bad flag, a stamp and a neighbour list.  The
// containers are the reference's: std::map for the counters (keyed by the key frame's index, which stands for its address), a copy of the
// observation map per point, std::vector for the lists, an unordered_map from point to slot as the drop-in keeps.  Flat arrays are kinder to the
// cache than the reference's heap objects behind mutexes: this route is a lower bound on what it replaces.
#include <cstddef>
#include <cstdint>
#include <map>
#include <unordered_map>
#include <vector>

namespace {
std::unordered_map<int64_t, int32_t> g_slot;          // MapPoint* -> slot, as LocalMapPoints::slot_
}  // namespace

extern "C" {

// the point -> slot table of the drop-in (built once, outside the timed region)
void lm_host_slots(const int32_t* mp_slot, int npts) {
    g_slot.clear();
    g_slot.reserve((std::size_t)npts * 2);
    for (int p = 0; p < npts; p++) g_slot[(int64_t)p * 64 + 0x10000] = mp_slot[p];
}

// src/Tracking.cc:764-839 -> the number of local key frames (local[] holds them), *ref the reference key frame
int lm_host_update_keyframes(int nkf, int npts, int cap, const int32_t* kf_mvp, const int32_t* kf_nt, const uint8_t* kf_bad, int64_t* kf_track,
                             const int32_t* kf_neigh, const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* mp_bad, int32_t* frame_mvp, int nfeat,
                             int64_t frame_id, int32_t* local, int32_t* ref) {
    std::map<int32_t, int> keyframeCounter;
    for (int i = 0; i < nfeat; i++) {
        const int p = frame_mvp[i];
        if (p < 0) continue;
        if (!mp_bad[p]) {
            std::map<int32_t, std::size_t> observations;                                  // GetObservations() returns a copy of the map
            for (int j = obs_off[p]; j < obs_off[p + 1]; j++) observations[obs_kf[j]] = (std::size_t)j;
            for (std::map<int32_t, std::size_t>::iterator it = observations.begin(); it != observations.end(); ++it) keyframeCounter[it->first]++;
        } else {
            frame_mvp[i] = -1;
        }
    }
    int max = 0, kfmax = -1;
    std::vector<int32_t> v;
    v.reserve(3 * keyframeCounter.size());
    for (std::map<int32_t, int>::iterator it = keyframeCounter.begin(); it != keyframeCounter.end(); ++it) {
        if (kf_bad[it->first]) continue;
        if (it->second > max) { max = it->second; kfmax = it->first; }
        v.push_back(it->first);
        kf_track[it->first] = frame_id;
    }
    for (std::size_t j = 0, n0 = v.size(); j < n0; j++) {
        if (v.size() > 80) break;
        for (int q = 0; q < 10; q++) {
            const int nb = kf_neigh[(std::size_t)v[j] * 10 + q];
            if (nb < 0) break;
            if (!kf_bad[nb] && kf_track[nb] != frame_id) { v.push_back(nb); kf_track[nb] = frame_id; break; }
        }
    }
    for (std::size_t j = 0; j < v.size(); j++) local[j] = v[j];
    *ref = kfmax;
    return (int)v.size();
}

// src/Tracking.cc:738-761, then the walk of LocalMapPoints::SearchReferencePointsInFrustum that turns the list into slots and skip flags
// -> the number of local points (list[] their slots, skip[] their flags)
int lm_host_update_points(int cap, const int32_t* kf_mvp, const int32_t* kf_nt, const uint8_t* mp_bad, int64_t* mp_track, const int64_t* mp_seen,
                          const int32_t* local, int nlocal, int64_t frame_id, int32_t* list, uint8_t* skip) {
    std::vector<int32_t> pts;
    for (int j = 0; j < nlocal; j++) {
        const int k = local[j];
        const std::vector<int32_t> vpMPs(kf_mvp + (std::size_t)k * cap, kf_mvp + (std::size_t)k * cap + kf_nt[k]);      // GetMapPointMatches() returns a copy
        for (std::size_t i = 0; i < vpMPs.size(); i++) {
            const int p = vpMPs[i];
            if (p < 0) continue;
            if (mp_track[p] == frame_id) continue;
            if (!mp_bad[p]) { pts.push_back(p); mp_track[p] = frame_id; }
        }
    }
    for (std::size_t i = 0; i < pts.size(); i++) {
        const int p = pts[i];
        list[i] = -1;
        skip[i] = 1;
        if (mp_seen[p] == frame_id || mp_bad[p]) continue;
        list[i] = g_slot.find((int64_t)p * 64 + 0x10000)->second;
        skip[i] = 0;
    }
    return (int)pts.size();
}

// src/Tracking.cc:678-694 without IncreaseVisible
void lm_host_seen(int32_t* frame_mvp, int nfeat, const uint8_t* mp_bad, int64_t* mp_seen, int64_t frame_id) {
    for (int i = 0; i < nfeat; i++) {
        const int p = frame_mvp[i];
        if (p < 0) continue;
        if (mp_bad[p]) frame_mvp[i] = -1;
        else mp_seen[p] = frame_id;
    }
}

// src/KeyFrame.cc:334-363 for key frame k -> the number of entries of KFcounter (out_kf / out_n hold them in the map's order)
int lm_host_connection_weights(int cap, const int32_t* kf_mvp, const int32_t* kf_nt, const int32_t* kf_id, const int32_t* obs_off, const int32_t* obs_kf,
                               const uint8_t* mp_bad, int k, int32_t* out_kf, int32_t* out_n) {
    std::map<int32_t, int> KFcounter;
    const std::vector<int32_t> vpMP(kf_mvp + (std::size_t)k * cap, kf_mvp + (std::size_t)k * cap + kf_nt[k]);
    for (std::size_t i = 0; i < vpMP.size(); i++) {
        const int p = vpMP[i];
        if (p < 0 || mp_bad[p]) continue;
        std::map<int32_t, std::size_t> observations;
        for (int j = obs_off[p]; j < obs_off[p + 1]; j++) observations[obs_kf[j]] = (std::size_t)j;
        for (std::map<int32_t, std::size_t>::iterator it = observations.begin(); it != observations.end(); ++it) {
            if (kf_id[it->first] == kf_id[k]) continue;
            KFcounter[it->first]++;
        }
    }
    int n = 0;
    for (std::map<int32_t, int>::iterator it = KFcounter.begin(); it != KFcounter.end(); ++it, ++n) { out_kf[n] = it->first; out_n[n] = it->second; }
    return n;
}

}  // extern "C"
