// The host route tools/bench_cull.py measures orbp_cull against, on one core: LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:524-578)
// with the observation erasure of KeyFrame::SetBadFlag (src/KeyFrame.cc:497-515) and MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:71-122),
// written here over flat stand-in arrays: a key frame is an index with its mvpMapPoints row and its octaves; a map point is an index with a bad flag
// and a std::map from key frame to feature, copied per visit as GetObservations() does.  Flat arrays are kinder to the cache than the reference's
// heap objects behind mutexes: this route is a lower bound on what it replaces.
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace {
struct State {
    int nkf = 0, npts = 0, cap = 0;
    std::vector<int32_t> mvp;                          // nkf * cap, -1 = NULL
    std::vector<uint8_t> oct;
    std::vector<int32_t> nt;
    std::vector<uint8_t> mp_bad, kf_bad;
    std::vector<std::map<int32_t, std::size_t> > obs;  // mObservations, keyed by the key frame's index (which stands for its address)
} g;

void point_set_bad(int p) {
    g.mp_bad[p] = 1;
    std::map<int32_t, std::size_t> obs = g.obs[p];
    g.obs[p].clear();
    for (std::map<int32_t, std::size_t>::iterator it = obs.begin(); it != obs.end(); ++it) g.mvp[(std::size_t)it->first * g.cap + it->second] = -1;
}

void erase_observation(int p, int k) {
    bool bad = false;
    if (g.obs[p].count(k)) {
        g.obs[p].erase(k);
        if (g.obs[p].size() <= 2) bad = true;
    }
    if (bad) point_set_bad(p);
}
}  // namespace

extern "C" {

// the map as the reference holds it (built outside the timed region; a run changes it, so it is built again in front of every run)
void cull_host_prepare(int nkf, int npts, int cap, const int32_t* kf_mvp, const uint8_t* kf_oct, const int32_t* kf_nt) {
    g.nkf = nkf; g.npts = npts; g.cap = cap;
    g.mvp.assign(kf_mvp, kf_mvp + (std::size_t)nkf * cap);
    g.oct.assign(kf_oct, kf_oct + (std::size_t)nkf * cap);
    g.nt.assign(kf_nt, kf_nt + nkf);
    g.mp_bad.assign(npts, 0);
    g.kf_bad.assign(nkf, 0);
    g.obs.assign(npts, std::map<int32_t, std::size_t>());
    for (int k = 0; k < nkf; k++)
        for (int i = 0; i < kf_nt[k]; i++) {
            const int p = kf_mvp[(std::size_t)k * cap + i];
            if (p >= 0) g.obs[p][k] = (std::size_t)i;
        }
}

// src/LocalMapping.cc:531-577 over the candidates -> the number culled
int cull_host_run(const int32_t* cand, int ncand, int32_t* nmps, int32_t* nred, int32_t* cull) {
    int culled = 0;
    for (int c = 0; c < ncand; c++) {
        const int k = cand[c];
        const std::vector<int32_t> vpMapPoints(g.mvp.begin() + (std::size_t)k * g.cap, g.mvp.begin() + (std::size_t)k * g.cap + g.nt[k]);   // GetMapPointMatches() copies
        int nRedundantObservations = 0, nMPs = 0;
        for (std::size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
            const int p = vpMapPoints[i];
            if (p < 0 || g.mp_bad[p]) continue;
            nMPs++;
            if (g.obs[p].size() > 3) {
                const int scaleLevel = g.oct[(std::size_t)k * g.cap + i];
                const std::map<int32_t, std::size_t> observations = g.obs[p];                          // GetObservations() copies
                int nObs = 0;
                for (std::map<int32_t, std::size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; ++mit) {
                    if (mit->first == k) continue;
                    const int scaleLeveli = g.oct[(std::size_t)mit->first * g.cap + mit->second];
                    if (scaleLeveli <= scaleLevel + 1) {
                        nObs++;
                        if (nObs >= 3) break;
                    }
                }
                if (nObs >= 3) nRedundantObservations++;
            }
        }
        nmps[c] = nMPs; nred[c] = nRedundantObservations;
        cull[c] = nRedundantObservations > 0.9 * nMPs ? 1 : 0;
        if (cull[c]) {
            for (int i = 0; i < g.nt[k]; i++) {
                const int p = g.mvp[(std::size_t)k * g.cap + i];
                if (p >= 0) erase_observation(p, k);
            }
            g.kf_bad[k] = 1;
            culled++;
        }
    }
    return culled;
}

}  // extern "C"
