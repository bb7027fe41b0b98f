// The route tools/bench_refresh.py measures orbp_refresh against: MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors for n map
// points on ONE host core, from host copies of the key frames, in the arithmetic include/orbp.h states (built with -ffp-contract=off); the
// caller then uploads the result with orbp_put.  The median is the reference's: the N x N distances, every row sorted.
//
//   refresh_host(n, pos, obs_off, obs, ref, kf_ow, kf_bad, kf_kps, kf_desc, cap, factors, nlevels, normal, dmin, dmax, desc, best_obs)
// pos[3n], obs_off[n+1], obs pairs {kf, idx}, ref[n]; out: normal[3n], dmin[n], dmax[n], desc[32n] (left alone where every key frame is bad),
// best_obs[n] (-1 there).  The lists are taken as valid: no status is computed.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "orbp.h"

static inline int hamming(const uint8_t* a, const uint8_t* b) {
    uint64_t x[4], y[4];
    std::memcpy(x, a, 32);
    std::memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

extern "C" void refresh_host(int n, const float* pos, const int32_t* obs_off, const int32_t* obs, const int32_t* ref, const float* kf_ow,
                             const uint8_t* kf_bad, const orbx_keypoint* kf_kps, const uint8_t* kf_desc, int cap, const float* factors, int nlevels,
                             float* normal, float* dmin, float* dmax, uint8_t* desc, int32_t* best_obs) {
    std::vector<const uint8_t*> rows;
    std::vector<int> where, dist, sorted;
    for (int p = 0; p < n; p++) {
        const float* P = pos + (size_t)p * 3;
        const int32_t* o = obs + (size_t)obs_off[p] * 2;
        const int N = obs_off[p + 1] - obs_off[p];
        float nrm[3] = {0.0f, 0.0f, 0.0f};
        for (int j = 0; j < N; j++) {
            const float* ow = kf_ow + (size_t)o[j * 2] * 3;
            const float d[3] = {P[0] - ow[0], P[1] - ow[1], P[2] - ow[2]};
            double s2 = 0.0;
            for (int k = 0; k < 3; k++) s2 = s2 + (double)d[k] * (double)d[k];
            const double s = std::sqrt(s2);
            for (int k = 0; k < 3; k++) nrm[k] = nrm[k] + (float)((double)d[k] / s);
        }
        for (int k = 0; k < 3; k++) normal[(size_t)p * 3 + k] = (float)((double)nrm[k] / (double)N);
        const int rkf = o[ref[p] * 2], ridx = o[ref[p] * 2 + 1];
        const float* ow = kf_ow + (size_t)rkf * 3;
        double s2 = 0.0;
        for (int k = 0; k < 3; k++) {
            const double d = (double)(P[k] - ow[k]);
            s2 = s2 + d * d;
        }
        const float dd = (float)std::sqrt(s2);
        const int level = kf_kps[(size_t)rkf * cap + ridx].octave;
        const float sf = factors[1];
        dmin[p] = ((1.0f / sf) * dd) / factors[level];
        dmax[p] = (sf * dd) * factors[nlevels - 1 - level];

        rows.clear();
        where.clear();
        for (int j = 0; j < N; j++)
            if (!kf_bad[o[j * 2]]) {
                rows.push_back(kf_desc + ((size_t)o[j * 2] * cap + o[j * 2 + 1]) * 32);
                where.push_back(j);
            }
        best_obs[p] = -1;
        const int M = (int)rows.size();
        if (M == 0) continue;
        dist.assign((size_t)M * M, 0);
        for (int i = 0; i < M; i++)
            for (int j = i + 1; j < M; j++) dist[(size_t)i * M + j] = dist[(size_t)j * M + i] = hamming(rows[i], rows[j]);
        int best_median = INT32_MAX, best = 0;
        for (int i = 0; i < M; i++) {
            sorted.assign(dist.begin() + (size_t)i * M, dist.begin() + (size_t)(i + 1) * M);
            std::sort(sorted.begin(), sorted.end());
            const int median = sorted[(size_t)(0.5 * (M - 1))];
            if (median < best_median) { best_median = median; best = i; }
        }
        std::memcpy(desc + (size_t)p * 32, rows[best], 32);
        best_obs[p] = where[best];
    }
}
