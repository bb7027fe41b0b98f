// The refresh of map points from their observations on gfx950: MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:273-312) and
// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:185-250) for many points per launch, written into the slots of the map-point
// table (orbp_project.hip) in place.  include/orbp.h is the boundary and states the arithmetic and the statuses; the host side lives next
// to put_locked in orbp_project.hip.
//
// k_refresh: one wave per map point, four waves per workgroup, the point index wave-uniform (the shape of k_distinctive, orbm_match.hip).
//   Phase 1  lanes take the observations 64 at a time: {kf, idx} are loaded and checked, d = P - Ow, the f64 sum of squares, its sqrt and
//            the three f64 divides run side by side.  The reference's float sum over the observations has to be taken in listed order, so
//            the chunk is then accumulated by a wave-uniform serial loop that fetches lane j's three floats: 3 float adds per observation
//            and nothing else is serial.  The distances of the reference key frame follow on every lane alike.
//   Phase 2  the median search of k_distinctive over the observations of key frames that are not bad.  Rows and columns both go by raw
//            tiles of 64 observations: a lane that holds a usable observation is a row, with its descriptor in eight registers; a column tile
//            is compacted by ballot + mbcnt into the wave's 2 KiB of LDS (descriptors in listed order, the bad ones dropped), and the bisection
//            counts over it with wave-uniform LDS reads.  With at most 64 observations, the common case, the tile is staged once; beyond
//            that every bisection step stages the column tiles again, which keeps the LDS fixed whatever the number of observations.
//            The bisection is a second copy of k_distinctive's, not a shared device function: the column fetch differs (LDS tile
//            against a packed global array), and k_distinctive's registers stay as they were because its text is untouched.
//   Phase 3  lane 0 writes the slot's two float4 and the live flag, lanes 0-1 the descriptor's two 16-byte halves, lane 0 the record.
// All stores are plain vector stores and nothing is atomic: one wave owns one slot, and the host has checked that no slot is listed twice.
// A wave touches the LDS of its own tile only, so the kernel has no barrier.
#include <hip/hip_runtime.h>

#include <climits>

#include "orbp.h"
#include "orbp_device.h"
#include "orbp_host.h"

namespace orbp {

constexpr int RF_TPB = 256;
constexpr int RF_WAVES = RF_TPB / 64;

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ void write_record(const Refresh& a, int p, int lane, const float nrm[3], float dmin, float dmax, int best_obs, int best_median,
                                             int status) {
    if (!a.out || lane != 0) return;
    orbp_refreshed r;
    r.normal[0] = nrm[0]; r.normal[1] = nrm[1]; r.normal[2] = nrm[2];
    r.min_dist = dmin; r.max_dist = dmax;
    r.best_obs = best_obs; r.best_median = best_median; r.status = status;
    a.out[p] = r;
}

__global__ __launch_bounds__(RF_TPB) void k_refresh(Refresh a, Factors F) {
    __shared__ uint4 tile[RF_WAVES][64 * 2];                           // per wave: up to 64 descriptors, compacted
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * RF_WAVES + wave));
    if (p >= a.n) return;
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    float dmin = 0.0f, dmax = 0.0f;
    if (a.L.skip && a.L.skip[p]) { write_record(a, p, lane, nrm, dmin, dmax, -1, INT_MAX, ORBP_REFRESH_SKIPPED); return; }
    const int s0 = a.L.obs_off[p];
    const long long Nl = (long long)a.L.obs_off[p + 1] - s0;
    if (Nl <= 0 || Nl > INT_MAX) { write_record(a, p, lane, nrm, dmin, dmax, -1, INT_MAX, ORBP_REFRESH_EMPTY); return; }
    const int N = (int)Nl;
    const int2* obs = reinterpret_cast<const int2*>(a.L.obs) + s0;     // pairs: 8-byte aligned
    const bool want_nd = (a.what & ORBP_REFRESH_NORMAL_DEPTH) != 0, want_desc = (a.what & ORBP_REFRESH_DESCRIPTOR) != 0;
    const int slot = a.slots[p];
    float4* g = reinterpret_cast<float4*>(a.geom) + (size_t)slot * 2;
    const bool was_live = a.live[slot] != 0;
    const float4 g0 = g[0], g1 = g[1];                                 // a free slot's are overwritten whole (both bits are required there)
    float P[3] = {g0.x, g0.y, g0.z};
    if (a.L.pos) { P[0] = a.L.pos[(size_t)p * 3]; P[1] = a.L.pos[(size_t)p * 3 + 1]; P[2] = a.L.pos[(size_t)p * 3 + 2]; }

    // ---- phase 1: the checks of every observation, and the sum of the unit vectors in listed order
    bool bad_index = false;
    int ngood = 0;                                                     // observations of key frames that are not bad
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        float unit[3] = {0.0f, 0.0f, 0.0f};
        bool good = false;
        if (j < N) {
            const int2 o = obs[j];
            if ((unsigned)o.x < (unsigned)a.K.nkf && (unsigned)o.y < (unsigned)a.K.cap) {
                good = !(a.K.bad && a.K.bad[o.x]);
                if (want_nd) {
                    const float* ow = a.K.ow + (size_t)o.x * 3;
                    const float d[3] = {P[0] - ow[0], P[1] - ow[1], P[2] - ow[2]};
                    double s2 = 0.0;
                    for (int k = 0; k < 3; k++) s2 = s2 + (double)d[k] * (double)d[k];
                    const double s = sqrt(s2);
                    for (int k = 0; k < 3; k++) unit[k] = (float)((double)d[k] / s);
                }
            } else {
                bad_index = true;
            }
        }
        ngood += __popcll(__ballot(good));
        if (want_nd) {
            const int cnt = N - j0 < 64 ? N - j0 : 64;                 // uniform
            for (int l = 0; l < cnt; l++)
                for (int k = 0; k < 3; k++) nrm[k] = nrm[k] + __shfl(unit[k], l, 64);
        }
    }
    int r = 0;
    if (want_nd) {
        r = a.L.ref[p];
        if (r < 0 || r >= N) bad_index = true;
    }
    if (__any(bad_index)) {
        nrm[0] = nrm[1] = nrm[2] = 0.0f;
        write_record(a, p, lane, nrm, dmin, dmax, -1, INT_MAX, ORBP_REFRESH_BAD_INDEX);
        return;
    }
    if (want_nd) {
        const int2 o = obs[r];                                         // checked above, with the others
        const int level = a.K.kps[(size_t)o.x * a.K.cap + o.y].octave;
        if (level < 0 || level >= F.n) {
            nrm[0] = nrm[1] = nrm[2] = 0.0f;
            write_record(a, p, lane, nrm, dmin, dmax, -1, INT_MAX, ORBP_REFRESH_BAD_OCTAVE);
            return;
        }
        for (int k = 0; k < 3; k++) nrm[k] = (float)((double)nrm[k] / (double)N);
        const float* ow = a.K.ow + (size_t)o.x * 3;
        double s2 = 0.0;
        for (int k = 0; k < 3; k++) {
            const double d = (double)(P[k] - ow[k]);
            s2 = s2 + d * d;
        }
        const float dist = (float)sqrt(s2);
        const float sf = F.f[1];
        dmin = ((1.0f / sf) * dist) / F.f[level];
        dmax = (sf * dist) * F.f[F.n - 1 - level];
        if (!(finite_f(nrm[0]) && finite_f(nrm[1]) && finite_f(nrm[2]) && finite_f(dmin) && finite_f(dmax))) {
            write_record(a, p, lane, nrm, dmin, dmax, -1, INT_MAX, ORBP_REFRESH_NONFINITE);
            return;
        }
    }

    // ---- phase 2: the descriptor with the least median distance to the others
    int best_obs = -1, best_median = INT_MAX;
    if (want_desc && ngood > 0) {
        const int m = (int)(0.5 * (double)(ngood - 1));                // `vDists[0.5*(N-1)]`
        const uint4* KD = reinterpret_cast<const uint4*>(a.K.desc);
        uint4* T = tile[wave];
        // column tile t0: its usable observations' descriptors into the LDS tile in listed order; returns their number
        auto stage = [&](int t0) -> int {
            const int j = t0 + lane;
            bool good = false;
            size_t f = 0;
            if (j < N) {
                const int2 o = obs[j];
                good = !(a.K.bad && a.K.bad[o.x]);
                f = (size_t)o.x * a.K.cap + o.y;
            }
            const unsigned long long mask = __ballot(good);
            __builtin_amdgcn_wave_barrier();                           // the reads of the previous tile are issued before these writes
            if (good) {
                const int c = orbx::lane_rank(mask);
                T[c * 2] = KD[f * 2];
                T[c * 2 + 1] = KD[f * 2 + 1];
            }
            __builtin_amdgcn_wave_barrier();
            return __popcll(mask);
        };
        const bool one_tile = N <= 64;
        const int c_one = one_tile ? stage(0) : 0;
        unsigned long long bestkey = ~0ull;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;
            bool row = false;
            uint32_t q[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            if (i < N) {
                const int2 o = obs[i];
                row = !(a.K.bad && a.K.bad[o.x]);
                if (row) {
                    const size_t f = (size_t)o.x * a.K.cap + o.y;
                    const uint4 x = KD[f * 2], y = KD[f * 2 + 1];
                    q[0] = x.x; q[1] = x.y; q[2] = x.z; q[3] = x.w; q[4] = y.x; q[5] = y.y; q[6] = y.z; q[7] = y.w;
                }
            }
            if (!__any(row)) continue;
            int lo = 0, hi = 256;                                      // smallest v with #{j : d(i,j) <= v} >= m + 1
            while (__any(lo < hi)) {
                const int mid = (lo + hi) >> 1;
                int cnt = 0;
                for (int t0 = 0; t0 < N; t0 += 64) {
                    const int c = one_tile ? c_one : stage(t0);
                    for (int j = 0; j < c; j++) {
                        const uint4 x = T[j * 2], y = T[j * 2 + 1];    // wave-uniform address: one LDS broadcast each
                        const uint32_t d = __popc(q[0] ^ x.x) + __popc(q[1] ^ x.y) + __popc(q[2] ^ x.z) + __popc(q[3] ^ x.w) + __popc(q[4] ^ y.x) +
                                           __popc(q[5] ^ y.y) + __popc(q[6] ^ y.z) + __popc(q[7] ^ y.w);
                        cnt += (int)d <= mid;
                    }
                }
                if (lo < hi) { if (cnt >= m + 1) hi = mid; else lo = mid + 1; }
            }
            if (row) {
                const unsigned long long key = ((unsigned long long)(uint32_t)lo << 32) | (uint32_t)i;
                bestkey = key < bestkey ? key : bestkey;
            }
        }
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long o = (unsigned long long)__shfl_xor((long long)bestkey, s, 64);
            bestkey = o < bestkey ? o : bestkey;
        }
        best_obs = (int)(uint32_t)bestkey;
        best_median = (int)(bestkey >> 32);
    }

    // ---- phase 3: the slot
    if (want_desc && lane < 2) {
        uint4* td = reinterpret_cast<uint4*>(a.tdesc) + (size_t)slot * 2;
        if (best_obs >= 0) {
            const int2 o = obs[best_obs];
            td[lane] = reinterpret_cast<const uint4*>(a.K.desc)[((size_t)o.x * a.K.cap + o.y) * 2 + lane];
        } else if (!was_live) {
            td[lane] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (lane == 0) {
        float4 n0 = g0, n1 = g1;
        n0.x = P[0]; n0.y = P[1]; n0.z = P[2];
        if (want_nd) { n0.w = nrm[0]; n1.x = nrm[1]; n1.y = nrm[2]; n1.z = dmin; n1.w = dmax; }
        g[0] = n0;
        g[1] = n1;
        a.live[slot] = 1;
    }
    write_record(a, p, lane, nrm, dmin, dmax, best_obs, best_median, ORBP_REFRESH_OK);
}

hipError_t launch_refresh(const Refresh& a, const Factors& F, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    k_refresh<<<(a.n + RF_WAVES - 1) / RF_WAVES, RF_TPB, 0, st>>>(a, F);
    return hipGetLastError();
}

}  // namespace orbp
