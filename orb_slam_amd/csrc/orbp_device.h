// Device code shared between kernels.  Ordered compaction inside one workgroup, used by the map-point walk (orbp_project.hip) and the
// triangulation's list of accepted matches (orbt_triangulate.hip): survivors keep the order of their threads, without atomics.  And the
// per-entry arithmetic of a map point seen from a view: the pieces the walk (k_project) shares with the flat kernels, and the one statement of
// the five tests of ORBP_MODE_FUSE / ORBP_MODE_LOOP (entry_test), which k_fuse (orbp_fuse.hip) and k_loop_test (orbp_loop.hip) both call.
#pragma once
#include <hip/hip_runtime.h>

#include "orbp.h"
#include "orbp_host.h"

namespace orbx {

// the set bits of a wave ballot below this lane
__device__ __forceinline__ int lane_rank(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// One tile of a workgroup of WAVES waves, called by all of its threads: returns `base` + the number of threads before this one whose
// `keep` holds (its place in the output when its own holds) and adds the tile's count to `base`, which stays uniform.  Survivors are
// ranked inside their wave by ballot + mbcnt and the wave totals meet in LDS; two barriers, the second so that the next tile may
// rewrite wave_total.
template <int WAVES>
__device__ __forceinline__ int tile_rank(bool keep, int (&wave_total)[WAVES], int& base) {
    const int wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    int before = base;
    for (int w = 0; w < WAVES; w++) {
        const int c = wave_total[w];
        before += w < wave ? c : 0;
        base += c;
    }
    __syncthreads();
    return before + lane_rank(m);
}

}  // namespace orbx

namespace orbp {

// the length of a list, clamped to [0, lcap]; of view p's list
__device__ __forceinline__ int clamp_count(int n, int lcap) { return n < 0 ? 0 : (n > lcap ? lcap : n); }
__device__ __forceinline__ int clamped_count(const Lists& L, int p) { return clamp_count(L.nlist[p], L.lcap); }

// A workgroup's copy of view p in LDS, called by all of its threads (at least sizeof(orbp_view) / 4 of them); the barrier behind it is the
// caller's.
__device__ __forceinline__ void stage_view(orbp_view& V, const orbp_view* views, int p) {
    const int tid = threadIdx.x;
    if (tid < (int)(sizeof(orbp_view) / 4)) reinterpret_cast<uint32_t*>(&V)[tid] = reinterpret_cast<const uint32_t*>(views + p)[tid];
}

// Rcw * P + tcw as the reference's cv::Mat product evaluates it.  Every operation here and below is a single IEEE operation in the
// reference's order (the build has -ffp-contract=off; `0.0f + x` is not an identity in IEEE arithmetic and is kept).
__device__ __forceinline__ void to_camera(const orbp_view& V, const float P[3], float Pc[3]) {
    for (int r = 0; r < 3; r++) {
        float s = 0.0f;
        s = s + V.Rcw[r * 3] * P[0];
        s = s + V.Rcw[r * 3 + 1] * P[1];
        s = s + V.Rcw[r * 3 + 2] * P[2];
        Pc[r] = s + V.tcw[r];
    }
}

// std::lower_bound on the ascending table, clipped to the last level
__device__ __forceinline__ int level_of(const Factors& F, float ratio) {
    int lv = 0;
    for (int k = 0; k < F.n; k++) lv += F.f[k] < ratio ? 1 : 0;
    return lv >= F.n ? F.n - 1 : lv;
}

// PO = P - Ow in float, handed on as doubles, and cv::norm(PO): the root of a double sum of squares from 0.0 in index order, as float
__device__ __forceinline__ float centre_distance(const orbp_view& V, const float P[3], double PO[3]) {
    for (int k = 0; k < 3; k++) PO[k] = (double)(P[k] - V.Ow[k]);
    double s2 = 0.0;
    for (int k = 0; k < 3; k++) s2 = s2 + PO[k] * PO[k];
    return (float)sqrt(s2);
}

// The five tests of ORBP_MODE_FUSE for one live slot (reference src/ORBmatcher.cc:1040-1113), which ORBP_MODE_LOOP repeats word for word
// (:311-363; include/orbp.h): depth, the float 1 / z, the half-open image test (a NaN fails it), the distance interval, and
// dot < 0.5 * dist in doubles.  Returns the first rejection (ORBP_FUSE_DEPTH / _IMAGE / _DISTANCE / _ANGLE) or `passed`.  The caller
// hands in u = v = 0 and level = 0: u and v are written once they are computed (so they stay zero behind a depth rejection), level only
// when every test passed.  g0, g1: the slot's two 16-byte pieces of geometry.
__device__ __forceinline__ int entry_test(const orbp_view& V, const Factors& F, const float4 g0, const float4 g1, int passed, float& u, float& v,
                                          int& level) {
    const float P[3] = {g0.x, g0.y, g0.z}, Pn[3] = {g0.w, g1.x, g1.y};
    const float dmin = g1.z, dmax = g1.w;
    float Pc[3];
    to_camera(V, P, Pc);
    if (Pc[2] < 0.0f) return ORBP_FUSE_DEPTH;
    const float invz = 1.0f / Pc[2];
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    u = V.fx * x + V.cx;
    v = V.fy * y + V.cy;
    if (!(u >= (float)V.min_x && u < (float)V.max_x && v >= (float)V.min_y && v < (float)V.max_y)) return ORBP_FUSE_IMAGE;
    double PO[3], dot = 0.0;
    const float dist = centre_distance(V, P, PO);
    if (dist < dmin || dist > dmax) return ORBP_FUSE_DISTANCE;
    for (int k = 0; k < 3; k++) dot = dot + PO[k] * (double)Pn[k];
    if (dot < 0.5 * (double)dist) return ORBP_FUSE_ANGLE;
    level = level_of(F, dist / dmin);
    return passed;
}

}  // namespace orbp
