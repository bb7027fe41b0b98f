// Device code shared between kernels.  Ordered compaction inside one workgroup, used by the map-point walk (orbp_project.hip) and the
// triangulation's list of accepted matches (orbt_triangulate.hip): survivors keep the order of their threads, without atomics.  And the
// per-entry arithmetic of a map point seen from a view, used by the walk (k_project) and by the fuse search (orbp_fuse.hip, k_fuse).
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

}  // namespace orbp
