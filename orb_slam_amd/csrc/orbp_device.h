// Ordered compaction inside one workgroup, shared by the map-point walk (orbp_project.hip) and the triangulation's list of accepted
// matches (orbt_triangulate.hip): survivors keep the order of their threads, without atomics.
#pragma once
#include <hip/hip_runtime.h>

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
