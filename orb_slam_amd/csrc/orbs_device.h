// Device helpers the search kernels share (orbs_search.hip, orbs_bow_rows.hip, orbs_tri_rows.hip): the wave minimum, lane broadcasts, the Hamming
// distance of two staged descriptors, the rotation bin, ORBmatcher::ComputeThreeMaxima and ORBmatcher::CheckDistEpipolarLine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbs {

constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;
constexpr int HISTO_LENGTH = 30;             // src/ORBmatcher.cc:42

// minimum over the 64 lanes, returned wave-uniform: 4 DPP steps inside each row of 16, then the 4 rows via readlane
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(r0, r1), min(r2, r3));
}

__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ uint4 lane_u4(const uint4& v, int l) {
    uint4 r;
    r.x = (uint32_t)__builtin_amdgcn_readlane((int)v.x, l); r.y = (uint32_t)__builtin_amdgcn_readlane((int)v.y, l);
    r.z = (uint32_t)__builtin_amdgcn_readlane((int)v.z, l); r.w = (uint32_t)__builtin_amdgcn_readlane((int)v.w, l);
    return r;
}

// src/ORBmatcher.cc:234-241 and siblings: rot in [0,360), bin = round(rot/30) (only bins 0..12 are ever hit)
__device__ __forceinline__ int rot_bin(float a1, float a2) {
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0;
    // angles outside [0, 360) (e.g. -1 = "no orientation") or NaN would leave [0, HISTO_LENGTH): the reference asserts here
    // (ROS_ASSERT(bin >= 0 && bin < HISTO_LENGTH)); such a match simply takes no part in the rotation vote (255 = no bin)
    return (unsigned)bin < (unsigned)HISTO_LENGTH ? bin : 255;
}

// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1748-1789) on bin sizes
__host__ __device__ inline void three_maxima(const int* sizes, int L, int& ind1, int& ind2, int& ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; i++) {           // the reference's if / else-if chain as selects (keeps everything in registers)
        const int s = sizes[i];
        const bool g1 = s > max1, g2 = !g1 && s > max2, g3 = !g1 && !g2 && s > max3;
        const int n3 = (g1 || g2) ? max2 : (g3 ? s : max3), j3 = (g1 || g2) ? ind2 : (g3 ? i : ind3);
        const int n2 = g1 ? max1 : (g2 ? s : max2), j2 = g1 ? ind1 : (g2 ? i : ind2);
        max3 = n3; ind3 = j3; max2 = n2; ind2 = j2;
        if (g1) { max1 = s; ind1 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
}

// ORBmatcher::CheckDistEpipolarLine (src/ORBmatcher.cc:136-153) split in two: the query's line l = x1' F12 once per query ...
struct EpiLine { float a, b, c, den; int th; };

__device__ __forceinline__ EpiLine epi_line(float x, float y, const float* F, int th) {
    EpiLine e;          // every product and sum rounded on its own, as the reference's float expressions are (no fma)
    e.a = __fadd_rn(__fadd_rn(__fmul_rn(x, F[0]), __fmul_rn(y, F[3])), F[6]);
    e.b = __fadd_rn(__fadd_rn(__fmul_rn(x, F[1]), __fmul_rn(y, F[4])), F[7]);
    e.c = __fadd_rn(__fadd_rn(__fmul_rn(x, F[2]), __fmul_rn(y, F[5])), F[8]);
    e.den = __fadd_rn(__fmul_rn(e.a, e.a), __fmul_rn(e.b, e.b));
    e.th = th;
    return e;
}
// ... and the distance test per candidate.  thr = the smallest float t with (double)t >= 3.84 * sigma2(octave), so that
// `dsqr < thr` in float IS the reference's `(double)dsqr < 3.84*sigma2` (host: orbs_epipolar_bound()).
__device__ __forceinline__ bool epi_ok(const EpiLine& e, float x2, float y2, float thr) {
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(e.a, x2), __fmul_rn(e.b, y2)), e.c);
    if (e.den == 0.0f) return false;
    const float dsqr = __fdiv_rn(__fmul_rn(num, num), e.den);
    return dsqr < thr;
}
// the entry of the per-octave bound table a key point's octave selects (the table has ORBS_MAX_LEVELS = 16 entries; the octave as the staged
// 16-bit field holds it, so a negative one selects the last entry)
__device__ __forceinline__ int epi_level(int octave) { return (int)min((uint32_t)octave & 0xFFFFu, 15u); }

__device__ __forceinline__ uint32_t hamming_key(const uint4& t0, const uint4& t1, const uint4& q0, const uint4& q1) {
    return __popc(t0.x ^ q0.x) + __popc(t0.y ^ q0.y) + __popc(t0.z ^ q0.z) + __popc(t0.w ^ q0.w) +
           __popc(t1.x ^ q1.x) + __popc(t1.y ^ q1.y) + __popc(t1.z ^ q1.z) + __popc(t1.w ^ q1.w);
}

}  // namespace orbs
