// Device code shared between kernels.  Ordered compaction inside one workgroup, used by the map-point walk (orbp_project.hip) and the
// triangulation's list of accepted matches (orbt_triangulate.hip): survivors keep the order of their threads, without atomics.  And the
// per-entry arithmetic of a map point seen from a view: the pieces the walk (k_project) shares with the flat kernels, and the one statement of
// the five tests of ORBP_MODE_FUSE / ORBP_MODE_LOOP (entry_test), which k_fuse (orbp_fuse.hip) and k_loop_test (orbp_loop.hip) both call; beside
// it the tests of ORBP_MODE_SIM3 (entry_test_sim3, k_sim3 of orbp_sim3.hip) over the same pieces, and the one statement of the window scan
// (scan_window), which k_fuse and k_sim3 both call.
#pragma once
#include <hip/hip_runtime.h>

#include "orbf_math.h"
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
// `views`: orbp_view, or the direction records of ORBP_MODE_SIM3 (orbp_sim3_dir).
template <class View>
__device__ __forceinline__ void stage_view(View& V, const View* views, int p) {
    const int tid = threadIdx.x;
    if (tid < (int)(sizeof(View) / 4)) reinterpret_cast<uint32_t*>(&V)[tid] = reinterpret_cast<const uint32_t*>(views + p)[tid];
}

// Rcw * P + tcw as the reference's cv::Mat product evaluates it.  Every operation here and below is a single IEEE operation in the
// reference's order (the build has -ffp-contract=off; `0.0f + x` is not an identity in IEEE arithmetic and is kept).
__device__ __forceinline__ void to_camera(const float R[9], const float t[3], const float P[3], float Pc[3]) {
    for (int r = 0; r < 3; r++) {
        float s = 0.0f;
        s = s + R[r * 3] * P[0];
        s = s + R[r * 3 + 1] * P[1];
        s = s + R[r * 3 + 2] * P[2];
        Pc[r] = s + t[r];
    }
}
__device__ __forceinline__ void to_camera(const orbp_view& V, const float P[3], float Pc[3]) { to_camera(V.Rcw, V.tcw, P, Pc); }

// std::lower_bound on the ascending table, clipped to the last level
__device__ __forceinline__ int level_of(const Factors& F, float ratio) {
    int lv = 0;
    for (int k = 0; k < F.n; k++) lv += F.f[k] < ratio ? 1 : 0;
    return lv >= F.n ? F.n - 1 : lv;
}

// cv::norm of three floats handed in as doubles: the root of a double sum of squares from 0.0 in index order, as float
__device__ __forceinline__ float norm3(const double d[3]) {
    double s2 = 0.0;
    for (int k = 0; k < 3; k++) s2 = s2 + d[k] * d[k];
    return (float)sqrt(s2);
}

// PO = P - Ow in float, handed on as doubles, and cv::norm(PO)
__device__ __forceinline__ float centre_distance(const orbp_view& V, const float P[3], double PO[3]) {
    for (int k = 0; k < 3; k++) PO[k] = (double)(P[k] - V.Ow[k]);
    return norm3(PO);
}

// The projection of a camera-frame point with z >= 0 and KeyFrame::IsInImage: the float 1 / z, x and y before the focal lengths (NOT the
// association of the frame modes), and the half-open bounds, which a NaN or an infinity fails.  View: orbp_view or orbp_sim3_dir.
template <class View>
__device__ __forceinline__ bool project_in_image(const View& V, const float Pc[3], float& u, float& v) {
    const float invz = 1.0f / Pc[2];
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    u = V.fx * x + V.cx;
    v = V.fy * y + V.cy;
    return u >= (float)V.min_x && u < (float)V.max_x && v >= (float)V.min_y && v < (float)V.max_y;
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
    if (!project_in_image(V, Pc, u, v)) return ORBP_FUSE_IMAGE;
    double PO[3], dot = 0.0;
    const float dist = centre_distance(V, P, PO);
    if (dist < dmin || dist > dmax) return ORBP_FUSE_DISTANCE;
    for (int k = 0; k < 3; k++) dot = dot + PO[k] * (double)Pn[k];
    if (dot < 0.5 * (double)dist) return ORBP_FUSE_ANGLE;
    level = level_of(F, dist / dmin);
    return passed;
}

// The tests of ORBP_MODE_SIM3 for one live slot, one direction (reference src/ORBmatcher.cc:1329-1360 = :1412-1443; include/orbp.h): the source key
// frame's pose, the similarity into the other camera's frame, depth, the image test, and the distance interval on the norm of the CAMERA-FRAME
// point.  No viewing angle: g0.w, g1.x and g1.y (the normal) are not read.  Returns ORBP_FUSE_DEPTH / _IMAGE / _DISTANCE or `passed`; u, v and level as
// entry_test.
__device__ __forceinline__ int entry_test_sim3(const orbp_sim3_dir& D, const Factors& F, const float4 g0, const float4 g1, int passed, float& u, float& v,
                                               int& level) {
    const float P[3] = {g0.x, g0.y, g0.z};
    const float dmin = g1.z, dmax = g1.w;
    float Pa[3], Pb[3];
    to_camera(D.Raw, D.taw, P, Pa);
    to_camera(D.S, D.t, Pa, Pb);
    if (Pb[2] < 0.0f) return ORBP_FUSE_DEPTH;
    if (!project_in_image(D, Pb, u, v)) return ORBP_FUSE_IMAGE;
    const double Pd[3] = {(double)Pb[0], (double)Pb[1], (double)Pb[2]};
    const float dist = norm3(Pd);
    if (dist < dmin || dist > dmax) return ORBP_FUSE_DISTANCE;
    level = level_of(F, dist / dmin);
    return passed;
}

// The window scan of ORBP_MODE_FUSE and ORBP_MODE_SIM3 for one entry: Frame::GetFeaturesInArea(u, v, radius, level - 1, level) over row `fr` of the key
// frames K, and the least Hamming distance to the table's descriptor td (two 16-byte pieces).  The cells of one grid column are neighbours in
// the CSR, so a column is one run cell_off[ix*48 + y0] .. cell_off[ix*48 + y1 + 1] in the reference's order; a strictly smaller distance replaces
// the best, so among equal distances the first feature in that order wins.  best / best_f come in as INT_MAX / -1 and stay so when there is no
// cell window or no feature is kept.
__device__ __forceinline__ void scan_window(const orbf_bounds& b, const FuseFrames& K, int fr, const uint4* td, float u, float v, float radius, int level,
                                            int& best, int& best_f) {
    int x0, x1, y0, y1;
    if (!orbf::window_cells(b, u, v, radius, &x0, &x1, &y0, &y1)) return;
    int nt = K.nt[fr];
    nt = nt < 0 ? 0 : (nt > K.cap ? K.cap : nt);
    const size_t fb = (size_t)fr * K.cap;
    const int32_t* off = K.cell_off + (size_t)fr * (ORBF_GRID_CELLS + 1);
    const int32_t* feat = K.cell_feat + fb;
    const orbx_keypoint* kps = K.kps_un + fb;
    const uint4* kd = reinterpret_cast<const uint4*>(K.desc) + fb * 2;
    const uint4 qa = td[0], qb = td[1];
    const uint32_t q0 = qa.x, q1 = qa.y, q2 = qa.z, q3 = qa.w, q4 = qb.x, q5 = qb.y, q6 = qb.z, q7 = qb.w;
    for (int ix = x0; ix <= x1; ix++) {
        int j = off[ix * ORBF_GRID_ROWS + y0], jend = off[ix * ORBF_GRID_ROWS + y1 + 1];
        j = j < 0 ? 0 : j;                                         // a grid that breaks its contract reads nothing outside the row
        jend = jend > nt ? nt : jend;
        for (; j < jend; j++) {
            const int f = feat[j];
            if ((unsigned)f >= (unsigned)nt) continue;
            const orbx_keypoint kp = kps[f];
            if (fabsf(kp.x - u) > radius || fabsf(kp.y - v) > radius || kp.octave < level - 1 || kp.octave > level) continue;
            const uint4 ca = kd[(size_t)f * 2], cb = kd[(size_t)f * 2 + 1];
            const int d = __popc(q0 ^ ca.x) + __popc(q1 ^ ca.y) + __popc(q2 ^ ca.z) + __popc(q3 ^ ca.w) + __popc(q4 ^ cb.x) + __popc(q5 ^ cb.y) +
                          __popc(q6 ^ cb.z) + __popc(q7 ^ cb.w);
            if (d < best) { best = d; best_f = f; }
        }
    }
}

}  // namespace orbp
