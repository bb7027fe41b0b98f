// Triangulation of new map points on gfx950: the match loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:269-353)
// over the matches orbs_triangulation_search_batch_device leaves in HBM.  include/orbt.h is the boundary and states the arithmetic.
//
// Kernel:
//   k_triangulate  one workgroup (eight waves) per key-frame pair, three passes separated by barriers:
//       1. every feature of KF1 gets status ORBT_NONE, match -1 and zero outputs;
//       2. one lane per match entry: the parallax test, the 4 x 4 matrix, its null vector by a cyclic Jacobi iteration on A'A in
//          FP64 (both 4 x 4 matrices stay in registers: every loop is unrolled, no indexed array survives), the six tests; the result
//          goes to the slot of the match's idx1;
//       3. the workgroup walks idx1 in ascending order; accepted features are ranked in that order (orbx::tile_rank) and a survivor
//          writes (idx1, idx2, x3D) at base + rank and updates the two flags: ascending idx1 without atomics.
//   About 60 bytes in and 40 out per match and a few thousand FP64 operations: at 20 pairs of a few hundred matches the launch is
//   bound by its latency (the dependent rotations of one lane), not by the FP64 rate or by HBM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "orb_jacobi.h"
#include "orbp_device.h"
#include "orbt.h"
#include "orbx_host.h"

namespace orbt {

constexpr int TPB = 512;              // one workgroup: eight waves, two per SIMD
constexpr int WAVES = TPB / 64;

struct Levels {
    float f1[ORBS_MAX_LEVELS], s1[ORBS_MAX_LEVELS], f2[ORBS_MAX_LEVELS], s2[ORBS_MAX_LEVELS];
    int n;
};

using orbj::null_vector;              // the 4 x 4 Jacobi iteration, shared with the monocular initialisation (orb_jacobi.h)

// (float)(row r of Rcw . x3D + tcw[r]): the dot as a double sum from 0.0 (cv::Mat::dot), the translation added in double
__device__ __forceinline__ float cam_coord(const orbt_camera& C, int r, const float (&X)[3]) {
    double d = 0.0;
    d = d + (double)C.Rcw[r * 3] * (double)X[0];
    d = d + (double)C.Rcw[r * 3 + 1] * (double)X[1];
    d = d + (double)C.Rcw[r * 3 + 2] * (double)X[2];
    return (float)(d + (double)C.tcw[r]);
}

__device__ __forceinline__ void normalised(const orbt_camera& C, float x, float y, float (&xn)[3], float (&ray)[3]) {
    const float invfx = 1.0f / C.fx, invfy = 1.0f / C.fy;
    xn[0] = (x - C.cx) * invfx;
    xn[1] = (y - C.cy) * invfy;
    xn[2] = 1.0f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float s = 0.0f;
        s = s + C.Rcw[i] * xn[0];
        s = s + C.Rcw[3 + i] * xn[1];
        s = s + C.Rcw[6 + i] * xn[2];
        ray[i] = s;
    }
}

// true when the reprojection of X (camera coordinates z, and x, y computed here) misses the key point by more than the level allows, or is NaN
__device__ __forceinline__ bool reprojection_fails(const orbt_camera& C, const float (&X)[3], float z, float kx, float ky, float sigma2) {
    const float x = cam_coord(C, 0, X), y = cam_coord(C, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = C.fx * x * invz + C.cx, v = C.fy * y * invz + C.cy;
    const float ex = u - kx, ey = v - ky;
    const float e2 = ex * ex + ey * ey;
    return !((double)e2 <= 5.991 * (double)sigma2);
}

__device__ __forceinline__ float distance_to(const float (&X)[3], const float (&O)[3]) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double d = (double)(X[i] - O[i]);
        s = s + d * d;
    }
    return (float)sqrt(s);
}

// src/LocalMapping.cc:277-352 for one match; X and v are left zero up to the step that defines them
__device__ __forceinline__ int triangulate(const orbt_pair& P, const Levels& L, const orbx_keypoint& k1, const orbx_keypoint& k2, float (&X)[3],
                                           float (&v)[4]) {
    const int o1 = k1.octave, o2 = k2.octave;
    if (o1 < 0 || o1 >= L.n || o2 < 0 || o2 >= L.n) return ORBT_SKIP_OCTAVE;
    float xn1[3], xn2[3], r1[3], r2[3];
    normalised(P.kf1, k1.x, k1.y, xn1, r1);
    normalised(P.kf2, k2.x, k2.y, xn2, r2);
    double dot = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        dot = dot + (double)r1[i] * (double)r2[i];
        s1 = s1 + (double)r1[i] * (double)r1[i];
        s2 = s2 + (double)r2[i] * (double)r2[i];
    }
    const float cosp = (float)(dot / (sqrt(s1) * sqrt(s2)));
    if (!(cosp >= 0.0f && (double)cosp <= 0.9998)) return ORBT_PARALLAX;
    float A[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float t10 = c < 3 ? P.kf1.Rcw[c] : P.kf1.tcw[0], t11 = c < 3 ? P.kf1.Rcw[3 + c] : P.kf1.tcw[1], t12 = c < 3 ? P.kf1.Rcw[6 + c] : P.kf1.tcw[2];
        const float t20 = c < 3 ? P.kf2.Rcw[c] : P.kf2.tcw[0], t21 = c < 3 ? P.kf2.Rcw[3 + c] : P.kf2.tcw[1], t22 = c < 3 ? P.kf2.Rcw[6 + c] : P.kf2.tcw[2];
        A[0][c] = xn1[0] * t12 - t10;
        A[1][c] = xn1[1] * t12 - t11;
        A[2][c] = xn2[0] * t22 - t20;
        A[3][c] = xn2[1] * t22 - t21;
    }
    null_vector(A, v);
    if (!(v[3] != 0.0f) || v[3] != v[3]) return ORBT_W_ZERO;
#pragma unroll
    for (int i = 0; i < 3; i++) X[i] = v[i] / v[3];
    const float z1 = cam_coord(P.kf1, 2, X);
    if (!(z1 > 0.0f)) return ORBT_DEPTH1;
    const float z2 = cam_coord(P.kf2, 2, X);
    if (!(z2 > 0.0f)) return ORBT_DEPTH2;
    if (reprojection_fails(P.kf1, X, z1, k1.x, k1.y, L.s1[o1])) return ORBT_REPROJ1;
    if (reprojection_fails(P.kf2, X, z2, k2.x, k2.y, L.s2[o2])) return ORBT_REPROJ2;
    const float d1 = distance_to(X, P.kf1.Ow), d2 = distance_to(X, P.kf2.Ow);
    if (d1 == 0.0f || d2 == 0.0f || d1 != d1 || d2 != d2) return ORBT_ZERO_DIST;
    const float ratio_dist = d1 / d2;
    const float ratio_octave = L.f1[o1] / L.f2[o2];
    const float ratio_factor = 1.5f * P.scale_factor;
    if (!(ratio_dist * ratio_factor >= ratio_octave && ratio_dist <= ratio_octave * ratio_factor)) return ORBT_SCALE;
    return ORBT_ACCEPTED;
}

__global__ __launch_bounds__(TPB) void k_triangulate(const orbt_pair* pairs, Levels L, const orbx_keypoint* kps1, const int32_t* n1s, int cap1, int stride1,
                                                     const orbx_keypoint* kps2, const int32_t* n2s, int cap2, const int32_t* q2t,
                                                     const int32_t* qindex, const int32_t* nqs, int qcap, uint8_t* status, float* x3d, float* vout,
                                                     int32_t* match12, int32_t* acc_idx, float* acc_x3d, int32_t* count, int32_t* overflow,
                                                     int ocap, uint8_t* qvalid, uint8_t* claimed) {
    __shared__ orbt_pair P;
    __shared__ int wave_total[WAVES];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (tid < (int)(sizeof(orbt_pair) / 4)) reinterpret_cast<uint32_t*>(&P)[tid] = reinterpret_cast<const uint32_t*>(pairs + p)[tid];
    int n1 = n1s[stride1 ? p : 0], n2 = n2s[p], nq = nqs[p];
    n1 = n1 < 0 ? 0 : (n1 > cap1 ? cap1 : n1);
    n2 = n2 < 0 ? 0 : (n2 > cap2 ? cap2 : n2);
    nq = nq < 0 ? 0 : (nq > qcap ? qcap : nq);
    const size_t b1 = (size_t)p * stride1, b2 = (size_t)p * cap2, bq = (size_t)p * qcap, bo = (size_t)p * cap1, ba = (size_t)p * ocap;
    // pass 1: every feature of KF1 starts without a match
    for (int i = tid; i < n1; i += TPB) {
        status[bo + i] = ORBT_NONE;
        match12[bo + i] = -1;
        float* x = x3d + (bo + i) * 3;
        x[0] = x[1] = x[2] = 0.0f;
        if (vout) reinterpret_cast<float4*>(vout)[bo + i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    // pass 2: one lane per match entry
    for (int q = tid; q < nq; q += TPB) {
        const int idx2 = q2t[bq + q];
        const int idx1 = qindex ? qindex[bq + q] : q;
        if (idx2 == -1 || idx1 < 0 || idx1 >= n1) continue;
        float X[3] = {0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int st = ORBT_SKIP_INDEX;
        if (idx2 >= 0 && idx2 < n2) st = triangulate(P, L, kps1[b1 + idx1], kps2[b2 + idx2], X, v);
        status[bo + idx1] = (uint8_t)st;
        match12[bo + idx1] = idx2;
        float* x = x3d + (bo + idx1) * 3;
        x[0] = X[0]; x[1] = X[1]; x[2] = X[2];
        if (vout) reinterpret_cast<float4*>(vout)[bo + idx1] = make_float4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    // pass 3: the accepted features in ascending idx1
    int base = 0;                                                      // accepted before this tile (uniform)
    for (int i0 = 0; i0 < n1; i0 += TPB) {
        const int i = i0 + tid;
        const bool acc = i < n1 && status[bo + i] == ORBT_ACCEPTED;
        const int k = orbx::tile_rank(acc, wave_total, base);
        if (acc) {
            const int idx2 = match12[bo + i];                          // in [0, n2): an accepted match passed the range test
            if (k < ocap) {
                acc_idx[(ba + k) * 2] = i;
                acc_idx[(ba + k) * 2 + 1] = idx2;
                const float* x = x3d + (bo + i) * 3;
                float* o = acc_x3d + (ba + k) * 3;
                o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
            }
            if (qvalid) qvalid[b1 + i] = 0;
            if (claimed) claimed[b2 + idx2] = 1;
        }
    }
    if (tid == 0) {
        count[p] = base;
        overflow[p] = base > ocap ? 1 : 0;
    }
}

int fill_levels(const float* f1, const float* s1, const float* f2, const float* s2, int nlevels, Levels& L) {
    if (!f1 || !s1 || !f2 || !s2 || nlevels < 1 || nlevels > ORBS_MAX_LEVELS) return ORBX_ERR_ARG;
    std::memset(&L, 0, sizeof(L));
    for (int i = 0; i < nlevels; i++) { L.f1[i] = f1[i]; L.s1[i] = s1[i]; L.f2[i] = f2[i]; L.s2[i] = s2[i]; }
    L.n = nlevels;
    return ORBX_OK;
}

}  // namespace orbt

extern "C" {

int orbt_triangulate_batch_device(const orbt_pair* d_pairs, int npairs, const float* factors1, const float* sigma2_1, const float* factors2,
                                  const float* sigma2_2, int nlevels, const orbx_keypoint* d_kps1, const int32_t* d_n1, int cap1, int stride1,
                                  const orbx_keypoint* d_kps2, const int32_t* d_n2, int cap2, const int32_t* d_q2t, const int32_t* d_qindex,
                                  const int32_t* d_nq, int qcap, uint8_t* d_status, float* d_x3d, float* d_v, int32_t* d_match12,
                                  int32_t* d_acc_idx, float* d_acc_x3d, int32_t* d_count, int32_t* d_overflow, int ocap, uint8_t* d_qvalid,
                                  uint8_t* d_claimed, void* stream) {
    orbt::Levels L;
    if (orbt::fill_levels(factors1, sigma2_1, factors2, sigma2_2, nlevels, L) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs < 0 || npairs > ORBT_MAX_PAIRS || cap1 < 1 || cap1 > ORBF_MAX_FEATURES || cap2 < 1 || cap2 > ORBF_MAX_FEATURES || qcap < 1 ||
        qcap > ORBF_MAX_FEATURES || ocap < 1)
        return ORBX_ERR_ARG;
    if (stride1 != 0 && stride1 < cap1) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    if (!d_pairs || !d_kps1 || !d_n1 || !d_kps2 || !d_n2 || !d_q2t || !d_nq || !d_status || !d_x3d || !d_match12 || !d_acc_idx || !d_acc_x3d ||
        !d_count || !d_overflow)
        return ORBX_ERR_ARG;
    if (d_v && ((uintptr_t)d_v & 15)) return ORBX_ERR_ARG;             // written as float4
    hipLaunchKernelGGL(orbt::k_triangulate, dim3(npairs), dim3(orbt::TPB), 0, (hipStream_t)stream, d_pairs, L, d_kps1, d_n1, cap1, stride1, d_kps2, d_n2,
                       cap2, d_q2t, d_qindex, d_nq, qcap, d_status, d_x3d, d_v, d_match12, d_acc_idx, d_acc_x3d, d_count, d_overflow, ocap, d_qvalid,
                       d_claimed);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbt_triangulate(const orbt_pair* pair, const float* factors1, const float* sigma2_1, const float* factors2, const float* sigma2_2,
                     int nlevels, const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, const int32_t* match12,
                     uint8_t* status, float* x3d, float* v, int32_t* acc_idx, float* acc_x3d, int ocap, int* count, int device) {
    orbt::Levels L;
    if (orbt::fill_levels(factors1, sigma2_1, factors2, sigma2_2, nlevels, L) != ORBX_OK) return ORBX_ERR_ARG;
    if (!pair || n1 < 0 || n1 > ORBF_MAX_FEATURES || n2 < 0 || n2 > ORBF_MAX_FEATURES || ocap < 1 || !count || !acc_idx || !acc_x3d) return ORBX_ERR_ARG;
    if (n1 > 0 && (!kps1 || !match12 || !status || !x3d)) return ORBX_ERR_ARG;
    if (n2 > 0 && !kps2) return ORBX_ERR_ARG;
    HIPTRY(hipSetDevice(device));
    const int32_t counts[2] = {n1, n2};
    const int cap1 = std::max(n1, 1), cap2 = std::max(n2, 1);
    orbx::Staging s;
    const auto pr = s.in(pair, 1);
    const auto k1 = s.in(kps1, n1), k2 = s.in(kps2, n2);
    const auto m12 = s.in(match12, n1);
    const auto cn = s.in(counts, 2);
    const auto st = s.out<uint8_t>(n1);
    const auto x = s.out<float>((size_t)n1 * 3), vv = s.out<float>((size_t)n1 * 4);
    const auto work = s.out<int32_t>(n1);
    const auto ai = s.out<int32_t>((size_t)ocap * 2);
    const auto ax = s.out<float>((size_t)ocap * 3);
    const auto res = s.out<int32_t>(2);
    HIPTRY(s.alloc());
    const int rc = orbt_triangulate_batch_device(s[pr], 1, factors1, sigma2_1, factors2, sigma2_2, nlevels, s[k1], s[cn], cap1, 0, s[k2], s[cn] + 1, cap2,
                                                 s[m12], nullptr, s[cn], cap1, s[st], s[x], v ? s[vv] : nullptr, s[work], s[ai], s[ax], s[res],
                                                 s[res] + 1, ocap, nullptr, nullptr, nullptr);
    if (rc != ORBX_OK) return rc;
    int32_t r[2] = {0, 0};
    HIPTRY(s.get(r, res, 2));
    HIPTRY(s.get(status, st, n1));
    HIPTRY(s.get(x3d, x, (size_t)n1 * 3));
    if (v) HIPTRY(s.get(v, vv, (size_t)n1 * 4));
    const size_t kept = (size_t)std::min(r[0], ocap);
    HIPTRY(s.get(acc_idx, ai, kept * 2));
    HIPTRY(s.get(acc_x3d, ax, kept * 3));
    *count = r[0];
    return r[1] ? ORBX_ERR_CAPACITY : ORBX_OK;
}

}  // extern "C"
