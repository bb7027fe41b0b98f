// The monocular initialisation on gfx950: the RANSAC of Initializer::FindHomography / FindFundamental (reference src/Initializer.cc:122-170,
// :173-221 with ComputeH21 :224-264, ComputeF21 :266-301, CheckHomography :303-386, CheckFundamental :388-466) and Initializer::CheckRT (:796-905 with
// Triangulate :732-745).  include/orbi.h is the boundary and states the arithmetic; orbi_math.h holds it, shared with the host.
//
// Kernels:
//   k_init_models    one workgroup of ONE wave per (iteration, model, problem): 400 waves for one reference-sized problem, bound by the
//       latency of the dependent rotations, not by any rate.  Lanes 0-7 normalise the set and fill A (LDS, float); the 81 entries of
//       A'A are spread over the lanes; the 9 x 9 Jacobi iteration keeps A'A and V in LDS (two 9 x 9 matrices of doubles do not fit one
//       lane's registers without spilling) with lane k owning row k (orbj::sym_eig_wave); lane 0 runs the 3 x 3 step and the matrix
//       chain in double.  Then the wave scores all matches in chunks of 64: every lane computes the two terms of its match and ONE
//       sequence of lane reads adds the 128 terms in match order into a uniform float, so the sum is the source's sequential sum.
//   k_init_select    one workgroup per problem: thread 0 scans the scores with the source's strict `>`, then the workgroup recomputes the
//       winners' inlier flags with the same device function.
//   k_init_check_rt  one workgroup per (hypothesis, problem), one lane per match entry as in k_triangulate's pass 2; nGood is the sum, by thread 0, of the
//       workgroup's 256 per-thread counts in LDS (no atomics).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "orbi.h"
#include "orbi_host.h"
#include "orbi_math.h"
#include "orbx_host.h"

namespace orbi {

constexpr int RT_TPB = 256;
constexpr int SEL_TPB = 256;

// key points of match entry i of a problem, false when an index lies outside the frames
__device__ __forceinline__ bool match_points(const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches, int i, float& u1,
                                             float& v1, float& u2, float& v2) {
    const int i1 = matches[i * 2], i2 = matches[i * 2 + 1];
    if (i1 < 0 || i1 >= n1 || i2 < 0 || i2 >= n2) return false;
    u1 = k1[i1].x; v1 = k1[i1].y;
    u2 = k2[i2].x; v2 = k2[i2].y;
    return true;
}

__device__ __forceinline__ float lane_value(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }

__global__ __launch_bounds__(64) void k_init_models(Problems PR, const orbx_keypoint* kps1, int kcap1, const orbx_keypoint* kps2, int kcap2,
                                                    const int32_t* matches, int mcap, const int32_t* sets, int icap, float* scoreH, float* scoreF,
                                                    float* H21, float* H12, float* F21, float* hn_out, float* fpre_out) {
    __shared__ float A[16 * 9];
    __shared__ double S[81], V[81], S3[9], V3[9];
    __shared__ float vec[9], mats[18];
    __shared__ int bad;
    const int it = blockIdx.x, model = blockIdx.y, p = blockIdx.z, lane = threadIdx.x;
    const orbi_problem& Q = PR.p[p];
    if (it >= Q.iters) return;
    const int N = Q.nmatches, n1 = Q.n1, n2 = Q.n2;
    const orbx_keypoint* k1 = kps1 + (size_t)p * kcap1;
    const orbx_keypoint* k2 = kps2 + (size_t)p * kcap2;
    const int32_t* mt = matches + (size_t)p * mcap * 2;
    const size_t slot = (size_t)p * icap + it;
    const int rows = model == 0 ? 16 : 8;
    if (lane == 0) bad = 0;
    __syncthreads();
    if (lane < 8) {
        const int idx = sets[slot * 8 + lane];
        float u1, v1, u2, v2;
        if (idx < 0 || idx >= N || !match_points(k1, n1, k2, n2, mt, idx, u1, v1, u2, v2)) {
            bad = 1;                                           // up to eight lanes store the same value: whichever lands, the flag is set
        } else {
            u1 = (u1 - Q.norm1[2]) * Q.norm1[0]; v1 = (v1 - Q.norm1[3]) * Q.norm1[1];
            u2 = (u2 - Q.norm2[2]) * Q.norm2[0]; v2 = (v2 - Q.norm2[3]) * Q.norm2[1];
            if (model == 0) {
                homography_row(0, u1, v1, u2, v2, A + (2 * lane) * 9);
                homography_row(1, u1, v1, u2, v2, A + (2 * lane + 1) * 9);
            } else {
                fundamental_row(u1, v1, u2, v2, A + lane * 9);
            }
        }
    }
    __syncthreads();
    float* const out1 = (model == 0 ? H21 : F21) + slot * 9;
    float* const out2 = H12 + slot * 9;
    float* const vout = model == 0 ? hn_out : fpre_out;
    if (bad) {
        if (lane < 9) {
            out1[lane] = 0.0f;
            if (model == 0) out2[lane] = 0.0f;
            if (vout) vout[slot * 9 + lane] = 0.0f;
        }
        if (lane == 0) (model == 0 ? scoreH : scoreF)[slot] = 0.0f;
        return;
    }
    for (int e = lane; e < 81; e += 64) S[e] = orbj::gram_entry<9>(A, rows, e / 9, e % 9);
    __syncthreads();
    orbj::sym_eig_wave<9>(S, V, lane);
    __syncthreads();
    const int k = orbj::smallest_eigenvalue<9>(S);
    if (lane < 9) {
        vec[lane] = (float)V[lane * 9 + k];
        if (vout) vout[slot * 9 + lane] = vec[lane];
    }
    __syncthreads();
    if (lane == 0) {
        if (model == 0) {
            homography_chain(vec, Q.norm1, Q.norm2, mats, mats + 9);
        } else {
            gram3(vec, S3);
            orbj::sym_eig<3>(S3, V3);
            fundamental_chain(vec, V3, orbj::smallest_eigenvalue<3>(S3), Q.norm1, Q.norm2, mats);
        }
    }
    __syncthreads();
    if (lane < 9) {
        out1[lane] = mats[lane];
        if (model == 0) out2[lane] = mats[9 + lane];
    }
    float M1[9], M2[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { M1[i] = mats[i]; M2[i] = model == 0 ? mats[9 + i] : 0.0f; }
    const float iss = inv_sigma_square(Q.sigma);
    float score = 0.0f;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        Terms t = {0.0f, 0.0f, false};
        float u1, v1, u2, v2;
        if (i < N && match_points(k1, n1, k2, n2, mt, i, u1, v1, u2, v2))
            t = model == 0 ? homography_terms(M1, M2, u1, v1, u2, v2, iss) : fundamental_terms(M1, u1, v1, u2, v2, iss);
        const int cnt = min(64, N - base);
        if (cnt == 64) {
#pragma unroll
            for (int l = 0; l < 64; l++) {
                score = score + lane_value(t.t1, l);
                score = score + lane_value(t.t2, l);
            }
        } else {
            for (int l = 0; l < cnt; l++) {
                score = score + lane_value(t.t1, l);
                score = score + lane_value(t.t2, l);
            }
        }
    }
    if (lane == 0) (model == 0 ? scoreH : scoreF)[slot] = score;
}

__global__ __launch_bounds__(SEL_TPB) void k_init_select(Problems PR, const orbx_keypoint* kps1, int kcap1, const orbx_keypoint* kps2, int kcap2,
                                                         const int32_t* matches, int mcap, int icap, const float* scoreH, const float* scoreF,
                                                         const float* H21, const float* H12, const float* F21, int32_t* best, float* Sout,
                                                         uint8_t* inlH, uint8_t* inlF) {
    __shared__ int bsel[2];
    __shared__ float mats[27];
    const int p = blockIdx.x, tid = threadIdx.x;
    const orbi_problem& Q = PR.p[p];
    const int N = Q.nmatches;
    if (tid < 2) {
        const float* sc = (tid == 0 ? scoreH : scoreF) + (size_t)p * icap;
        float s = 0.0f;
        int b = -1;
        for (int it = 0; it < Q.iters; it++) {
            const float c = sc[it];
            if (c > s) { s = c; b = it; }
        }
        bsel[tid] = b;
        best[p * 2 + tid] = b;
        Sout[p * 2 + tid] = s;
    }
    __syncthreads();
    const int bH = bsel[0], bF = bsel[1];
    if (tid < 27) {
        float x = 0.0f;
        if (tid < 9) { if (bH >= 0) x = H21[((size_t)p * icap + bH) * 9 + tid]; }
        else if (tid < 18) { if (bH >= 0) x = H12[((size_t)p * icap + bH) * 9 + tid - 9]; }
        else if (bF >= 0) x = F21[((size_t)p * icap + bF) * 9 + tid - 18];
        mats[tid] = x;
    }
    __syncthreads();
    const orbx_keypoint* k1 = kps1 + (size_t)p * kcap1;
    const orbx_keypoint* k2 = kps2 + (size_t)p * kcap2;
    const int32_t* mt = matches + (size_t)p * mcap * 2;
    const float iss = inv_sigma_square(Q.sigma);
    for (int i = tid; i < N; i += SEL_TPB) {
        float u1, v1, u2, v2;
        bool h = false, f = false;
        if (match_points(k1, Q.n1, k2, Q.n2, mt, i, u1, v1, u2, v2)) {
            h = bH >= 0 && homography_terms(mats, mats + 9, u1, v1, u2, v2, iss).in;
            f = bF >= 0 && fundamental_terms(mats + 18, u1, v1, u2, v2, iss).in;
        }
        inlH[(size_t)p * mcap + i] = h ? 1 : 0;
        inlF[(size_t)p * mcap + i] = f ? 1 : 0;
    }
}

__global__ __launch_bounds__(RT_TPB) void k_init_check_rt(float fx, float fy, float cx, float cy, const orbi_pose* poses, int nhyp, RtCounts C,
                                                          const orbx_keypoint* kps1, int kcap1, const orbx_keypoint* kps2, int kcap2,
                                                          const int32_t* matches, int mcap, const uint8_t* flags, float th2, uint8_t* status,
                                                          float* x3d, float* cosp, uint8_t* good, float* vout, int32_t* ngood) {
    __shared__ int counts[RT_TPB];
    const int h = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const int N = C.nm[p], n1 = C.n1[p], n2 = C.n2[p];
    const orbi_pose P = poses[(size_t)p * nhyp + h];
    const orbx_keypoint* k1 = kps1 + (size_t)p * kcap1;
    const orbx_keypoint* k2 = kps2 + (size_t)p * kcap2;
    const int32_t* mt = matches + (size_t)p * mcap * 2;
    const uint8_t* fl = flags + (size_t)p * mcap;
    const size_t eb = ((size_t)p * nhyp + h) * mcap;
    int mine = 0;
    for (int i = tid; i < N; i += RT_TPB) {
        RtOut o;
        o.X[0] = o.X[1] = o.X[2] = 0.0f;
        o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f;
        o.cosp = 0.0f;
        o.status = ORBI_RT_NONE;
        if (fl[i]) {
            float u1, v1, u2, v2;
            if (match_points(k1, n1, k2, n2, mt, i, u1, v1, u2, v2)) check_rt_one(fx, fy, cx, cy, P, u1, v1, u2, v2, th2, o);
            else o.status = ORBI_RT_SKIP_INDEX;
        }
        const size_t e = eb + i;
        status[e] = (uint8_t)o.status;
        x3d[e * 3] = o.X[0]; x3d[e * 3 + 1] = o.X[1]; x3d[e * 3 + 2] = o.X[2];
        cosp[e] = o.cosp;
        good[e] = o.status == ORBI_RT_GOOD ? 1 : 0;
        if (vout) reinterpret_cast<float4*>(vout)[e] = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
        mine += o.status == ORBI_RT_GOOD || o.status == ORBI_RT_COUNTED;
    }
    counts[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int i = 0; i < RT_TPB; i++) total += counts[i];
        ngood[p * nhyp + h] = total;
    }
}

}  // namespace orbi

extern "C" {

int orbi_normalize(const orbx_keypoint* kps, int n, float* out) {
    if (!kps || !out || n < 1) return ORBX_ERR_ARG;
    orbi::normalize(kps, n, out);
    return ORBX_OK;
}

int orbi_pose_from_rt(float fx, float fy, float cx, float cy, const float* R, const float* t, orbi_pose* pose) {
    if (!R || !t || !pose) return ORBX_ERR_ARG;
    orbi::pose_from_rt(fx, fy, cx, cy, R, t, pose);
    return ORBX_OK;
}

int orbi_models_batch_device(const orbi_problem* problems, int nproblems, const orbx_keypoint* d_kps1, int kcap1, const orbx_keypoint* d_kps2,
                             int kcap2, const int32_t* d_matches, int mcap, const int32_t* d_sets, int icap, float* d_scoreH, float* d_scoreF,
                             float* d_H21, float* d_H12, float* d_F21, float* d_hn, float* d_fpre, int32_t* d_best, float* d_S,
                             uint8_t* d_inlH, uint8_t* d_inlF, void* stream) {
    orbi::Problems PR;
    int iters = 0;
    TRY(orbi::check_models(problems, nproblems, d_kps1, kcap1, d_kps2, kcap2, d_matches, mcap, d_sets, icap, d_scoreH, d_scoreF, d_H21, d_H12, d_F21, d_best,
                           d_S, d_inlH, d_inlF, PR, iters));
    hipLaunchKernelGGL(orbi::k_init_models, dim3(iters, 2, nproblems), dim3(64), 0, (hipStream_t)stream, PR, d_kps1, kcap1, d_kps2, kcap2, d_matches, mcap,
                       d_sets, icap, d_scoreH, d_scoreF, d_H21, d_H12, d_F21, d_hn, d_fpre);
    hipLaunchKernelGGL(orbi::k_init_select, dim3(nproblems), dim3(orbi::SEL_TPB), 0, (hipStream_t)stream, PR, d_kps1, kcap1, d_kps2, kcap2, d_matches, mcap,
                       icap, d_scoreH, d_scoreF, d_H21, d_H12, d_F21, d_best, d_S, d_inlH, d_inlF);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbi_models(const orbi_problem* problem, const orbx_keypoint* kps1, const orbx_keypoint* kps2, const int32_t* matches, const int32_t* sets,
                float* scoreH, float* scoreF, float* H21, float* H12, float* F21, float* hn, float* fpre, int32_t* best, float* S,
                uint8_t* inlH, uint8_t* inlF, int device) {
    if (!problem || orbi::check_problem(*problem) != ORBX_OK) return ORBX_ERR_ARG;
    if (!kps1 || !kps2 || !matches || !sets || !scoreH || !scoreF || !H21 || !H12 || !F21 || !best || !S || !inlH || !inlF) return ORBX_ERR_ARG;
    const orbi_problem& q = *problem;
    const size_t N = q.nmatches, I = q.iters;
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto k1 = s.in(kps1, q.n1), k2 = s.in(kps2, q.n2);
    const auto mt = s.in(matches, N * 2), st = s.in(sets, I * 8);
    const auto sh = s.out<float>(I), sf = s.out<float>(I);
    const auto h21 = s.out<float>(I * 9), h12 = s.out<float>(I * 9), f21 = s.out<float>(I * 9), vh = s.out<float>(I * 9), vf = s.out<float>(I * 9);
    const auto bs = s.out<int32_t>(2);
    const auto ss = s.out<float>(2);
    const auto ih = s.out<uint8_t>(N), jf = s.out<uint8_t>(N);
    HIPTRY(s.alloc());
    const int rc = orbi_models_batch_device(problem, 1, s[k1], q.n1, s[k2], q.n2, s[mt], (int)N, s[st], (int)I, s[sh], s[sf], s[h21], s[h12], s[f21],
                                            hn ? s[vh] : nullptr, fpre ? s[vf] : nullptr, s[bs], s[ss], s[ih], s[jf], nullptr);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(scoreH, sh, I));
    HIPTRY(s.get(scoreF, sf, I));
    HIPTRY(s.get(H21, h21, I * 9));
    HIPTRY(s.get(H12, h12, I * 9));
    HIPTRY(s.get(F21, f21, I * 9));
    if (hn) HIPTRY(s.get(hn, vh, I * 9));
    if (fpre) HIPTRY(s.get(fpre, vf, I * 9));
    HIPTRY(s.get(best, bs, 2));
    HIPTRY(s.get(S, ss, 2));
    HIPTRY(s.get(inlH, ih, N));
    HIPTRY(s.get(inlF, jf, N));
    return ORBX_OK;
}

int orbi_check_rt_batch_device(float fx, float fy, float cx, float cy, const orbi_pose* d_poses, int nhyp, int nproblems, const int32_t* n1,
                               const int32_t* n2, const int32_t* nmatches, const orbx_keypoint* d_kps1, int kcap1, const orbx_keypoint* d_kps2,
                               int kcap2, const int32_t* d_matches, int mcap, const uint8_t* d_flags, float th2, uint8_t* d_status,
                               float* d_x3d, float* d_cos, uint8_t* d_good, float* d_v, int32_t* d_ngood, void* stream) {
    orbi::RtCounts C;
    TRY(orbi::check_rt(d_poses, nhyp, nproblems, n1, n2, nmatches, d_kps1, kcap1, d_kps2, kcap2, d_matches, mcap, d_flags, d_status, d_x3d, d_cos, d_good,
                       d_v, d_ngood, C));
    hipLaunchKernelGGL(orbi::k_init_check_rt, dim3(nhyp, nproblems), dim3(orbi::RT_TPB), 0, (hipStream_t)stream, fx, fy, cx, cy, d_poses, nhyp, C, d_kps1,
                       kcap1, d_kps2, kcap2, d_matches, mcap, d_flags, th2, d_status, d_x3d, d_cos, d_good, d_v, d_ngood);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbi_check_rt(float fx, float fy, float cx, float cy, const orbi_pose* poses, int nhyp, const orbx_keypoint* kps1, int n1,
                  const orbx_keypoint* kps2, int n2, const int32_t* matches, int nmatches, const uint8_t* flags, float th2, uint8_t* status,
                  float* x3d, float* cosp, uint8_t* good, float* v, int32_t* ngood, float* parallax, int device) {
    if (!poses || nhyp < 1 || nhyp > ORBI_MAX_HYP || n1 < 1 || n1 > ORBF_MAX_FEATURES || n2 < 1 || n2 > ORBF_MAX_FEATURES || nmatches < 1 ||
        nmatches > ORBI_MAX_MATCHES)
        return ORBX_ERR_ARG;
    if (!kps1 || !kps2 || !matches || !flags || !status || !x3d || !cosp || !good || !ngood || !parallax) return ORBX_ERR_ARG;
    const size_t N = nmatches, HN = (size_t)nhyp * N;
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto ps = s.in(poses, nhyp);
    const auto k1 = s.in(kps1, n1), k2 = s.in(kps2, n2);
    const auto mt = s.in(matches, N * 2);
    const auto fl = s.in(flags, N);
    const auto st = s.out<uint8_t>(HN);
    const auto x = s.out<float>(HN * 3), cs = s.out<float>(HN);
    const auto gd = s.out<uint8_t>(HN);
    const auto vv = s.out<float>(HN * 4);
    const auto ng = s.out<int32_t>(nhyp);
    HIPTRY(s.alloc());
    const int32_t c1 = n1, c2 = n2, cm = nmatches;
    const int rc = orbi_check_rt_batch_device(fx, fy, cx, cy, s[ps], nhyp, 1, &c1, &c2, &cm, s[k1], n1, s[k2], n2, s[mt], nmatches, s[fl], th2, s[st],
                                              s[x], s[cs], s[gd], v ? s[vv] : nullptr, s[ng], nullptr);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(status, st, HN));
    HIPTRY(s.get(x3d, x, HN * 3));
    HIPTRY(s.get(cosp, cs, HN));
    HIPTRY(s.get(good, gd, HN));
    if (v) HIPTRY(s.get(v, vv, HN * 4));
    HIPTRY(s.get(ngood, ng, nhyp));
    std::vector<float> counted;
    for (int h = 0; h < nhyp; h++) {
        counted.clear();
        for (size_t i = 0; i < N; i++)
            if (status[h * N + i] == ORBI_RT_GOOD || status[h * N + i] == ORBI_RT_COUNTED) counted.push_back(cosp[h * N + i]);
        parallax[h] = orbi::parallax_of(counted.data(), (int)counted.size());
    }
    return ORBX_OK;
}

}  // extern "C"
