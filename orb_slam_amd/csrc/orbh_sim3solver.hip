// The Sim3 RANSAC of loop closing on gfx950: Sim3Solver::iterate / computeT / CheckInliers / Project (reference src/Sim3Solver.cc:140-359, :377-398).
// include/orbh.h is the boundary and states the arithmetic; orbh_math.h holds it, shared with the host.
//
// Kernels:
//   k_sim3_hypotheses  one workgroup of ONE wave per (iteration, problem): up to 300 waves per solver.  The fit is about 600 dependent double
//       operations (the 4 x 4 Jacobi iteration in registers) over six floats per correspondence; EVERY lane runs it on the same three
//       correspondences (their indices are uniform, so the loads are scalar).  That costs the wave what one lane would cost it, and leaves the
//       transforms in every lane's registers: no LDS, no barrier, no broadcast.  Then the lanes stride over the N correspondences of the
//       struct-of-arrays point table (consecutive lanes, consecutive floats) for both projections; a ballot is one flag word, written by lane 0,
//       and the count is the sum of the ballots' population counts.
//   k_sim3_select      one workgroup per problem: the workgroup gathers the counts into LDS, thread 0 walks them, the workgroup copies the chosen flag words.
// No floating-point atomics, no atomics at all, no scratch, no inline assembly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "orbh.h"
#include "orbh_host.h"
#include "orbh_math.h"
#include "orbx_host.h"

namespace orbh {

constexpr int HYP_TPB = 64;
constexpr int SEL_TPB = 128;

__global__ __launch_bounds__(HYP_TPB) void k_sim3_hypotheses(Problems PR, const float* points, int ncap, const int32_t* sets, int icap, orbh_hyp* hyp,
                                                             uint64_t* flags) {
    const int it = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const orbh_problem& q = PR.p[p];
    if (it >= q.iters) return;
    const int n = q.n, words = ORBH_WORDS(n);
    const size_t s = (size_t)p * icap + it;
    const float* T = points + (size_t)p * ORBH_POINT_ROWS * ncap;
    uint64_t* fl = flags + s * ORBH_WORDS(ncap);
    const int i0 = sets[s * 3], i1 = sets[s * 3 + 1], i2 = sets[s * 3 + 2];
    orbh_hyp h;
    if (i0 < 0 || i0 >= n || i1 < 0 || i1 >= n || i2 < 0 || i2 >= n) {                              // uniform
        void_hyp(h);
        if (lane == 0) hyp[s] = h;
        for (int w = lane; w < words; w += HYP_TPB) fl[w] = 0;
        return;
    }
    float A[6], B[6], C[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        A[r] = T[(size_t)r * ncap + i0];
        B[r] = T[(size_t)r * ncap + i1];
        C[r] = T[(size_t)r * ncap + i2];
    }
    fit(A, B, C, h);
    int count = 0;
    for (int base = 0; base < n; base += HYP_TPB) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            float v[ORBH_POINT_ROWS];
#pragma unroll
            for (int r = 0; r < ORBH_POINT_ROWS; r++) v[r] = T[(size_t)r * ncap + i];
            in = is_inlier(q, h.T12, h.T21, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]);
        }
        const unsigned long long m = __ballot(in);                                                  // bit l = lane l = correspondence base + l
        if (lane == 0) fl[base / 64] = m;
        count += __popcll(m);
    }
    h.count = count;
    if (lane == 0) hyp[s] = h;
}

__global__ __launch_bounds__(SEL_TPB) void k_sim3_select(Problems PR, int ncap, int icap, const orbh_hyp* hyp, const uint64_t* flags, orbh_state* state,
                                                         uint64_t* best_flags, orbh_result* result, uint64_t* result_flags) {
    __shared__ int32_t cnt[ORBH_MAX_ITERS];                        // the range's counts: the walk is serial, and from global memory it costs a load's latency per iteration
    __shared__ int best_it, found;
    const int p = blockIdx.x, tid = threadIdx.x;
    const orbh_problem& q = PR.p[p];
    const size_t base = (size_t)p * icap, wcap = ORBH_WORDS(ncap);
    for (int i = tid; i < q.iters; i += SEL_TPB) cnt[i] = hyp[base + i].count;      // iters <= ORBH_MAX_ITERS (check_batch)
    __syncthreads();
    if (tid == 0) {
        orbh_state st = state[p];
        orbh_result res;
        best_it = walk(q, cnt, st, res).best_it;
        if (best_it >= 0) take_best(hyp[base + best_it], st, res);
        found = res.found;
        state[p] = st;
        result[p] = res;
    }
    __syncthreads();
    const int b_it = best_it, f = found;
    for (int w = tid; w < ORBH_WORDS(q.n); w += SEL_TPB) {
        uint64_t b = best_flags[p * wcap + w];
        if (b_it >= 0) {
            b = flags[(base + b_it) * wcap + w];
            best_flags[p * wcap + w] = b;
        }
        result_flags[p * wcap + w] = f ? b : 0;
    }
}

}  // namespace orbh

extern "C" {

int orbh_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int32_t* max_its_out) {
    if (n < 0 || !max_its_out) return ORBX_ERR_ARG;
    *max_its_out = orbh::ransac_parameters(n, probability, min_inliers, max_iterations);
    return ORBX_OK;
}

int orbh_max_errors(int n, const float* sigma2, float* maxerr) {
    if (n < 0 || (n > 0 && (!sigma2 || !maxerr))) return ORBX_ERR_ARG;
    for (int i = 0; i < n; i++) maxerr[i] = orbh::max_error(sigma2[i]);
    return ORBX_OK;
}

int orbh_hypotheses_batch_device(const orbh_problem* problems, int nproblems, const float* d_points, int ncap, const int32_t* d_sets, int icap,
                                 orbh_hyp* d_hyp, uint64_t* d_flags, void* stream) {
    orbh::Problems PR;
    int iters = 0;
    TRY(orbh::check_batch(problems, nproblems, ncap, icap, PR, iters));
    if (!orbh::all_set({d_points, d_sets, d_hyp, d_flags})) return ORBX_ERR_ARG;
    hipLaunchKernelGGL(orbh::k_sim3_hypotheses, dim3(iters, nproblems), dim3(orbh::HYP_TPB), 0, (hipStream_t)stream, PR, d_points, ncap, d_sets, icap, d_hyp,
                       d_flags);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbh_select_batch_device(const orbh_problem* problems, int nproblems, int ncap, int icap, const orbh_hyp* d_hyp, const uint64_t* d_flags,
                             orbh_state* d_state, uint64_t* d_best_flags, orbh_result* d_result, uint64_t* d_result_flags, void* stream) {
    orbh::Problems PR;
    int iters = 0;
    TRY(orbh::check_batch(problems, nproblems, ncap, icap, PR, iters));
    if (!orbh::all_set({d_hyp, d_flags, d_state, d_best_flags, d_result, d_result_flags})) return ORBX_ERR_ARG;
    hipLaunchKernelGGL(orbh::k_sim3_select, dim3(nproblems), dim3(orbh::SEL_TPB), 0, (hipStream_t)stream, PR, ncap, icap, d_hyp, d_flags, d_state,
                       d_best_flags, d_result, d_result_flags);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbh_hypotheses(const orbh_problem* problem, const float* x3dc1, const float* x3dc2, const float* p1im1, const float* p2im2, const float* maxerr1,
                    const float* maxerr2, const int32_t* sets, orbh_hyp* hyp, uint64_t* flags, int device) {
    if (!problem || orbh::check_problem(*problem) != ORBX_OK || !orbh::all_set({x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, sets, hyp, flags}))
        return ORBX_ERR_ARG;
    const size_t N = problem->n, I = problem->iters, W = ORBH_WORDS(N);
    std::vector<float> table(ORBH_POINT_ROWS * N);
    orbh::pack_points((int)N, (int)N, x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, table.data());
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto ip = s.in(table.data(), table.size());
    const auto is = s.in(sets, I * 3);
    const auto oh = s.out<orbh_hyp>(I);
    const auto of = s.out<uint64_t>(I * W);
    HIPTRY(s.alloc());
    TRY(orbh_hypotheses_batch_device(problem, 1, s[ip], (int)N, s[is], (int)I, s[oh], s[of], nullptr));
    HIPTRY(s.get(hyp, oh, I));
    HIPTRY(s.get(flags, of, I * W));
    return ORBX_OK;
}

int orbh_select(const orbh_problem* problem, const orbh_hyp* hyp, const uint64_t* flags, orbh_state* state, uint64_t* best_flags, orbh_result* result,
                uint64_t* result_flags, int device) {
    if (!problem || orbh::check_problem(*problem) != ORBX_OK || !orbh::all_set({hyp, flags, state, best_flags, result, result_flags})) return ORBX_ERR_ARG;
    TRY(orbh::check_state(*state));
    const size_t N = problem->n, I = problem->iters, W = ORBH_WORDS(N);
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto ih = s.in(hyp, I);
    const auto jf = s.in(flags, I * W);
    const auto is = s.in(state, 1);
    const auto bf = s.in(best_flags, W);
    const auto orr = s.out<orbh_result>(1);
    const auto of = s.out<uint64_t>(W);
    HIPTRY(s.alloc());
    TRY(orbh_select_batch_device(problem, 1, (int)N, (int)I, s[ih], s[jf], s[is], s[bf], s[orr], s[of], nullptr));
    HIPTRY(s.get(state, is, 1));
    HIPTRY(s.get(best_flags, bf, W));
    HIPTRY(s.get(result, orr, 1));
    HIPTRY(s.get(result_flags, of, W));
    return ORBX_OK;
}

int orbh_iterate_batch(const orbh_problem* problems, int nproblems, const float* const* x3dc1, const float* const* x3dc2, const float* const* p1im1,
                       const float* const* p2im2, const float* const* maxerr1, const float* const* maxerr2, const int32_t* const* sets,
                       orbh_state* states, uint64_t* const* best_flags, orbh_result* results, uint64_t* const* result_flags, orbh_hyp* const* hyp,
                       uint64_t* const* flags, int device) {
    if (!problems || nproblems < 1 || nproblems > ORBH_MAX_PROBLEMS ||
        !orbh::all_set({x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, sets, states, best_flags, results, result_flags}))
        return ORBX_ERR_ARG;
    size_t N = 0, I = 0;
    for (int p = 0; p < nproblems; p++) {
        if (orbh::check_problem(problems[p]) != ORBX_OK || orbh::check_state(states[p]) != ORBX_OK ||
            !orbh::all_set({x3dc1[p], x3dc2[p], p1im1[p], p2im2[p], maxerr1[p], maxerr2[p], sets[p], best_flags[p], result_flags[p]}))
            return ORBX_ERR_ARG;
        N = std::max(N, (size_t)problems[p].n);
        I = std::max(I, (size_t)problems[p].iters);
    }
    // the solvers' arrays packed to the shared caps N, I
    const size_t P = nproblems, W = ORBH_WORDS(N);
    std::vector<float> hp(P * ORBH_POINT_ROWS * N);
    std::vector<int32_t> hs(P * I * 3);
    std::vector<uint64_t> hb(P * W);
    for (size_t p = 0; p < P; p++) {
        const size_t n = problems[p].n, it = problems[p].iters;
        orbh::pack_points((int)n, (int)N, x3dc1[p], x3dc2[p], p1im1[p], p2im2[p], maxerr1[p], maxerr2[p], &hp[p * ORBH_POINT_ROWS * N]);
        std::memcpy(&hs[p * I * 3], sets[p], it * 3 * sizeof(int32_t));
        std::memcpy(&hb[p * W], best_flags[p], ORBH_WORDS(n) * sizeof(uint64_t));
    }
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto ip = s.in(hp.data(), hp.size());
    const auto st = s.in(hs.data(), hs.size());
    const auto is = s.in(states, P);
    const auto bf = s.in(hb.data(), hb.size());
    const auto oh = s.out<orbh_hyp>(P * I);
    const auto of = s.out<uint64_t>(P * I * W);
    const auto orr = s.out<orbh_result>(P);
    const auto rfl = s.out<uint64_t>(P * W);
    HIPTRY(s.alloc());
    const int nc = (int)N, ic = (int)I;
    TRY(orbh_hypotheses_batch_device(problems, nproblems, s[ip], nc, s[st], ic, s[oh], s[of], nullptr));
    TRY(orbh_select_batch_device(problems, nproblems, nc, ic, s[oh], s[of], s[is], s[bf], s[orr], s[rfl], nullptr));
    std::vector<uint64_t> ho(P * W), hf;
    std::vector<orbh_hyp> hh;
    HIPTRY(s.get(states, is, P));
    HIPTRY(s.get(hb.data(), bf, hb.size()));
    HIPTRY(s.get(results, orr, P));
    HIPTRY(s.get(ho.data(), rfl, ho.size()));
    if (hyp) {
        hh.resize(P * I);
        HIPTRY(s.get(hh.data(), oh, hh.size()));
    }
    if (flags) {
        hf.resize(P * I * W);
        HIPTRY(s.get(hf.data(), of, hf.size()));
    }
    for (size_t p = 0; p < P; p++) {
        const size_t w = ORBH_WORDS(problems[p].n), it = problems[p].iters;
        std::memcpy(best_flags[p], &hb[p * W], w * sizeof(uint64_t));
        std::memcpy(result_flags[p], &ho[p * W], w * sizeof(uint64_t));
        if (hyp && hyp[p]) std::memcpy(hyp[p], &hh[p * I], it * sizeof(orbh_hyp));
        if (flags && flags[p])
            for (size_t i = 0; i < it; i++) std::memcpy(flags[p] + i * w, &hf[(p * I + i) * W], w * sizeof(uint64_t));
    }
    return ORBX_OK;
}

int orbh_iterate(const orbh_problem* problem, const float* x3dc1, const float* x3dc2, const float* p1im1, const float* p2im2, const float* maxerr1,
                 const float* maxerr2, const int32_t* sets, orbh_state* state, uint64_t* best_flags, orbh_result* result, uint64_t* result_flags,
                 orbh_hyp* hyp, uint64_t* flags, int device) {
    if (!problem || !state || !result) return ORBX_ERR_ARG;
    return orbh_iterate_batch(problem, 1, &x3dc1, &x3dc2, &p1im1, &p2im2, &maxerr1, &maxerr2, &sets, state, &best_flags, result, &result_flags,
                              hyp ? &hyp : nullptr, flags ? &flags : nullptr, device);
}

}  // extern "C"
