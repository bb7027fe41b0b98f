// The host route tools/bench_sim3solver.py measures the device chain of the Sim3 RANSAC against: the C ABI of include/orbh.h (its host forms) on one
// host core over the same arithmetic text (orb_slam_amd/csrc/orbh_math.h) with the same double Jacobi iteration (orb_jacobi.h) and the same argument
// checks (orbh_host.h).  tests/test_sim3solver_host.py holds it against the numpy restatement; code written against the library links against this
// file instead and runs on the host.  `device` is ignored.  Build with -ffp-contract=off.
#include <cstring>
#include <vector>

#include "orbh_host.h"
#include "orbh_math.h"

namespace {

using namespace orbh;

// one hypothesis over host arrays: the fit and CheckInliers
void hypothesis(const orbh_problem& q, const float* x3dc1, const float* x3dc2, const float* p1im1, const float* p2im2, const float* maxerr1,
                const float* maxerr2, const int32_t* set, orbh_hyp& h, uint64_t* fl) {
    const int n = q.n, words = ORBH_WORDS(n);
    std::memset(fl, 0, words * sizeof(uint64_t));
    if (set[0] < 0 || set[0] >= n || set[1] < 0 || set[1] >= n || set[2] < 0 || set[2] >= n) {
        void_hyp(h);
        return;
    }
    float pt[3][6];
    for (int j = 0; j < 3; j++)
        for (int r = 0; r < 3; r++) {
            pt[j][r] = x3dc1[(size_t)set[j] * 3 + r];
            pt[j][3 + r] = x3dc2[(size_t)set[j] * 3 + r];
        }
    fit(pt[0], pt[1], pt[2], h);
    int count = 0;
    for (int i = 0; i < n; i++) {
        const float *a = x3dc1 + (size_t)i * 3, *b = x3dc2 + (size_t)i * 3, *u = p1im1 + (size_t)i * 2, *v = p2im2 + (size_t)i * 2;
        if (is_inlier(q, h.T12, h.T21, a[0], a[1], a[2], b[0], b[1], b[2], u[0], u[1], v[0], v[1], maxerr1[i], maxerr2[i])) {
            fl[i / 64] |= (uint64_t)1 << (i % 64);
            count++;
        }
    }
    h.count = count;
}

}  // namespace

extern "C" {

int orbh_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int32_t* max_its_out) {
    if (n < 0 || !max_its_out) return ORBX_ERR_ARG;
    *max_its_out = ransac_parameters(n, probability, min_inliers, max_iterations);
    return ORBX_OK;
}

int orbh_max_errors(int n, const float* sigma2, float* maxerr) {
    if (n < 0 || (n > 0 && (!sigma2 || !maxerr))) return ORBX_ERR_ARG;
    for (int i = 0; i < n; i++) maxerr[i] = max_error(sigma2[i]);
    return ORBX_OK;
}

int orbh_hypotheses(const orbh_problem* problem, const float* x3dc1, const float* x3dc2, const float* p1im1, const float* p2im2, const float* maxerr1,
                    const float* maxerr2, const int32_t* sets, orbh_hyp* hyp, uint64_t* flags, int) {
    if (!problem || check_problem(*problem) != ORBX_OK || !all_set({x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, sets, hyp, flags})) return ORBX_ERR_ARG;
    const size_t W = ORBH_WORDS(problem->n);
    for (int it = 0; it < problem->iters; it++)
        hypothesis(*problem, x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, sets + (size_t)it * 3, hyp[it], flags + it * W);
    return ORBX_OK;
}

int orbh_select(const orbh_problem* problem, const orbh_hyp* hyp, const uint64_t* flags, orbh_state* state, uint64_t* best_flags, orbh_result* result,
                uint64_t* result_flags, int) {
    if (!problem || check_problem(*problem) != ORBX_OK || !all_set({hyp, flags, state, best_flags, result, result_flags})) return ORBX_ERR_ARG;
    if (check_state(*state) != ORBX_OK) return ORBX_ERR_ARG;
    const size_t W = ORBH_WORDS(problem->n);
    std::vector<int32_t> count(problem->iters);
    for (int it = 0; it < problem->iters; it++) count[it] = hyp[it].count;
    const Walk wk = walk(*problem, count.data(), *state, *result);
    if (wk.best_it >= 0) {
        take_best(hyp[wk.best_it], *state, *result);
        std::memcpy(best_flags, flags + wk.best_it * W, W * sizeof(uint64_t));
    }
    if (result->found) std::memcpy(result_flags, best_flags, W * sizeof(uint64_t));
    else std::memset(result_flags, 0, W * sizeof(uint64_t));
    return ORBX_OK;
}

int orbh_iterate(const orbh_problem* problem, const float* x3dc1, const float* x3dc2, const float* p1im1, const float* p2im2, const float* maxerr1,
                 const float* maxerr2, const int32_t* sets, orbh_state* state, uint64_t* best_flags, orbh_result* result, uint64_t* result_flags,
                 orbh_hyp* hyp, uint64_t* flags, int) {
    if (!problem || check_problem(*problem) != ORBX_OK ||
        !all_set({x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, sets, state, best_flags, result, result_flags}))
        return ORBX_ERR_ARG;
    if (check_state(*state) != ORBX_OK) return ORBX_ERR_ARG;
    const size_t I = problem->iters, W = ORBH_WORDS(problem->n);
    std::vector<orbh_hyp> hh(I);
    std::vector<uint64_t> hf(I * W);
    int rc = orbh_hypotheses(problem, x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, sets, hh.data(), hf.data(), 0);
    if (rc != ORBX_OK) return rc;
    rc = orbh_select(problem, hh.data(), hf.data(), state, best_flags, result, result_flags, 0);
    if (rc != ORBX_OK) return rc;
    if (hyp) std::memcpy(hyp, hh.data(), I * sizeof(orbh_hyp));
    if (flags) std::memcpy(flags, hf.data(), I * W * sizeof(uint64_t));
    return ORBX_OK;
}

int orbh_iterate_batch(const orbh_problem* problems, int nproblems, const float* const* x3dc1, const float* const* x3dc2, const float* const* p1im1,
                       const float* const* p2im2, const float* const* maxerr1, const float* const* maxerr2, const int32_t* const* sets,
                       orbh_state* states, uint64_t* const* best_flags, orbh_result* results, uint64_t* const* result_flags, orbh_hyp* const* hyp,
                       uint64_t* const* flags, int) {
    if (!problems || nproblems < 1 || nproblems > ORBH_MAX_PROBLEMS ||
        !all_set({x3dc1, x3dc2, p1im1, p2im2, maxerr1, maxerr2, sets, states, best_flags, results, result_flags}))
        return ORBX_ERR_ARG;
    for (int p = 0; p < nproblems; p++)
        if (check_problem(problems[p]) != ORBX_OK || check_state(states[p]) != ORBX_OK ||
            !all_set({x3dc1[p], x3dc2[p], p1im1[p], p2im2[p], maxerr1[p], maxerr2[p], sets[p], best_flags[p], result_flags[p]}))
            return ORBX_ERR_ARG;
    for (int p = 0; p < nproblems; p++) {
        const int rc = orbh_iterate(problems + p, x3dc1[p], x3dc2[p], p1im1[p], p2im2[p], maxerr1[p], maxerr2[p], sets[p], states + p, best_flags[p],
                                    results + p, result_flags[p], hyp ? hyp[p] : nullptr, flags ? flags[p] : nullptr, 0);
        if (rc != ORBX_OK) return rc;
    }
    return ORBX_OK;
}

}  // extern "C"
