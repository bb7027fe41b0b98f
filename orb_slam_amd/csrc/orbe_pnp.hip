// The EPnP RANSAC of the relocalisation on gfx950: PnPsolver::iterate / Refine / CheckInliers and compute_pose with everything below it (reference
// src/PnPsolver.cc:166-340, :376-951).  include/orbe.h is the boundary and states the arithmetic; orbe_math.h holds it, shared with the host.
//
// Kernels:
//   k_pnp_hypotheses  one workgroup of ONE wave per (iteration, problem): up to 300 waves per solver, bound by the latency of the dependent
//       rotations of the 12 x 12 Jacobi iteration (M'M and V in LDS, lane k owns row k: orbj::sym_eig_wave<12>).  The sums over the set are the
//       partial sums of orbe.h, of which four are not zero and are kept (orbe::Work4); lanes 0-2 take the three beta branches; then the lanes stride over the N
//       correspondences for the inlier test, the count is a sum of ballots.
//   k_pnp_refine      one workgroup of four waves per (iteration, problem).  It leaves at once unless its iteration is a record.  Wave 0 packs the
//       flagged correspondences into an index list in LDS in index order (ballot prefix), the fit is the same text with n = the length of
//       the list (wave 0 carries the partial sums, the 12 x 12 rotations use threads 0-12), all four waves test the N correspondences.
//   k_pnp_select      one workgroup per problem: thread 0 walks the counts, the workgroup copies the chosen flags.
// No floating-point atomics anywhere; the counts are integer sums.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbe.h"
#include "orbe_host.h"
#include "orbe_math.h"
#include "orbx_host.h"

namespace orbe {

constexpr int HYP_TPB = 64;
constexpr int REF_TPB = 256;
constexpr int SEL_TPB = 256;

struct DevCx {
    int tid, stride;
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void eig12(double* S, double* V) { orbj::sym_eig_wave<12>(S, V, tid); }
};

// the fit's results of one workgroup, in LDS until every thread has them
struct Pose { double R[9], t[3], err[3]; int32_t branch; };

__device__ __forceinline__ Cam cam_of(const orbe_problem& q) { return Cam{(double)q.fu, (double)q.fv, (double)q.uc, (double)q.vc}; }

// CheckInliers over the n correspondences by the whole workgroup; *total (LDS, zero on entry) ends as the count after the barrier
__device__ __forceinline__ void check_inliers(const Cam& cam, const Pose& pose, const float* p3d, const float* p2d, const float* maxerr, int n, uint8_t* flags,
                                              int* total, int tid, int tpb) {
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = pose.R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = pose.t[i];
    int mine = 0;
    for (int base = 0; base < n; base += tpb) {
        const int i = base + tid;
        bool in = false;
        if (i < n) {
            in = is_inlier(cam, R, t, p3d + (size_t)i * 3, p2d + (size_t)i * 2, maxerr[i]);
            flags[i] = in ? 1 : 0;
        }
        mine += __popcll(__ballot(in));                      // the wave's count, the same in every lane
    }
    if ((tid & 63) == 0) atomicAdd(total, mine);             // an integer sum of one value per wave
    __syncthreads();
}

// a fit that cannot run: NaN pose and errors, branch 0, count 0, zero flags
__device__ __forceinline__ void write_void(double* R, double* t, double* err, int32_t* branch, double* vecs, int32_t* count, uint8_t* flags, int n, int tid,
                                           int tpb) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (tid < 9) R[tid] = nan;
    if (tid < 3) t[tid] = nan;
    if (tid < 3 && err) err[tid] = nan;
    if (tid == 0) {
        if (branch) *branch = 0;
        *count = 0;
    }
    if (vecs)
        for (int e = tid; e < 48; e += tpb) vecs[e] = nan;
    for (int i = tid; i < n; i += tpb) flags[i] = 0;
}

__global__ __launch_bounds__(HYP_TPB) void k_pnp_hypotheses(Problems PR, const float* p3d_all, const float* p2d_all, const float* maxerr_all, int ncap,
                                                            const int32_t* sets, int icap, double* R, double* t, double* err, int32_t* branch, double* vecs,
                                                            int32_t* count, uint8_t* flags) {
#if defined(ORBE_PART64)                                               // measurement aid (NOTES §32): the work arrays sized as Refine's
    __shared__ Work w;
#else
    __shared__ Work4 w;
#endif
    __shared__ Pose pose;
    __shared__ uint16_t list[4];
    __shared__ int total;
    const int it = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const orbe_problem& q = PR.p[p];
    if (it >= q.iters) return;
    const int n = q.n;
    const size_t s = (size_t)p * icap + it;
    const float* p3d = p3d_all + (size_t)p * ncap * 3;
    const float* p2d = p2d_all + (size_t)p * ncap * 2;
    const float* maxerr = maxerr_all + (size_t)p * ncap;
    uint8_t* fl = flags + s * ncap;
    double* vout = vecs ? vecs + s * 48 : nullptr;
    const int i0 = sets[s * 4], i1 = sets[s * 4 + 1], i2 = sets[s * 4 + 2], i3 = sets[s * 4 + 3];
    if (i0 < 0 || i0 >= n || i1 < 0 || i1 >= n || i2 < 0 || i2 >= n || i3 < 0 || i3 >= n) {          // uniform
        write_void(R + s * 9, t + s * 3, err + s * 3, branch + s, vout, count + s, fl, n, tid, HYP_TPB);
        return;
    }
    if (tid == 0) {
        list[0] = (uint16_t)i0; list[1] = (uint16_t)i1; list[2] = (uint16_t)i2; list[3] = (uint16_t)i3;
        total = 0;
    }
    __syncthreads();
    const Cam cam = cam_of(q);
    const Points P = {p3d, p2d, list, 4};
    DevCx cx = {tid, HYP_TPB};
    fit(cx, w, cam, P, pose.R, pose.t, pose.err, &pose.branch, vout);
    if (tid < 9) R[s * 9 + tid] = pose.R[tid];
    if (tid < 3) {
        t[s * 3 + tid] = pose.t[tid];
        err[s * 3 + tid] = pose.err[tid];
    }
    if (tid == 0) branch[s] = pose.branch;
    check_inliers(cam, pose, p3d, p2d, maxerr, n, fl, &total, tid, HYP_TPB);
    if (tid == 0) count[s] = total;
}

// planted = 0: Refine of the records over the flags of the hypotheses; planted = 1: the fit of every slot over flags_in
__global__ __launch_bounds__(REF_TPB) void k_pnp_refine(Problems PR, int planted, const float* p3d_all, const float* p2d_all, const float* maxerr_all, int ncap,
                                                        int icap, const int32_t* count, const uint8_t* flags_in, const orbe_state* state, double* rR,
                                                        double* rt, double* rvecs, int32_t* rcount, uint8_t* rflags, int32_t* rok) {
    __shared__ Work w;
    __shared__ Pose pose;
    __shared__ uint16_t list[ORBE_MAX_POINTS];
    __shared__ int total, nsel, beaten;
    const int it = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const orbe_problem& q = PR.p[p];
    if (it >= q.iters) return;
    const int n = q.n;
    const size_t s = (size_t)p * icap + it;
    if (tid == 0) { total = 0; nsel = 0; beaten = 0; }
    __syncthreads();
    if (!planted) {
        const int32_t* cnt = count + (size_t)p * icap;
        const int c = cnt[it];
        if (c < q.min_inliers || c <= state[p].best_inliers) return;                                 // uniform
        for (int j = tid; j < it; j += REF_TPB)
            if (cnt[j] >= c) beaten = 1;                                                             // every writer stores the same value
        __syncthreads();
        if (beaten) return;
    }
    const float* p3d = p3d_all + (size_t)p * ncap * 3;
    const float* p2d = p2d_all + (size_t)p * ncap * 2;
    const float* maxerr = maxerr_all + (size_t)p * ncap;
    const uint8_t* fin = flags_in + s * ncap;
    uint8_t* fl = rflags + s * ncap;
    double* vout = rvecs ? rvecs + s * 48 : nullptr;
    if (tid < 64) {                                                                                 // wave 0: the flagged indices in index order
        int have = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + tid;
            const bool f = i < n && fin[i] != 0;
            const unsigned long long m = __ballot(f);
            if (f) list[have + __popcll(m & ((1ull << tid) - 1ull))] = (uint16_t)i;
            have += __popcll(m);
        }
        if (tid == 0) nsel = have;
    }
    __syncthreads();
    const int nfit = nsel;
    if (nfit < 4) {                                                                                  // uniform; planted arrays only
        write_void(rR + s * 9, rt + s * 3, nullptr, nullptr, vout, rcount + s, fl, n, tid, REF_TPB);
        if (tid == 0) rok[s] = 0;
        return;
    }
    const Cam cam = cam_of(q);
    const Points P = {p3d, p2d, list, nfit};
    DevCx cx = {tid, REF_TPB};
    fit(cx, w, cam, P, pose.R, pose.t, pose.err, &pose.branch, vout);
    if (tid < 9) rR[s * 9 + tid] = pose.R[tid];
    if (tid < 3) rt[s * 3 + tid] = pose.t[tid];
    check_inliers(cam, pose, p3d, p2d, maxerr, n, fl, &total, tid, REF_TPB);
    if (tid == 0) {
        rcount[s] = total;
        rok[s] = total > q.min_inliers ? 1 : 0;
    }
}

__global__ __launch_bounds__(SEL_TPB) void k_pnp_select(Problems PR, int ncap, int icap, const double* R, const double* t, const int32_t* count,
                                                        const uint8_t* flags, const double* rR, const double* rt, const int32_t* rcount,
                                                        const uint8_t* rflags, const int32_t* rok, orbe_state* state, uint8_t* best_flags,
                                                        uint8_t* refined_flags, orbe_result* result, uint8_t* result_flags) {
    __shared__ Walk wk;
    __shared__ int kind;
    const int p = blockIdx.x, tid = threadIdx.x;
    const orbe_problem& q = PR.p[p];
    const size_t base = (size_t)p * icap;
    if (tid == 0) {
        orbe_state st = state[p];
        orbe_result res;
        wk = walk(q, R + base * 9, t + base * 3, count + base, rR + base * 9, rt + base * 3, rcount + base, rok + base, st, res);
        kind = res.kind;
        state[p] = st;
        result[p] = res;
    }
    __syncthreads();
    const int best_it = wk.best_it, k = kind;
    uint8_t* bf = best_flags + (size_t)p * ncap;
    uint8_t* rf = refined_flags + (size_t)p * ncap;
    uint8_t* of = result_flags + (size_t)p * ncap;
    for (int i = tid; i < q.n; i += SEL_TPB) {
        uint8_t b = bf[i], r = rf[i];
        if (best_it >= 0) {
            b = flags[(base + best_it) * ncap + i];
            r = rflags[(base + best_it) * ncap + i];
            bf[i] = b;
            rf[i] = r;
        }
        of[i] = k == ORBE_KIND_REFINED ? r : k == ORBE_KIND_BEST ? b : 0;
    }
}

}  // namespace orbe

extern "C" {

int orbe_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2, const float* sigma2,
                           int32_t* min_inliers_out, int32_t* max_its_out, float* epsilon_out, float* maxerr) {
    if (n < 1 || !sigma2 || !min_inliers_out || !max_its_out || !epsilon_out || !maxerr) return ORBX_ERR_ARG;
    orbe::ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon, th2, sigma2, min_inliers_out, max_its_out, epsilon_out, maxerr);
    return ORBX_OK;
}

int orbe_hypotheses_batch_device(const orbe_problem* problems, int nproblems, const float* d_p3d, const float* d_p2d, const float* d_maxerr, int ncap,
                                 const int32_t* d_sets, int icap, double* d_R, double* d_t, double* d_err, int32_t* d_branch, double* d_vecs,
                                 int32_t* d_count, uint8_t* d_flags, void* stream) {
    orbe::Problems PR;
    int iters = 0;
    TRY(orbe::check_batch(problems, nproblems, ncap, icap, PR, iters));
    if (!orbe::all_set({d_p3d, d_p2d, d_maxerr, d_sets, d_R, d_t, d_err, d_branch, d_count, d_flags})) return ORBX_ERR_ARG;
    hipLaunchKernelGGL(orbe::k_pnp_hypotheses, dim3(iters, nproblems), dim3(orbe::HYP_TPB), 0, (hipStream_t)stream, PR, d_p3d, d_p2d, d_maxerr, ncap, d_sets,
                       icap, d_R, d_t, d_err, d_branch, d_vecs, d_count, d_flags);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbe_refine_batch_device(const orbe_problem* problems, int nproblems, const float* d_p3d, const float* d_p2d, const float* d_maxerr, int ncap,
                             int icap, const int32_t* d_count, const uint8_t* d_flags, const orbe_state* d_state, double* d_rR, double* d_rt,
                             int32_t* d_rcount, uint8_t* d_rflags, int32_t* d_rok, void* stream) {
    orbe::Problems PR;
    int iters = 0;
    TRY(orbe::check_batch(problems, nproblems, ncap, icap, PR, iters));
    if (!orbe::all_set({d_p3d, d_p2d, d_maxerr, d_count, d_flags, d_state, d_rR, d_rt, d_rcount, d_rflags, d_rok})) return ORBX_ERR_ARG;
    hipLaunchKernelGGL(orbe::k_pnp_refine, dim3(iters, nproblems), dim3(orbe::REF_TPB), 0, (hipStream_t)stream, PR, 0, d_p3d, d_p2d, d_maxerr, ncap, icap,
                       d_count, d_flags, d_state, d_rR, d_rt, (double*)nullptr, d_rcount, d_rflags, d_rok);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbe_refit_batch_device(const orbe_problem* problems, int nproblems, const float* d_p3d, const float* d_p2d, const float* d_maxerr, int ncap, int icap,
                            const uint8_t* d_flags_in, double* d_rR, double* d_rt, double* d_rvecs, int32_t* d_rcount, uint8_t* d_rflags, int32_t* d_rok,
                            void* stream) {
    orbe::Problems PR;
    int iters = 0;
    TRY(orbe::check_batch(problems, nproblems, ncap, icap, PR, iters));
    if (!orbe::all_set({d_p3d, d_p2d, d_maxerr, d_flags_in, d_rR, d_rt, d_rcount, d_rflags, d_rok})) return ORBX_ERR_ARG;
    hipLaunchKernelGGL(orbe::k_pnp_refine, dim3(iters, nproblems), dim3(orbe::REF_TPB), 0, (hipStream_t)stream, PR, 1, d_p3d, d_p2d, d_maxerr, ncap, icap,
                       (const int32_t*)nullptr, d_flags_in, (const orbe_state*)nullptr, d_rR, d_rt, d_rvecs, d_rcount, d_rflags, d_rok);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbe_select_batch_device(const orbe_problem* problems, int nproblems, int ncap, int icap, const double* d_R, const double* d_t, const int32_t* d_count,
                             const uint8_t* d_flags, const double* d_rR, const double* d_rt, const int32_t* d_rcount, const uint8_t* d_rflags,
                             const int32_t* d_rok, orbe_state* d_state, uint8_t* d_best_flags, uint8_t* d_refined_flags, orbe_result* d_result,
                             uint8_t* d_result_flags, void* stream) {
    orbe::Problems PR;
    int iters = 0;
    TRY(orbe::check_batch(problems, nproblems, ncap, icap, PR, iters));
    if (!orbe::all_set({d_R, d_t, d_count, d_flags, d_rR, d_rt, d_rcount, d_rflags, d_rok, d_state, d_best_flags, d_refined_flags, d_result, d_result_flags}))
        return ORBX_ERR_ARG;
    hipLaunchKernelGGL(orbe::k_pnp_select, dim3(nproblems), dim3(orbe::SEL_TPB), 0, (hipStream_t)stream, PR, ncap, icap, d_R, d_t, d_count, d_flags, d_rR, d_rt,
                       d_rcount, d_rflags, d_rok, d_state, d_best_flags, d_refined_flags, d_result, d_result_flags);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbe_hypotheses(const orbe_problem* problem, const float* p3d, const float* p2d, const float* maxerr, const int32_t* sets, double* R, double* t,
                    double* err, int32_t* branch, double* vecs, int32_t* count, uint8_t* flags, int device) {
    if (!problem || orbe::check_problem(*problem) != ORBX_OK || !orbe::all_set({p3d, p2d, maxerr, sets, R, t, err, branch, count, flags})) return ORBX_ERR_ARG;
    const size_t N = problem->n, I = problem->iters;
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto a3 = s.in(p3d, N * 3), a2 = s.in(p2d, N * 2), am = s.in(maxerr, N);
    const auto st = s.in(sets, I * 4);
    const auto oR = s.out<double>(I * 9), ot = s.out<double>(I * 3), oe = s.out<double>(I * 3), ov = s.out<double>(I * 48);
    const auto ob = s.out<int32_t>(I), oc = s.out<int32_t>(I);
    const auto of = s.out<uint8_t>(I * N);
    HIPTRY(s.alloc());
    TRY(orbe_hypotheses_batch_device(problem, 1, s[a3], s[a2], s[am], (int)N, s[st], (int)I, s[oR], s[ot], s[oe], s[ob], vecs ? s[ov] : nullptr, s[oc], s[of],
                                     nullptr));
    HIPTRY(s.get(R, oR, I * 9));
    HIPTRY(s.get(t, ot, I * 3));
    HIPTRY(s.get(err, oe, I * 3));
    HIPTRY(s.get(branch, ob, I));
    if (vecs) HIPTRY(s.get(vecs, ov, I * 48));
    HIPTRY(s.get(count, oc, I));
    HIPTRY(s.get(flags, of, I * N));
    return ORBX_OK;
}

int orbe_refine(const orbe_problem* problem, const float* p3d, const float* p2d, const float* maxerr, const int32_t* count, const uint8_t* flags, int best_in,
                double* rR, double* rt, int32_t* rcount, uint8_t* rflags, int32_t* rok, int device) {
    if (!problem || orbe::check_problem(*problem) != ORBX_OK || best_in < 0 || !orbe::all_set({p3d, p2d, maxerr, count, flags, rR, rt, rcount, rflags, rok}))
        return ORBX_ERR_ARG;
    const size_t N = problem->n, I = problem->iters;
    orbe_state state;
    std::memset(&state, 0, sizeof(state));
    state.best_inliers = best_in;
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto a3 = s.in(p3d, N * 3), a2 = s.in(p2d, N * 2), am = s.in(maxerr, N);
    const auto ic = s.in(count, I);
    const auto jf = s.in(flags, I * N);
    const auto is = s.in(&state, 1);
    // the outputs start as the caller's arrays: what is not a record is left alone
    const auto oR = s.in(rR, I * 9), ot = s.in(rt, I * 3);
    const auto oc = s.in(rcount, I), ok = s.in(rok, I);
    const auto of = s.in(rflags, I * N);
    HIPTRY(s.alloc());
    TRY(orbe_refine_batch_device(problem, 1, s[a3], s[a2], s[am], (int)N, (int)I, s[ic], s[jf], s[is], s[oR], s[ot], s[oc], s[of], s[ok], nullptr));
    HIPTRY(s.get(rR, oR, I * 9));
    HIPTRY(s.get(rt, ot, I * 3));
    HIPTRY(s.get(rcount, oc, I));
    HIPTRY(s.get(rflags, of, I * N));
    HIPTRY(s.get(rok, ok, I));
    return ORBX_OK;
}

int orbe_refit(const orbe_problem* problem, const float* p3d, const float* p2d, const float* maxerr, const uint8_t* flags_in, double* rR, double* rt,
               double* rvecs, int32_t* rcount, uint8_t* rflags, int32_t* rok, int device) {
    if (!problem || orbe::check_problem(*problem) != ORBX_OK || !orbe::all_set({p3d, p2d, maxerr, flags_in, rR, rt, rcount, rflags, rok})) return ORBX_ERR_ARG;
    const size_t N = problem->n, I = problem->iters;
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto a3 = s.in(p3d, N * 3), a2 = s.in(p2d, N * 2), am = s.in(maxerr, N);
    const auto jf = s.in(flags_in, I * N);
    const auto oR = s.out<double>(I * 9), ot = s.out<double>(I * 3), ov = s.out<double>(I * 48);
    const auto oc = s.out<int32_t>(I), ok = s.out<int32_t>(I);
    const auto of = s.out<uint8_t>(I * N);
    HIPTRY(s.alloc());
    TRY(orbe_refit_batch_device(problem, 1, s[a3], s[a2], s[am], (int)N, (int)I, s[jf], s[oR], s[ot], rvecs ? s[ov] : nullptr, s[oc], s[of], s[ok], nullptr));
    HIPTRY(s.get(rR, oR, I * 9));
    HIPTRY(s.get(rt, ot, I * 3));
    if (rvecs) HIPTRY(s.get(rvecs, ov, I * 48));
    HIPTRY(s.get(rcount, oc, I));
    HIPTRY(s.get(rflags, of, I * N));
    HIPTRY(s.get(rok, ok, I));
    return ORBX_OK;
}

int orbe_select(const orbe_problem* problem, const double* R, const double* t, const int32_t* count, const uint8_t* flags, const double* rR, const double* rt,
                const int32_t* rcount, const uint8_t* rflags, const int32_t* rok, orbe_state* state, uint8_t* best_flags, uint8_t* refined_flags,
                orbe_result* result, uint8_t* result_flags, int device) {
    if (!problem || orbe::check_problem(*problem) != ORBX_OK ||
        !orbe::all_set({R, t, count, flags, rR, rt, rcount, rflags, rok, state, best_flags, refined_flags, result, result_flags}))
        return ORBX_ERR_ARG;
    TRY(orbe::check_state(*state));
    const size_t N = problem->n, I = problem->iters;
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto iR = s.in(R, I * 9), it = s.in(t, I * 3);
    const auto ic = s.in(count, I);
    const auto jf = s.in(flags, I * N);
    const auto jR = s.in(rR, I * 9), jt = s.in(rt, I * 3);
    const auto jc = s.in(rcount, I), jk = s.in(rok, I);
    const auto kf = s.in(rflags, I * N);
    const auto is = s.in(state, 1);
    const auto bf = s.in(best_flags, N), rf = s.in(refined_flags, N);
    const auto orr = s.out<orbe_result>(1);
    const auto of = s.out<uint8_t>(N);
    HIPTRY(s.alloc());
    TRY(orbe_select_batch_device(problem, 1, (int)N, (int)I, s[iR], s[it], s[ic], s[jf], s[jR], s[jt], s[jc], s[kf], s[jk], s[is], s[bf], s[rf], s[orr], s[of],
                                 nullptr));
    HIPTRY(s.get(state, is, 1));
    HIPTRY(s.get(best_flags, bf, N));
    HIPTRY(s.get(refined_flags, rf, N));
    HIPTRY(s.get(result, orr, 1));
    HIPTRY(s.get(result_flags, of, N));
    return ORBX_OK;
}

int orbe_iterate_batch(const orbe_problem* problems, int nproblems, const float* const* p3d, const float* const* p2d, const float* const* maxerr,
                       const int32_t* const* sets, orbe_state* states, uint8_t* const* best_flags, uint8_t* const* refined_flags, orbe_result* results,
                       uint8_t* const* result_flags, int device) {
    if (!problems || nproblems < 1 || nproblems > ORBE_MAX_PROBLEMS ||
        !orbe::all_set({p3d, p2d, maxerr, sets, states, best_flags, refined_flags, results, result_flags}))
        return ORBX_ERR_ARG;
    size_t N = 0, I = 0;
    for (int p = 0; p < nproblems; p++) {
        if (orbe::check_problem(problems[p]) != ORBX_OK || orbe::check_state(states[p]) != ORBX_OK ||
            !orbe::all_set({p3d[p], p2d[p], maxerr[p], sets[p], best_flags[p], refined_flags[p], result_flags[p]}))
            return ORBX_ERR_ARG;
        N = std::max(N, (size_t)problems[p].n);
        I = std::max(I, (size_t)problems[p].iters);
    }
    // the solvers' arrays packed to the shared caps N, I
    const size_t P = nproblems;
    std::vector<float> h3(P * N * 3), h2(P * N * 2), hm(P * N);
    std::vector<int32_t> hs(P * I * 4);
    std::vector<uint8_t> hb(P * N), hr(P * N);
    for (size_t p = 0; p < P; p++) {
        const size_t n = problems[p].n, it = problems[p].iters;
        std::memcpy(&h3[p * N * 3], p3d[p], n * 3 * sizeof(float));
        std::memcpy(&h2[p * N * 2], p2d[p], n * 2 * sizeof(float));
        std::memcpy(&hm[p * N], maxerr[p], n * sizeof(float));
        std::memcpy(&hs[p * I * 4], sets[p], it * 4 * sizeof(int32_t));
        std::memcpy(&hb[p * N], best_flags[p], n);
        std::memcpy(&hr[p * N], refined_flags[p], n);
    }
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto a3 = s.in(h3.data(), h3.size()), a2 = s.in(h2.data(), h2.size()), am = s.in(hm.data(), hm.size());
    const auto st = s.in(hs.data(), hs.size());
    const auto is = s.in(states, P);
    const auto bf = s.in(hb.data(), hb.size()), rf = s.in(hr.data(), hr.size());
    const auto oR = s.out<double>(P * I * 9), ot = s.out<double>(P * I * 3), oe = s.out<double>(P * I * 3);
    const auto ob = s.out<int32_t>(P * I), oc = s.out<int32_t>(P * I);
    const auto of = s.out<uint8_t>(P * I * N);
    const auto jR = s.out<double>(P * I * 9), jt = s.out<double>(P * I * 3);
    const auto jc = s.out<int32_t>(P * I), jk = s.out<int32_t>(P * I);
    const auto kf = s.out<uint8_t>(P * I * N);
    const auto orr = s.out<orbe_result>(P);
    const auto rfl = s.out<uint8_t>(P * N);
    HIPTRY(s.alloc());
    const int nc = (int)N, ic = (int)I;
    TRY(orbe_hypotheses_batch_device(problems, nproblems, s[a3], s[a2], s[am], nc, s[st], ic, s[oR], s[ot], s[oe], s[ob], nullptr, s[oc], s[of], nullptr));
    TRY(orbe_refine_batch_device(problems, nproblems, s[a3], s[a2], s[am], nc, ic, s[oc], s[of], s[is], s[jR], s[jt], s[jc], s[kf], s[jk], nullptr));
    TRY(orbe_select_batch_device(problems, nproblems, nc, ic, s[oR], s[ot], s[oc], s[of], s[jR], s[jt], s[jc], s[kf], s[jk], s[is], s[bf], s[rf], s[orr], s[rfl],
                                 nullptr));
    std::vector<uint8_t> ho(P * N);
    HIPTRY(s.get(states, is, P));
    HIPTRY(s.get(hb.data(), bf, hb.size()));
    HIPTRY(s.get(hr.data(), rf, hr.size()));
    HIPTRY(s.get(results, orr, P));
    HIPTRY(s.get(ho.data(), rfl, ho.size()));
    for (size_t p = 0; p < P; p++) {
        const size_t n = problems[p].n;
        std::memcpy(best_flags[p], &hb[p * N], n);
        std::memcpy(refined_flags[p], &hr[p * N], n);
        std::memcpy(result_flags[p], &ho[p * N], n);
    }
    return ORBX_OK;
}

int orbe_iterate(const orbe_problem* problem, const float* p3d, const float* p2d, const float* maxerr, const int32_t* sets, orbe_state* state,
                 uint8_t* best_flags, uint8_t* refined_flags, orbe_result* result, uint8_t* result_flags, int device) {
    if (!problem || !state || !result) return ORBX_ERR_ARG;
    return orbe_iterate_batch(problem, 1, &p3d, &p2d, &maxerr, &sets, state, &best_flags, &refined_flags, result, &result_flags, device);
}

}  // extern "C"
