// Loop closing's Sim3 refinement on gfx950: Optimizer::OptimizeSim3 (reference src/Optimizer.cc:789-987) with the Levenberg iteration of g2o and
// its numeric Jacobian behind it.  include/orbg.h is the boundary and states the arithmetic; orbg_math.h holds it, shared with the host.
//
// Kernel:
//   k_sim3_optimize  one workgroup of ONE wave per loop candidate; both phases (5 and then 5 or 10 outer iterations of up to 10 trials each) and
//       both inlier checks inside the one launch.  As in k_pose_optimize a pass over the pairs is lane-strided over the struct-of-arrays pair table,
//       the 64 partial sums meet in an xor butterfly that leaves the same bits in every lane, and every lane runs the 7 x 7 solve and the
//       Levenberg bookkeeping on those bits.
//   The similarities of a linearisation (the estimate, its fourteen perturbations by +-1e-9 and the fifteen inverses edge 21 needs) are the same
//       for every pair.  Lane k < 15 computes slot k and its inverse (one exp each, side by side, instead of fifteen in a row in every lane) and
//       writes both to LDS: 30 x 8 doubles, 1920 bytes.  The build pass reads them back with wave-uniform addresses (broadcast reads), so they
//       cost no VGPR between two edges.  The two barriers around the fill are those of a one-wave workgroup.
//   The build pass takes edge 12 and then edge 21 of a pair through the same text (add_edge): the 2 x 7 Jacobian of ONE edge is live next to the
//       36 running sums, not both.
//   The pair rows are re-read from global memory in every pass (twelve floats per pair, at most 384 KiB per candidate), as k_pose_optimize does.
// No atomics, no inline assembly; registers, scratch and LDS of the kept form are in NOTES.md §37.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "orbg.h"
#include "orbg_host.h"
#include "orbg_math.h"
#include "orbx_host.h"

namespace orbg {

constexpr int SIM3_TPB = LANES;

struct DeviceLoad {
    const float* T;
    int ncap;
    __device__ double at(int r, int i) const { return (double)T[(size_t)r * ncap + i]; }
    __device__ Pair operator()(int i) const {
        Pair P;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            P.P1[r] = at(r, i);
            P.P2[r] = at(3 + r, i);
        }
        P.u1 = at(6, i);
        P.v1 = at(7, i);
        P.w1 = at(8, i);
        P.u2 = at(9, i);
        P.v2 = at(10, i);
        P.w2 = at(11, i);
        return P;
    }
};

// own + partner over the distances 32 .. 1: every lane ends with the same bits
__device__ __forceinline__ double butterfly(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, LANES);
    return v;
}

// a lane's 2 x 7 Jacobian in LDS: entry k of lane l at jac[k*64 + l] (consecutive lanes, consecutive doubles)
struct DeviceJac {
    double* base;
    __device__ void put(int k, double v) { base[k * LANES] = v; }
    __device__ double get(int k) const { return base[k * LANES]; }
};

struct DeviceSys {
    DeviceLoad load;
    Cam c1, c2;
    double delta, dsqr, th2;
    int n, lane;
    Flags f;                                                                        // pairs the first check removed
    uint64_t* out;
    orbo_step* tr;
    Sim3* sims;                                                                     // LDS: 2*NSIM
    DeviceJac jac;
    __device__ void linearise(const Sim3& S) {
        __syncthreads();                                                            // the last pass has read the previous slots
        if (lane < NSIM) {
            Sim3 P, Pi;
            perturbed(S, lane, P);
            sim3_inverse(P, Pi);
            sims[lane] = P;
            sims[NSIM + lane] = Pi;
        }
        __syncthreads();
    }
    __device__ void full(double (&acc)[NACC]) {
        lane_full(load, sims, c1, c2, delta, dsqr, n, lane, f, jac, acc);
#pragma unroll
        for (int a = 0; a < NACC; a++) acc[a] = butterfly(acc[a]);
    }
    __device__ double chi(const Sim3& S, const Sim3& Si) { return butterfly(lane_chi(load, S, Si, c1, c2, delta, dsqr, n, lane, f)); }
    __device__ int check(const Sim3& last, const Sim3& lasti, bool first) {
        int nbad = 0;
        for (int base = 0, k = 0; base < n; base += LANES, k++) {
            const int i = base + lane;
            bool removed = false, bad = false;
            if (i < n) {
                removed = f.get(k);
                if (!removed) bad = pair_is_bad(load, last, lasti, c1, c2, th2, i);
                if (first && bad) f.set(k, true);
            }
            const unsigned long long mr = __ballot(removed || bad), mb = __ballot(bad);     // bit l = lane l = pair base + l
            if (lane == 0) out[k] = mr;
            nbad += __popcll(mb);
        }
        return nbad;
    }
    __device__ double u(double v) const {
        const uint64_t b = __double_as_longlong(v);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b), hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
        return __longlong_as_double(((uint64_t)hi << 32) | lo);
    }
    __device__ void step(int slot, const orbo_step& s) {
        if (tr && lane == 0) tr[slot] = s;
    }
};

__global__ __launch_bounds__(SIM3_TPB, 1) void k_sim3_optimize(Problems PR, const float* pairs, int ncap, const float* S12, orbg_result* result,
                                                            uint64_t* removed, orbo_step* trace) {
    __shared__ Sim3 sims[2 * NSIM];
    __shared__ double jac[2 * DIM * LANES];
    const int p = blockIdx.x;
    const orbg_problem& q = PR.p[p];
    DeviceSys sys;
    sys.load = {pairs + (size_t)p * ORBG_PAIR_ROWS * ncap, ncap};
    sys.c1 = {(double)q.fx1, (double)q.fy1, (double)q.cx1, (double)q.cy1};
    sys.c2 = {(double)q.fx2, (double)q.fy2, (double)q.cx2, (double)q.cy2};
    sys.th2 = (double)q.th2;
    sys.delta = (double)(float)sqrt((double)q.th2);                                 // Optimizer.cc:840
    sys.dsqr = (double)(float)(sys.delta * sys.delta);
    sys.n = q.n;
    sys.lane = threadIdx.x;
    sys.out = removed + (size_t)p * ORBO_WORDS(ncap);
    sys.tr = trace ? trace + (size_t)p * ORBG_MAX_ITERS : nullptr;
    sys.sims = sims;
    sys.jac = {jac + threadIdx.x};
    orbg_result res;
    optimize_sim3(sys, q.n, S12 + (size_t)p * 13, res);
    if (sys.lane == 0) result[p] = res;
}

}  // namespace orbg

extern "C" {

int orbg_sim3_batch_device(const orbg_problem* problems, int nproblems, const float* d_pairs, int ncap, const float* d_S12, orbg_result* d_result,
                           uint64_t* d_removed, orbo_step* d_trace, void* stream) {
    orbg::Problems PR;
    TRY(orbg::check_batch(problems, nproblems, ncap, PR));
    if (!orbg::all_set({d_pairs, d_S12, d_result, d_removed})) return ORBX_ERR_ARG;
    hipLaunchKernelGGL(orbg::k_sim3_optimize, dim3(nproblems), dim3(orbg::SIM3_TPB), 0, (hipStream_t)stream, PR, d_pairs, ncap, d_S12, d_result, d_removed,
                       d_trace);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbg_sim3_batch(const orbg_problem* problems, int nproblems, const float* const* P1c, const float* const* P2c, const float* const* obs1,
                    const float* const* obs2, const float* S12, orbg_result* results, uint64_t* const* removed, orbo_step* const* trace, int device) {
    if (!problems || nproblems < 1 || nproblems > ORBG_MAX_PROBLEMS || !orbg::all_set({P1c, P2c, obs1, obs2, S12, results, removed})) return ORBX_ERR_ARG;
    size_t N = 1;
    for (int p = 0; p < nproblems; p++) {
        if (orbg::check_candidate(problems[p], P1c[p], P2c[p], obs1[p], obs2[p], removed[p]) != ORBX_OK) return ORBX_ERR_ARG;
        N = std::max(N, (size_t)problems[p].n);
    }
    // the candidates' arrays packed to the shared cap N
    const size_t P = nproblems, W = ORBO_WORDS(N);
    std::vector<float> hp(P * ORBG_PAIR_ROWS * N);
    for (size_t p = 0; p < P; p++) orbg::pack_pairs(problems[p].n, (int)N, P1c[p], P2c[p], obs1[p], obs2[p], &hp[p * ORBG_PAIR_ROWS * N]);
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto ip = s.in(hp.data(), hp.size());
    const auto is = s.in(S12, P * 13);
    const auto orr = s.out<orbg_result>(P);
    const auto of = s.out<uint64_t>(P * W);
    const auto ot = s.out<orbo_step>(trace ? P * ORBG_MAX_ITERS : 0);
    HIPTRY(s.alloc());
    TRY(orbg_sim3_batch_device(problems, nproblems, s[ip], (int)N, s[is], s[orr], s[of], trace ? s[ot] : nullptr, nullptr));
    std::vector<uint64_t> hf(P * W);
    std::vector<orbo_step> ht;
    HIPTRY(s.get(results, orr, P));
    HIPTRY(s.get(hf.data(), of, hf.size()));
    if (trace) {
        ht.resize(P * ORBG_MAX_ITERS);
        HIPTRY(s.get(ht.data(), ot, ht.size()));
    }
    for (size_t p = 0; p < P; p++) {
        if (problems[p].n > 0) std::memcpy(removed[p], &hf[p * W], ORBO_WORDS(problems[p].n) * sizeof(uint64_t));
        if (trace && trace[p]) std::memcpy(trace[p], &ht[p * ORBG_MAX_ITERS], ORBG_MAX_ITERS * sizeof(orbo_step));
    }
    return ORBX_OK;
}

int orbg_sim3(const orbg_problem* problem, const float* P1c, const float* P2c, const float* obs1, const float* obs2, const float* S12,
              orbg_result* result, uint64_t* removed, orbo_step* trace, int device) {
    if (!problem || !result) return ORBX_ERR_ARG;
    return orbg_sim3_batch(problem, 1, &P1c, &P2c, &obs1, &obs2, S12, result, &removed, trace ? &trace : nullptr, device);
}

}  // extern "C"
