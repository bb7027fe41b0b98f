// Tracking's motion-only pose optimisation on gfx950: Optimizer::PoseOptimization (reference src/Optimizer.cc:154-285) with the Levenberg
// iteration of g2o behind it.  include/orbo.h is the boundary and states the arithmetic; orbo_math.h holds it, shared with the host.
//
// Kernel:
//   k_pose_optimize  one workgroup of ONE wave per frame; all four rounds, up to 32 outer iterations of up to 10 trials each, inside the one
//       launch.  A pass over the edges is lane-strided over the struct-of-arrays edge table (consecutive lanes, consecutive floats): the build
//       pass accumulates the 21 upper entries of H, the 6 of b and the chi2 as 28 doubles in registers, the trial pass the chi2 alone, and the
//       64 partial sums meet in an xor butterfly (__shfl_xor on the halves of each double) that leaves the same bits in every lane.  EVERY lane
//       then runs the 6 x 6 solve, exp and the Levenberg bookkeeping on those bits (k_sim3_hypotheses's choice): it costs the wave what one
//       lane would cost it and needs no LDS, no barrier and no broadcast.  A lane keeps the outlier flags of its own edges in two 64-bit
//       registers (8192 / 64 = 128 edges per lane); the words leave by __ballot, written by lane 0.
//   The edge rows are RE-READ from global memory in every pass (six floats per edge; a frame's table is at most 192 KiB and stays in L2)
//       instead of being kept in registers.  Both forms were built and priced (NOTES.md §35): eight edges per lane in registers (48 more
//       registers, frames of at most 512 edges, so a second kernel next to this one) ran the kernel 5 % faster at 100 edges, 13 % at 300 and
//       17 % at 512.  One kernel for every n was kept: what the wave waits on is the serial Levenberg step between two passes (about 700
//       dependent double operations), not the six loads of a pass, which the strided loop issues back to back.
//   Registers: the values every lane holds alike and that live long (the estimate, the last trial, x, H, b, lambda) are named uniform with
//       readfirstlane (Sys::u) and wait in scalar registers while the lanes walk the edges.  The kernel still takes 198 VGPRs and no scratch:
//       at 128 the compiler spills inside the build pass (28 double sums, the Jacobian and the expanded double divisions of one edge are live
//       together).  With one wave per frame and at most 64 frames per call occupancy is not what limits this kernel, so the bound asks for two
//       waves per SIMD and no more.
// No atomics, no scratch, no LDS, no inline assembly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "orbo.h"
#include "orbo_host.h"
#include "orbo_math.h"
#include "orbx_host.h"

namespace orbo {

constexpr int POSE_TPB = LANES;

struct DeviceLoad {
    const float* T;
    int ncap;
    __device__ Edge operator()(int i) const {
        Edge e;
        e.X = (double)T[i];
        e.Y = (double)T[(size_t)ncap + i];
        e.Z = (double)T[(size_t)2 * ncap + i];
        e.u = (double)T[(size_t)3 * ncap + i];
        e.v = (double)T[(size_t)4 * ncap + i];
        e.w = (double)T[(size_t)5 * ncap + i];
        return e;
    }
};

// own + partner over the distances 32 .. 1: every lane ends with the same bits
__device__ __forceinline__ double butterfly(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, LANES);
    return v;
}

struct DeviceSys {
    DeviceLoad load;
    Cam cam;
    int n, lane;
    Flags f;
    uint64_t* out;
    orbo_step* tr;
    __device__ void full(const Pose& P, double (&acc)[NACC]) {
        lane_full(load, cam, P, n, lane, f, acc);
#pragma unroll
        for (int a = 0; a < NACC; a++) acc[a] = butterfly(acc[a]);
    }
    __device__ double chi(const Pose& P) { return butterfly(lane_chi(load, cam, P, n, lane, f)); }
    __device__ void classify(const Pose& est, const Pose& last, double th, int& nbad, int& nout) {
        nbad = 0;
        nout = 0;
        for (int base = 0, k = 0; base < n; base += LANES, k++) {
            const int i = base + lane;
            bool outlier = false, bad = false;
            if (i < n) {
                outlier = f.get(k);
                classify_edge(load, cam, est, last, th, i, outlier, bad);
                f.set(k, outlier);
            }
            const unsigned long long mo = __ballot(outlier), mb = __ballot(bad);        // bit l = lane l = edge base + l
            if (lane == 0) out[k] = mo;
            nbad += __popcll(mb);
            nout += __popcll(mo);
        }
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

__global__ __launch_bounds__(POSE_TPB, 2) void k_pose_optimize(Problems PR, const float* edges, int ncap, const float* Tcw, orbo_result* result,
                                                            uint64_t* outlier, orbo_step* trace) {
    const int p = blockIdx.x;
    const orbo_problem& q = PR.p[p];
    DeviceSys sys;
    sys.load = {edges + (size_t)p * ORBO_EDGE_ROWS * ncap, ncap};
    sys.cam = {(double)q.fx, (double)q.fy, (double)q.cx, (double)q.cy};
    sys.n = q.n;
    sys.lane = threadIdx.x;
    sys.out = outlier + (size_t)p * ORBO_WORDS(ncap);
    sys.tr = trace ? trace + (size_t)p * ORBO_MAX_ITERS : nullptr;
    orbo_result res;
    pose_optimization(sys, q.n, Tcw + (size_t)p * 12, res);
    if (sys.lane == 0) result[p] = res;
}

}  // namespace orbo

extern "C" {

int orbo_pose_batch_device(const orbo_problem* problems, int nproblems, const float* d_edges, int ncap, const float* d_Tcw, orbo_result* d_result,
                           uint64_t* d_outlier, orbo_step* d_trace, void* stream) {
    orbo::Problems PR;
    TRY(orbo::check_batch(problems, nproblems, ncap, PR));
    if (!orbo::all_set({d_edges, d_Tcw, d_result, d_outlier})) return ORBX_ERR_ARG;
    hipLaunchKernelGGL(orbo::k_pose_optimize, dim3(nproblems), dim3(orbo::POSE_TPB), 0, (hipStream_t)stream, PR, d_edges, ncap, d_Tcw, d_result, d_outlier,
                       d_trace);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbo_pose_batch(const orbo_problem* problems, int nproblems, const float* const* xyz, const float* const* uv, const float* const* inv_sigma2,
                    const float* Tcw, orbo_result* results, uint64_t* const* outlier, orbo_step* const* trace, int device) {
    if (!problems || nproblems < 1 || nproblems > ORBO_MAX_PROBLEMS || !orbo::all_set({xyz, uv, inv_sigma2, Tcw, results, outlier})) return ORBX_ERR_ARG;
    size_t N = 1;
    for (int p = 0; p < nproblems; p++) {
        if (orbo::check_frame(problems[p], xyz[p], uv[p], inv_sigma2[p], outlier[p]) != ORBX_OK) return ORBX_ERR_ARG;
        N = std::max(N, (size_t)problems[p].n);
    }
    // the frames' arrays packed to the shared cap N
    const size_t P = nproblems, W = ORBO_WORDS(N);
    std::vector<float> he(P * ORBO_EDGE_ROWS * N);
    for (size_t p = 0; p < P; p++) orbo::pack_edges(problems[p].n, (int)N, xyz[p], uv[p], inv_sigma2[p], &he[p * ORBO_EDGE_ROWS * N]);
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto ie = s.in(he.data(), he.size());
    const auto it = s.in(Tcw, P * 12);
    const auto orr = s.out<orbo_result>(P);
    const auto of = s.out<uint64_t>(P * W);
    const auto ot = s.out<orbo_step>(trace ? P * ORBO_MAX_ITERS : 0);
    HIPTRY(s.alloc());
    TRY(orbo_pose_batch_device(problems, nproblems, s[ie], (int)N, s[it], s[orr], s[of], trace ? s[ot] : nullptr, nullptr));
    std::vector<uint64_t> hf(P * W);
    std::vector<orbo_step> ht;
    HIPTRY(s.get(results, orr, P));
    HIPTRY(s.get(hf.data(), of, hf.size()));
    if (trace) {
        ht.resize(P * ORBO_MAX_ITERS);
        HIPTRY(s.get(ht.data(), ot, ht.size()));
    }
    for (size_t p = 0; p < P; p++) {
        if (problems[p].n > 0) std::memcpy(outlier[p], &hf[p * W], ORBO_WORDS(problems[p].n) * sizeof(uint64_t));
        if (trace && trace[p]) std::memcpy(trace[p], &ht[p * ORBO_MAX_ITERS], ORBO_MAX_ITERS * sizeof(orbo_step));
    }
    return ORBX_OK;
}

int orbo_pose(const orbo_problem* problem, const float* xyz, const float* uv, const float* inv_sigma2, const float* Tcw, orbo_result* result,
              uint64_t* outlier, orbo_step* trace, int device) {
    if (!problem || !result) return ORBX_ERR_ARG;
    return orbo_pose_batch(problem, 1, &xyz, &uv, &inv_sigma2, Tcw, result, &outlier, trace ? &trace : nullptr, device);
}

}  // extern "C"
