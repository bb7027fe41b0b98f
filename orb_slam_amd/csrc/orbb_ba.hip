// The bundle adjustment of the mapping thread on gfx950: g2o's optimize(iters) with Levenberg over the Schur complement, as
// Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:287-536) and Optimizer::BundleAdjustment (:46-151) run it.  include/orbb.h is the
// boundary and states the arithmetic and the orders of the sums; orbb_math.h holds them, shared with the host route.
//
// What was built, and why:
//   k_ba_point_setup, k_ba_pose_count, k_ba_pose_fill   once per call: every edge's point, and the by-pose list (one wave per free pose scans the
//       edge_pose array twice, counting and then placing its edges by ballot and prefix popcount: stable, ascending, no sort and no atomic).
//   k_ba_linearize<FULL>  one THREAD per point walks the point's edges in order: error, chi2, Huber weight; FULL also both Jacobians, Hll, bl and
//       the 3 x 6 Hpl block of every edge into the work buffer.  Without FULL it is the trial pass.  A point has 2 to 10 edges and the sums are
//       serial in edge order, so a sub-wave per point would idle; points are what there are thousands of.
//   k_ba_pose_sums  one wave per free pose over its edge list, orbo's lane-strided sums (orbo::add_edge itself) and its xor butterfly: 27 sums in
//       registers.  The pose block is RECOMPUTED from the edge here instead of being read back from the linearize pass (21 doubles per edge).
//   k_ba_dinv       one thread per point: (Hll + lambda*I)^-1.
//   k_ba_schur      one workgroup per block row of S with the row (6 x 6*nfree doubles, 36 KiB at the cap) in LDS.  It walks the pose's edges in
//       order; per edge 18 threads form B*Dinv, then the threads take the (edge of the same point, a, b) entries: a point has at most one edge to a
//       pose, so no two threads meet in an entry and an entry's subtractions come in point order.  Only the blocks p2 <= p1 are formed.
//   k_ba_solve      ONE workgroup of 1024 threads: the right-looking LDL' in place in global memory (the matrix is 4.5 MiB at the cap), the column of
//       L and the right-hand side in LDS, the three substitutions column by column, and the pose part of computeScale.  No kernel may wait on
//       another workgroup, so a multi-workgroup factorisation would be one launch per column; tools/bench_localba.py prices this kernel.
//   k_ba_back       one thread per point (xl, the trial point, the point's share of computeScale) and per pose (exp(x)*estimate).
//   k_ba_reduce     one workgroup of ORBB_REDUCE_LANES threads: the total chi, the point part of computeScale, the largest diagonal and the number
//       of active edges, lane-strided and then a tree over LDS, in the order orbb.h fixes.
//   k_ba_flags      one thread per edge, one ballot per word.
// The Levenberg loop is driven from the HOST (orbb::optimize in orbb_math.h): one control block of ORBB_CTL doubles comes down per outer iteration
// and per trial.  No atomics, no inline assembly, no waiting between workgroups; every loop is bounded by an array length.
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>
#include <vector>

#include "orbb.h"
#include "orbb_host.h"
#include "orbb_math.h"
#include "orbx_host.h"

namespace orbb {

constexpr int PT_TPB = 128, SCHUR_TPB = 256, SOLVE_TPB = 1024, FLAG_TPB = 256;

__global__ __launch_bounds__(PT_TPB) void k_ba_point_setup(Ctx c) {
    const int j = blockIdx.x * PT_TPB + threadIdx.x;
    if (j < c.npoints) point_setup(c, j);
}

// the edges of free pose p = blockIdx.x, counted (pose_count) ...
__global__ __launch_bounds__(LANES) void k_ba_pose_count(Ctx c) {
    const int p = blockIdx.x, lane = threadIdx.x;
    int cnt = 0;
    for (int base = 0; base < c.nedges; base += LANES) {
        const int e = base + lane;
        cnt += __popcll(__ballot(e < c.nedges && c.edge_pose[e] == p));
    }
    if (lane == 0) c.pose_count[p] = cnt;
}
// ... and placed behind those of the poses before it, in ascending edge index
__global__ __launch_bounds__(LANES) void k_ba_pose_fill(Ctx c) {
    const int p = blockIdx.x, lane = threadIdx.x;
    int pos = 0;
    for (int q = 0; q < p; q++) pos += c.pose_count[q];
    if (lane == 0) c.pose_first[p] = pos;
    for (int base = 0; base < c.nedges; base += LANES) {
        const int e = base + lane;
        const bool m = e < c.nedges && c.edge_pose[e] == p;
        const unsigned long long mask = __ballot(m);
        if (m) c.pose_edges[pos + __popcll(mask & (((unsigned long long)1 << lane) - 1))] = e;
        pos += __popcll(mask);
    }
    if (lane == 0 && p == c.nfree - 1) c.pose_first[c.nfree] = pos;
}

template <bool FULL>
__global__ __launch_bounds__(PT_TPB) void k_ba_linearize(Ctx c, const double* poses, const double* points) {
    const int j = blockIdx.x * PT_TPB + threadIdx.x;
    if (j < c.npoints) point_linearize<FULL>(c, poses, points, j);
}

__global__ __launch_bounds__(LANES) void k_ba_pose_sums(Ctx c, const double* poses, const double* points) {
    const int p = blockIdx.x, lane = threadIdx.x;
    double acc[NACC];
    int nact;
    pose_lane_sums(c, poses, points, p, lane, acc, nact);
#pragma unroll
    for (int a = 0; a < NACC; a++) {
        double v = acc[a];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, LANES);
        acc[a] = v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nact += __shfl_xor(nact, d, LANES);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < NACC; a++) c.Hpp[(size_t)p * NACC + a] = acc[a];
        c.pose_nact[p] = nact;
    }
}

__global__ __launch_bounds__(PT_TPB) void k_ba_dinv(Ctx c, double lambda) {
    const int j = blockIdx.x * PT_TPB + threadIdx.x;
    if (j < c.npoints) point_dinv(c, lambda, j);
}

__global__ __launch_bounds__(SCHUR_TPB) void k_ba_schur(Ctx c, double lambda) {
    extern __shared__ double row[];                             // 6 x n
    __shared__ double bsr[6], BD[18];
    const int p1 = blockIdx.x, t = threadIdx.x, n = c.n;
    for (int i = t; i < 6 * n; i += SCHUR_TPB) row[i] = schur_row_init(c, lambda, p1, i / n, i % n);
    if (t < 6) bsr[t] = schur_rhs_init(c, p1, t);
    __syncthreads();
    const int klo = c.pose_first[p1], khi = c.pose_first[p1 + 1];
    for (int k = klo; k < khi; k++) {
        const int e1 = c.pose_edges[k], j = c.edge_point[e1];
        if (!edge_active(c, e1) || j < 0) continue;             // the same for every thread
        if (t < 18) BD[t] = schur_bd(c, e1, j, t / 3, t % 3);
        __syncthreads();
        if (t < 6) bsr[t] = bsr[t] - schur_rhs_term(c, BD, j, t);
        int lo, hi;
        point_range(c, j, lo, hi);
        for (int task = t; task < (hi - lo) * 36; task += SCHUR_TPB) {
            const int e2 = lo + task / 36, a = (task % 36) / 6, b = task % 6;
            if (!schur_pairs(c, e2, p1)) continue;
            const int i = a * n + c.edge_pose[e2] * 6 + b;
            row[i] = row[i] - schur_term(c, BD, e2, a, b);
        }
        __syncthreads();
    }
    const int w = (p1 + 1) * 6;
    for (int i = t; i < 6 * w; i += SCHUR_TPB) c.S[(size_t)(p1 * 6 + i / w) * n + i % w] = row[(i / w) * n + i % w];
    if (t < 6) c.bs[p1 * 6 + t] = bsr[t];
}

__global__ __launch_bounds__(SOLVE_TPB) void k_ba_solve(Ctx c, double lambda) {
    __shared__ double col[6 * ORBB_MAX_FREE], y[6 * ORBB_MAX_FREE];
    __shared__ int failed;
    const int t = threadIdx.x, n = c.n;
    double* S = c.S;
    if (t == 0) failed = 0;
    for (int i = t; i < n; i += SOLVE_TPB) y[i] = c.bs[i];
    __syncthreads();
    for (int k = 0; k < n; k++) {
        const double dk = S[(size_t)k * n + k];
        if (t == 0 && !ldl_pivot_ok(dk)) failed = 1;
        for (int i = k + 1 + t; i < n; i += SOLVE_TPB) {
            const double l = S[(size_t)i * n + k] / dk;
            S[(size_t)i * n + k] = l;
            col[i] = l;
        }
        __syncthreads();
        for (int i = k + 1 + t / LANES; i < n; i += SOLVE_TPB / LANES)
            for (int j = k + 1 + t % LANES; j <= i; j += LANES) S[(size_t)i * n + j] = ldl_update(S[(size_t)i * n + j], col[i], col[j], dk);
        __syncthreads();
    }
    for (int k = 0; k < n; k++) {
        const double yk = y[k];
        for (int i = k + 1 + t; i < n; i += SOLVE_TPB) y[i] = sub_update(y[i], S[(size_t)i * n + k], yk);
        __syncthreads();
    }
    for (int i = t; i < n; i += SOLVE_TPB) y[i] = y[i] / S[(size_t)i * n + i];
    __syncthreads();
    for (int k = n - 1; k >= 1; k--) {
        const double xk = y[k];
        for (int i = t; i < k; i += SOLVE_TPB) y[i] = sub_update(y[i], S[(size_t)k * n + i], xk);
        __syncthreads();
    }
    if (!failed)
        for (int i = t; i < n; i += SOLVE_TPB) c.xp[i] = y[i];
    __syncthreads();
    if (t == 0) {
        c.ctl[CTL_SOLVED] = failed ? 0.0 : 1.0;
        c.ctl[CTL_SCALE_POSES] = scale_poses(c, lambda);
    }
}

__global__ __launch_bounds__(PT_TPB) void k_ba_back(Ctx c, double lambda, const double* est_pose, double* trial_pose, const double* est_point,
                                                    double* trial_point) {
    const int i = blockIdx.x * PT_TPB + threadIdx.x;
    if (i < c.npoints) point_back(c, lambda, c.ctl[CTL_SOLVED] != 0.0, est_point, trial_point, i);
    else if (i < c.npoints + c.np) pose_back(c, est_pose, trial_pose, i - c.npoints);
}

__global__ __launch_bounds__(RL) void k_ba_reduce(Ctx c) {
    __shared__ double v[4][RL];
    const int l = threadIdx.x;
    Red r = reduce_lane(c, l);
    v[0][l] = r.chi;
    v[1][l] = r.scale;
    v[2][l] = r.diag;
    v[3][l] = r.nact;
    __syncthreads();
    for (int d = RL / 2; d >= 1; d >>= 1) {
        if (l < d) {
            Red a = {v[0][l], v[1][l], v[2][l], v[3][l]};
            const Red b = {v[0][l + d], v[1][l + d], v[2][l + d], v[3][l + d]};
            reduce_join(a, b);
            v[0][l] = a.chi;
            v[1][l] = a.scale;
            v[2][l] = a.diag;
            v[3][l] = a.nact;
        }
        __syncthreads();
    }
    if (l == 0) reduce_finish(c, Red{v[0][0], v[1][0], v[2][0], v[3][0]});
}

__global__ __launch_bounds__(FLAG_TPB) void k_ba_flags(Ctx c, const double* poses, const double* points, uint64_t* flags) {
    const int e = blockIdx.x * FLAG_TPB + threadIdx.x;
    const bool f = e < c.nedges && edge_flag(c, poses, points, e);
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & (LANES - 1)) == 0 && (e >> 6) < ORBB_WORDS(c.nedges)) flags[e >> 6] = m;
}

inline int blocks(int items, int tpb) { return (items + tpb - 1) / tpb; }

// the passes as launches on one stream; the control block comes down with one copy and one synchronisation
struct DeviceSys {
    Ctx c;
    hipStream_t st;
    int cur = 0;
    double* dump = nullptr;
    int launches = 0, syncs = 0;

#define ORBB_LAUNCH(kernel, grid, tpb, lds, ...)                                               \
    do {                                                                                       \
        if ((grid) > 0) {                                                                      \
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(tpb), lds, st, __VA_ARGS__);           \
            launches++;                                                                        \
        }                                                                                      \
    } while (0)

    int fetch(double* ctl) {
        HIPTRY(hipGetLastError());
        HIPTRY(hipMemcpyAsync(ctl, c.ctl, sizeof(double) * ORBB_CTL, hipMemcpyDeviceToHost, st));
        HIPTRY(hipStreamSynchronize(st));
        syncs++;
        return ORBX_OK;
    }
    void setup() {
        ORBB_LAUNCH(k_ba_point_setup, blocks(c.npoints, PT_TPB), PT_TPB, 0, c);
        ORBB_LAUNCH(k_ba_pose_count, c.nfree, LANES, 0, c);
        ORBB_LAUNCH(k_ba_pose_fill, c.nfree, LANES, 0, c);
    }
    int chi_only(double* ctl) {
        ORBB_LAUNCH(k_ba_linearize<false>, blocks(c.npoints, PT_TPB), PT_TPB, 0, c, c.pose[cur], c.point[cur]);
        ORBB_LAUNCH(k_ba_reduce, 1, RL, 0, c);
        return fetch(ctl);
    }
    int build(double* ctl) {
        ORBB_LAUNCH(k_ba_linearize<true>, blocks(c.npoints, PT_TPB), PT_TPB, 0, c, c.pose[cur], c.point[cur]);
        ORBB_LAUNCH(k_ba_pose_sums, c.nfree, LANES, 0, c, c.pose[cur], c.point[cur]);
        ORBB_LAUNCH(k_ba_reduce, 1, RL, 0, c);
        return fetch(ctl);
    }
    int trial(double lambda, bool first, double* ctl) {
        const auto copy = [this](double* d, const double* s, size_t k) {
            if (k) (void)hipMemcpyAsync(d, s, k * sizeof(double), hipMemcpyDeviceToDevice, st);
        };
        ORBB_LAUNCH(k_ba_dinv, blocks(c.npoints, PT_TPB), PT_TPB, 0, c, lambda);
        ORBB_LAUNCH(k_ba_schur, c.nfree, SCHUR_TPB, (size_t)6 * c.n * sizeof(double), c, lambda);
        if (first && dump) dump_part(c, dump, 0, copy);
        ORBB_LAUNCH(k_ba_solve, 1, SOLVE_TPB, 0, c, lambda);
        ORBB_LAUNCH(k_ba_back, blocks(c.npoints + c.np, PT_TPB), PT_TPB, 0, c, lambda, c.pose[cur], c.pose[cur ^ 1], c.point[cur], c.point[cur ^ 1]);
        if (first && dump) dump_part(c, dump, 1, copy);
        ORBB_LAUNCH(k_ba_linearize<false>, blocks(c.npoints, PT_TPB), PT_TPB, 0, c, c.pose[cur ^ 1], c.point[cur ^ 1]);
        ORBB_LAUNCH(k_ba_reduce, 1, RL, 0, c);
        return fetch(ctl);
    }
    void accept() { cur ^= 1; }
};

}  // namespace orbb

extern "C" {

int orbb_state_from_float(const orbb_problem* problem, const float* Tcw, const float* world, double* pose_qt, double* point_xyz) {
    return orbb::state_from_float(problem, Tcw, world, pose_qt, point_xyz);
}
int orbb_state_to_float(const orbb_problem* problem, const double* pose_qt, const double* point_xyz, float* Tcw, float* world) {
    return orbb::state_to_float(problem, pose_qt, point_xyz, Tcw, world);
}
size_t orbb_work_bytes(const orbb_problem* problem) {
    orbb::Ctx c;
    return orbb::check_problem(problem) == ORBX_OK ? orbb::layout(*problem, nullptr, c) : 0;
}

int orbb_optimize_device(const orbb_problem* problem, const float* d_cam, const int32_t* d_point_first, const int32_t* d_edge_pose,
                         const float* d_edge_uv, const float* d_edge_inv_sigma2, float huber_delta, double* d_pose_qt, double* d_point_xyz,
                         const uint64_t* d_active, double* d_chi2, int iters, void* d_work, size_t work_bytes, orbb_result* result,
                         uint64_t* d_flags, orbo_step* d_trace, double* d_dump, void* stream) {
    using namespace orbb;
    if (check_problem(problem) != ORBX_OK || check_iters(iters) != ORBX_OK) return ORBX_ERR_ARG;
    if (!all_set({d_cam, d_point_first, d_edge_pose, d_edge_uv, d_edge_inv_sigma2, d_pose_qt, d_point_xyz, d_active, d_chi2, d_work, result, d_flags}))
        return ORBX_ERR_ARG;
    const orbb_problem& q = *problem;
    DeviceSys sys;
    const size_t need = layout(q, d_work, sys.c);
    if (work_bytes < need || (uintptr_t)d_work % 256) return ORBX_ERR_ARG;
    Ctx& c = sys.c;
    set_huber(c, huber_delta);
    c.cam = d_cam;
    c.point_first = d_point_first;
    c.edge_pose = d_edge_pose;
    c.edge_uv = d_edge_uv;
    c.edge_w = d_edge_inv_sigma2;
    c.active = d_active;
    c.chi2 = d_chi2;
    sys.st = (hipStream_t)stream;
    sys.dump = d_dump;
    const hipStream_t st = sys.st;
    const size_t pose_bytes = (size_t)c.np * 7 * sizeof(double), point_bytes = (size_t)q.npoints * 3 * sizeof(double);
    HIPTRY(hipMemsetAsync(d_work, 0, need, st));
    HIPTRY(hipMemsetAsync(c.edge_point, 0xff, (size_t)(q.nedges ? q.nedges : 1) * sizeof(int32_t), st));
    if (d_dump) HIPTRY(hipMemsetAsync(d_dump, 0, ORBB_DUMP_DOUBLES(q.nfree, q.npoints) * sizeof(double), st));
    HIPTRY(hipMemcpyAsync(c.pose[0], d_pose_qt, pose_bytes, hipMemcpyDeviceToDevice, st));
    if (point_bytes) HIPTRY(hipMemcpyAsync(c.point[0], d_point_xyz, point_bytes, hipMemcpyDeviceToDevice, st));
    sys.setup();
    std::memset(result, 0, sizeof(*result));
    std::vector<orbo_step> trace(d_trace ? ORBB_MAX_ITERS : 0);
    TRY(optimize(sys, iters, *result, d_trace ? trace.data() : nullptr));
    HIPTRY(hipMemcpyAsync(d_pose_qt, c.pose[sys.cur], pose_bytes, hipMemcpyDeviceToDevice, st));
    if (point_bytes) HIPTRY(hipMemcpyAsync(d_point_xyz, c.point[sys.cur], point_bytes, hipMemcpyDeviceToDevice, st));
    if (q.nedges) {
        hipLaunchKernelGGL(k_ba_flags, dim3(blocks(q.nedges, FLAG_TPB)), dim3(FLAG_TPB), 0, st, c, (const double*)c.pose[sys.cur],
                           (const double*)c.point[sys.cur], d_flags);
        sys.launches++;
    }
    if (d_trace) HIPTRY(hipMemcpyAsync(d_trace, trace.data(), trace.size() * sizeof(orbo_step), hipMemcpyHostToDevice, st));
    HIPTRY(hipGetLastError());
    HIPTRY(hipStreamSynchronize(st));
    sys.syncs++;
    result->launches = sys.launches;
    result->syncs = sys.syncs;
    return ORBX_OK;
}

int orbb_optimize(const orbb_problem* problem, const float* cam, const int32_t* point_first, const int32_t* edge_pose, const float* edge_uv,
                  const float* edge_inv_sigma2, float huber_delta, double* pose_qt, double* point_xyz, const uint64_t* active, double* chi2,
                  int iters, orbb_result* result, uint64_t* flags, orbo_step* trace, double* dump, int device) {
    using namespace orbb;
    if (check_problem(problem) != ORBX_OK || check_iters(iters) != ORBX_OK || !all_set({cam, point_first, pose_qt, result})) return ORBX_ERR_ARG;
    const orbb_problem& q = *problem;
    if (q.npoints > 0 && !point_xyz) return ORBX_ERR_ARG;
    if (q.nedges > 0 && !all_set({edge_pose, edge_uv, edge_inv_sigma2, active, chi2, flags})) return ORBX_ERR_ARG;
    if (check_indices(q, point_first, edge_pose) != ORBX_OK) return ORBX_ERR_ARG;
    const size_t np = (size_t)q.nfree + q.nfixed, P = q.npoints, E = q.nedges, W = ORBB_WORDS(E);
    Ctx c;
    const size_t work_bytes = layout(q, nullptr, c);
    HIPTRY(hipSetDevice(device));
    orbx::Staging s;
    const auto icam = s.in(cam, np * 4);
    const auto ifirst = s.in(point_first, P + 1);
    const auto ipose = s.in(edge_pose, E);
    const auto iuv = s.in(edge_uv, E * 2);
    const auto iw = s.in(edge_inv_sigma2, E);
    const auto iact = s.in(active, W);
    const auto sq = s.in((const double*)pose_qt, np * 7);
    const auto sx = s.in((const double*)point_xyz, P * 3);
    const auto sc = s.in((const double*)chi2, E);
    const auto of = s.out<uint64_t>(W);
    const auto ot = s.out<orbo_step>(trace ? ORBB_MAX_ITERS : 0);
    const auto od = s.out<double>(dump ? ORBB_DUMP_DOUBLES(q.nfree, q.npoints) : 0);
    const auto ow = s.out<uint8_t>(work_bytes);
    HIPTRY(s.alloc());
    TRY(orbb_optimize_device(problem, s[icam], s[ifirst], s[ipose], s[iuv], s[iw], huber_delta, s[sq], s[sx], s[iact], s[sc], iters, s[ow], work_bytes,
                             result, s[of], trace ? s[ot] : nullptr, dump ? s[od] : nullptr, nullptr));
    HIPTRY(s.get(pose_qt, sq, np * 7));
    HIPTRY(s.get(point_xyz, sx, P * 3));
    HIPTRY(s.get(chi2, sc, E));
    HIPTRY(s.get(flags, of, W));
    if (trace) HIPTRY(s.get(trace, ot, (size_t)ORBB_MAX_ITERS));
    if (dump) HIPTRY(s.get(dump, od, ORBB_DUMP_DOUBLES(q.nfree, q.npoints)));
    return ORBX_OK;
}

}  // extern "C"
