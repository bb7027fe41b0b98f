/* orbb.h — C ABI of the bundle adjustment of the mapping thread (part of liborbx.so).
 *
 * ONE operation: g2o's SparseOptimizer::optimize(iters) with OptimizationAlgorithmLevenberg over a BlockSolver with the Schur complement, on
 * a graph of SE3 poses (free and fixed), points and reprojection edges with a Huber kernel.  The estimates live in caller buffers as doubles,
 * so a second call continues exactly where the first stopped: Optimizer::LocalBundleAdjustment is optimize(5), a host loop over the flags,
 * optimize(10); Optimizer::BundleAdjustment is one call.
 *
 * Reference interface replaced (paths relative to the reference ORB_SLAM tree; g2o under Thirdparty/g2o/g2o):
 *   orbb_optimize[_device]  <- optimizer.optimize(n) of Optimizer::LocalBundleAdjustment                  src/Optimizer.cc:449-450, :493-494
 *                              and of Optimizer::BundleAdjustment                                         src/Optimizer.cc:128-129
 *                              the test `e->chi2()>5.991 || !e->isDepthPositive()`                        src/Optimizer.cc:461, :509
 *                              EdgeSE3ProjectXYZ::computeError, linearizeOplus, isDepthPositive           types/types_six_dof_expmap.h, .cpp:97-142
 *                              RobustKernelHuber                                                          core/robust_kernel_impl.cpp:65-91
 *                              BaseBinaryEdge::constructQuadraticForm                                     core/base_binary_edge.hpp:91-113
 *                              BlockSolver::setLambda, solve (the Schur complement)                       core/block_solver.hpp:564-589, :367-486
 *                              OptimizationAlgorithmLevenberg::solve, computeLambdaInit, computeScale     core/optimization_algorithm_levenberg.cpp:61-189
 *                              SparseOptimizer::optimize                                                  core/sparse_optimizer.cpp:354-419
 *   orbb_state_from_float   <- Converter::toSE3Quat(GetPose()), Converter::toVector3d(GetWorldPos())      src/Optimizer.cc:361, :403
 *   orbb_state_to_float     <- SetPose(Converter::toCvMat(SE3quat)), SetWorldPos(toCvMat(estimate()))     src/Optimizer.cc:525, :533
 * What stays with the caller: the walk over the key frames and map points that makes the lists and the edges (:289-338, :399-447) and the
 * loops over the flags (:453-470, :497-515).  orb_slam_amd/cpp/BundleAdjuster.h is meant to hold them.
 *
 * ---- the problem ----
 *   Poses: nfree free ones first, then nfixed fixed ones; pose index p < nfree + nfixed.  cam[p*4 ..] = fx fy cx cy of the pose's key frame
 *   (the reference sets them per edge from pKFi, :435-438).  Edges are POINT-MAJOR, as the reference creates them: point j owns the edges
 *   point_first[j] .. point_first[j + 1] - 1, point_first[0] = 0, point_first[npoints] = nedges, non-decreasing.  Per edge: edge_pose (the
 *   pose index), edge_uv (kpUn.pt), edge_inv_sigma2.  A point has AT MOST ONE edge to a pose (GetObservations() is a map keyed by the key frame);
 *   the host form checks it.  huber_delta is the float `thHuber`, (float)sqrt(5.991) for both callers.
 *   The library builds the by-pose list itself: for every free pose its edges in ascending edge index.
 *   State: pose_qt[p*7 ..] = q (x y z w), t; point_xyz[j*3 ..]; active: bit e % 64 of word e / 64 set = edge e is in the optimisation (level 0);
 *   chi2[e]: the chi2 of the error edge e LAST computed, under orbo.h's rule: an active edge keeps the chi2 of the last trial of the call, even
 *   a rejected one (nothing recomputes after pop()).  An inactive edge's chi2 is left alone.  A call that iterates nothing (iters == 0, or no
 *   active edge) computes the chi2 of the active edges at the estimate (g2o leaves _error as it was, there uninitialised).
 *
 * ---- the arithmetic, in double, operation for operation with no contraction (orb_slam_amd/csrc/orbb_math.h over orbo_math.h) ----
 *   Error, chi2, Huber (with delta = (double)huber_delta, dsqr = (double)(float)(delta*delta)), the pose Jacobian Jp (2 x 6), r and wr, exp and
 *   the SE3 product, the start and the float output of a pose: the text of orbo.h, shared.
 *   Point Jacobian (types_six_dof_expmap.cpp:110-119): s = -1.0/z; T = [[s*fx, s*0, s*(((-x)/z)*fx)], [s*0, s*fy, s*(((-y)/z)*fy)]];
 *       Jl[r][c] = (T[r][0]*R[0][c] + T[r][1]*R[1][c]) + T[r][2]*R[2][c] with R = toRotationMatrix of the pose (orbo.h's text).
 *   Normal equations (base_binary_edge.hpp:91-113), per active edge e of point j and pose p:
 *       Hll_j[c][d] += (Jl0c*wr)*Jl0d + (Jl1c*wr)*Jl1d (c <= d), bl_j[c] += Jl0c*r0 + Jl1c*r1; when p is free also
 *       Hpl_e[c][a] = (Jl0c*wr)*Jp0a + (Jl1c*wr)*Jp1a (3 x 6) and Hpp_p, bp_p as orbo.h.  chi += rho0.
 *   SUMMATION ORDERS (part of this ABI; none depends on a grid size or on timing, there is no floating-point atomic):
 *       point sums (Hll, bl, the point's rho0 sum): the point's active edges in edge order, from 0.
 *       pose sums (Hpp, bp): orbo.h's: lane l of 64 sums the active edges at the positions l, l + 64, ... of the pose's list, from 0, and the
 *           64 partial sums meet in the xor butterfly over 32, 16, 8, 4, 2, 1.
 *       sums over points (the total chi, the point part of computeScale, the largest diagonal): lane l of ORBB_REDUCE_LANES = 1024 takes the
 *           points l, l + 1024, ... in order from 0 (resp. from the first for the maximum); for d = 512, 256, .. 1: v[l] = v[l] + v[l + d]
 *           for l < d; the result is v[0].  The maximum uses std::max's form m = (h < m) ? m : h in the same shape, poses first
 *           (serially over the 6 diagonals of each free pose), then joined with the points' as (pts < poses) ? poses : pts.
 *   Damping (block_solver.hpp:564-589): lambda is added to EVERY diagonal entry of Hpp and Hll.
 *   Schur complement (block_solver.hpp:367-486), per point j with Di = inverse(Hll_j + lambda*I) (below), B_e[a][c] = Hpl_e[c][a]:
 *       BD_e[a][c] = (B[a][0]*Di[0][c] + B[a][1]*Di[1][c]) + B[a][2]*Di[2][c];
 *       S[p1][p2][a][b] = (Hpp + lambda*I)[p1][p2][a][b] - sum_j (BD_e1[a][0]*B_e2[b][0] + BD_e1[a][1]*B_e2[b][1]) + BD_e1[a][2]*B_e2[b][2]
 *       bs[p1][a] = bp[p1][a] - sum_j (BD_e1[a][0]*bl_j[0] + BD_e1[a][1]*bl_j[1]) + BD_e1[a][2]*bl_j[2]
 *       over the points j with active edges e1 to p1 and e2 to p2, in ascending j, one subtraction per point.  Only the blocks p2 <= p1 are
 *       formed and only the lower triangle of S is read.
 *   Reduced solve: below.  Back-substitution: cl = bl_j, then for the point's active edges e to free poses in edge order
 *       cl[c] = cl[c] - (((((H[c][0]*x0 + H[c][1]*x1) + H[c][2]*x2) + H[c][3]*x3) + H[c][4]*x4) + H[c][5]*x5), H = Hpl_e, x = xp[pose];
 *       xl[r] = (Di[r][0]*cl[0] + Di[r][1]*cl[1]) + Di[r][2]*cl[2].
 *   Update: exp(x)*estimate for a pose (orbo.h), estimate + xl for a point.
 *   computeLambdaInit (:166-180): 1e-5 x the largest |diagonal| of Hpp and Hll over all free poses and all points.
 *   computeScale (:182-189): sum_j x[j]*(lambda*x[j] + b[j]) over the whole x, poses first: the pose part serially from 0 in j order; per point
 *       (x0*(lambda*x0 + b0) + x1*(lambda*x1 + b1)) + x2*(lambda*x2 + b2), summed over the points as above; scale = (poses + points) + 1e-3.
 *   The trial, accept, reject and stop rules are exactly the ones orbo.h states at its lines 36-42.  A failed solve leaves x as it was (zeros
 *   at the start of a call) and the trial is still made with it.
 *   Vertices without an active edge: a free pose or a point with no active edge gets x = 0 and keeps its estimate bit for bit (g2o drops it
 *   from the index mapping; its block of S is the identity).  A point with ONE edge has a rank-2 Hll; only lambda makes it invertible.
 *
 * NOT PINNED TO EIGEN:
 *   1. The 3 x 3 D->inverse() is the adjugate over the determinant.  With a b c / b d e / c e f = Hll + lambda*I:
 *      c00 = d*f - e*e, c01 = c*e - b*f, c02 = b*e - c*d, c11 = a*f - c*c, c12 = b*c - a*e, c22 = a*d - b*b,
 *      det = (a*c00 + b*c01) + c*c02, Di = c../det (symmetric).
 *   2. g2o's LinearSolverEigen (a sparse LLT behind an ordering) is a dense LDL' WITHOUT pivoting of the n = 6*nfree system, in this order:
 *      for k = 0 .. n-1: d[k] = A[k][k]; L[i][k] = A[i][k]/d[k] for i > k; A[i][j] = A[i][j] - (L[i][k]*L[j][k])*d[k] for k < j <= i.
 *      Forward: for k ascending y[i] = y[i] - L[i][k]*y[k] (i > k); y[i] = y[i]/d[i]; backward: for k DESCENDING x[i] = x[i] - L[k][i]*x[k]
 *      (i < k).  The solve FAILS when a pivot d[k] is negative or not finite: tempChi = DBL_MAX, as orbo.h point 2.
 *   The device and the host route (tools/liblocalba_host.so) share this text and these orders.  Nothing before the first exp calls libm, so the
 *   two agree BYTE FOR BYTE on the first-build dump; after that they differ only through sin, cos and pow.
 *
 * ---- flags ----
 *   Bit e (words as `active`) = edge e was active on entry && (chi2[e] > 5.991 || !((q*X + t).z > 0)), with the DOUBLE literal 5.991 of
 *   Optimizer.cc:461 (not orbo.h's float) and the depth at the final ESTIMATE, not at the last trial (isDepthPositive).  A NaN chi2 with a
 *   positive depth sets no flag.
 *
 * ---- the host-driven loop ----
 *   The Levenberg bookkeeping (rho, lambda, accept or reject, the stop rule) runs on the host from a block of ORBB_CTL doubles downloaded once
 *   per outer iteration and once per trial: orbb_optimize_device synchronises `stream` a bounded number of times (at most iters*11 + 3) and
 *   returns when done.  It allocates nothing.  The stop-flag of the reference cannot interrupt a call.
 *
 * ---- measured (tests/golden/localba_ref.md has every scene; NOTES.md §36 has the benchmark tables) ----
 *   The host route equals the numpy restatement tests/localba_ref.py bit for bit on every scene of the suite and both phases (they share libm), the
 *   first-build dump included.  The device's poses and points are held to 3.5e-12 absolute, four times the restatement's own spread under reversed
 *   summation orders (8.75e-13), and were measured at 0 from it on an MI355X; the floats of orbb_state_to_float are held to one float ulp
 *   (measured 0); flags, iterations and status are equal; the first-build dump equals the host route's bytes.  The scenes keep every classifying
 *   chi2 and depth a relative 7.6e-3 or more from its threshold.  optimize(5) with one trial per iteration is 49 launches and 11 synchronisations.
 *   Against the host route on one core (this project's text, not g2o) the two-phase local BA over device-resident arrays takes 8.9 against 11.3 ms at
 *   10 free poses and 4000 edges, 15.4 against 42.8 ms at 30 and 15000, 82 against 222 ms at 80 and 48000, where the one-workgroup solve is 73 of
 *   the 82 ms; through the host-array form the smallest problem loses (13.9 ms).
 *
 * Arguments are checked on the host before anything touches the GPU.  Status codes are orbx.h's; there is no CPU fallback.
 */
#ifndef ORBB_H
#define ORBB_H

#include <stddef.h>
#include <stdint.h>

#include "orbo.h"
#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ORBB_MAX_FREE: the reduced system is dense, 6*128 = 768 rows, 4.5 MiB of doubles: it stays in the L2 / MALL, one workgroup factors it
 * (768^3/6 = 75 M multiply-subtracts a solve), and the Schur row of one pose (6 x 768 doubles = 36 KiB) fits the LDS of a workgroup.  The
 * local window of the reference is the covisible key frames of one key frame, some tens.  The other caps only bound the index arithmetic. */
#define ORBB_MAX_FREE    128
#define ORBB_MAX_POSES   4096        /* free + fixed */
#define ORBB_MAX_POINTS  (1 << 20)
#define ORBB_MAX_EDGES   (1 << 22)
#define ORBB_MAX_ITERS   64          /* iters of one call; the trace has this many records */
#define ORBB_REDUCE_LANES 1024
#define ORBB_CTL         8           /* doubles of the control block */
#define ORBB_WORDS(n)    (((n) + 63) / 64)

typedef struct orbb_problem {
    int32_t nfree, nfixed, npoints, nedges;
} orbb_problem;

#define ORBB_RUN_OK        0   /* every iteration ran */
#define ORBB_RUN_TERMINATE 1   /* the stop rule ended the call early */
#define ORBB_RUN_NOTHING   2   /* iters == 0 or no active edge */

typedef struct orbb_result {
    double chi_first, chi_last;     /* the robust chi of the active edges at the entry estimate and at the final one */
    double lambda;                  /* _currentLambda at the end */
    int32_t iters;                  /* outer iterations run */
    int32_t status;                 /* ORBB_RUN_* */
    int32_t launches, syncs;        /* kernel launches and stream synchronisations of this call */
} orbb_result;

/* the doubles of the first-build dump: Hpp|bp|chi (28 per free pose, orbo.h's packing), Hll (6 per point: 00 01 02 11 12 22), bl (3 per point),
 * S (n x n row major, lower blocks; the rest zero), bs (n), x poses (n), x points (3 per point); n = 6*nfree.  All at iteration 0, trial 0. */
#define ORBB_DUMP_DOUBLES(nfree, npoints) ((size_t)(nfree) * 28 + (size_t)(npoints) * 12 + (size_t)36 * (nfree) * (nfree) + (size_t)12 * (nfree))

/* Tcw[np*12] (rows of [R | t]) and world[npoints*3] floats -> the state.  Plain host arithmetic. */
int orbb_state_from_float(const orbb_problem* problem, const float* Tcw, const float* world, double* pose_qt, double* point_xyz);
/* the state -> Tcw[np*16] and world[npoints*3] floats as SetPose and SetWorldPos store them */
int orbb_state_to_float(const orbb_problem* problem, const double* pose_qt, const double* point_xyz, float* Tcw, float* world);

size_t orbb_work_bytes(const orbb_problem* problem);

/* Every d_ pointer is device memory: d_cam[np*4], d_point_first[npoints + 1], d_edge_pose[nedges], d_edge_uv[nedges*2], d_edge_inv_sigma2[nedges],
 * d_pose_qt, d_point_xyz, d_active[ORBB_WORDS(nedges)] (read only), d_chi2[nedges], d_work of work_bytes >= orbb_work_bytes(), 256-aligned;
 * d_flags[ORBB_WORDS(nedges)]; d_trace[ORBB_MAX_ITERS] orbo_step (may be NULL; records past `iters` get status 2); d_dump
 * (ORBB_DUMP_DOUBLES, may be NULL).  `result` is HOST memory.  Index arrays are not checked here: a pose index outside the problem makes the edge
 * inactive, a point range is clamped to the edges.  Synchronises `stream`; returns when the state, chi2, flags and trace are written. */
int orbb_optimize_device(const orbb_problem* problem, const float* d_cam, const int32_t* d_point_first, const int32_t* d_edge_pose,
                         const float* d_edge_uv, const float* d_edge_inv_sigma2, float huber_delta, double* d_pose_qt, double* d_point_xyz,
                         const uint64_t* d_active, double* d_chi2, int iters, void* d_work, size_t work_bytes, orbb_result* result,
                         uint64_t* d_flags, orbo_step* d_trace, double* d_dump, void* stream);

/* The same over HOST arrays (state, chi2 in and out; flags, trace, dump out; trace and dump may be NULL).  Checks the index arrays. */
int orbb_optimize(const orbb_problem* problem, const float* cam, const int32_t* point_first, const int32_t* edge_pose, const float* edge_uv,
                  const float* edge_inv_sigma2, float huber_delta, double* pose_qt, double* point_xyz, const uint64_t* active, double* chi2,
                  int iters, orbb_result* result, uint64_t* flags, orbo_step* trace, double* dump, int device);

#ifdef __cplusplus
}
#endif
#endif
