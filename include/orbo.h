/* orbo.h — C ABI of tracking's motion-only pose optimisation (part of liborbx.so).
 *
 * What Optimizer::PoseOptimization computes for Tracking between the projection searches: the Levenberg iteration of g2o over one SE3 vertex
 * and n fixed map points, four rounds with the inlier region shrinking, every round of every frame of a call inside one launch.
 *
 * Reference interface replaced (paths relative to the reference ORB_SLAM tree; g2o under Thirdparty/g2o/g2o):
 *   orbo_pose[_batch[_device]]  <- Optimizer::PoseOptimization                                           src/Optimizer.cc:154-285
 *                                  Converter::toSE3Quat, toCvMat(SE3Quat)                                src/Converter.cc:38-54
 *                                  EdgeSE3ProjectXYZ::computeError, linearizeOplus, cam_project          types/types_six_dof_expmap.h:88, .cpp:97-142
 *                                  RobustKernelHuber                                                     core/robust_kernel_impl.cpp:65-91
 *                                  BaseBinaryEdge::constructQuadraticForm                                core/base_binary_edge.hpp:91-113
 *                                  OptimizationAlgorithmLevenberg::solve                                 core/optimization_algorithm_levenberg.cpp:61-189
 *                                  SparseOptimizer::optimize                                             core/sparse_optimizer.cpp:354-419
 *                                  SE3Quat::exp, operator*, normalizeRotation, to_homogeneous_matrix     types/se3quat.h:104-110, :223-285
 *                                  LinearSolverDense::solve                                              solvers/linear_solver_dense.h:104-112
 * What stays with the caller: the walk over mvpMapPoints that makes the edges (Optimizer.cc:191-237) and vnIndexEdge.  Edges are COMPACT:
 * edge i is the i-th non-null map point, flag bit i belongs to edge i.
 *
 * ---- the arithmetic, in double, operation for operation with no contraction (orb_slam_amd/csrc/orbo_math.h) ----
 *   start (Converter.cc:38-48, se3quat.h:62-64, :280-285): the float R | t widened; q = Quaterniond(R) (below); w < 0 negates the four
 *       coefficients; q /= sqrt(((x*x + y*y) + z*z) + w*w).
 *   q*X (the rotation of a point): uv = 2 * (qv x X) (as uv + uv); q*X = (X + w*uv) + (qv x uv); a cross product is
 *       (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
 *   error (types_six_dof_expmap.h:88, .cpp:136-142): (x, y, z) = q*X + t; e = (u - ((x/z)*fx + cx), v - ((y/z)*fy + cy)); fx .. cy, u, v, X
 *       and invSigma2 are floats widened.  chi2 = invSigma2*(e0*e0 + e1*e1).
 *   Huber (robust_kernel_impl.cpp:65-91): delta = (double)(float)sqrt(5.991); dsqr = (double)(float)(delta*delta), the kernel's FLOAT member.
 *       chi2 <= dsqr: rho0 = chi2, rho1 = 1.  Otherwise s = sqrt(chi2): rho0 = (2*s)*delta - dsqr, rho1 = delta/s.  The second-order term
 *       is commented out in the reference (base_edge.h:96-102): the weight is wr = invSigma2*rho1.
 *   Jacobian (.cpp:121-133), z2 = z*z, rotation columns first:
 *       row 0: ((x*y)/z2)*fx   (-(1 + (x*x)/z2))*fx   (y/z)*fx    (-1/z)*fx   0           (x/z2)*fx
 *       row 1: (1 + (y*y)/z2)*fy   (((-x)*y)/z2)*fy   ((-x)/z)*fy   0         (-1/z)*fy   (y/z2)*fy
 *   normal equations (base_binary_edge.hpp:91-113): r = ((-invSigma2)*e)*rho1; H[i][j] += (J0i*wr)*J0j + (J1i*wr)*J1j for i <= j;
 *       b[i] += J0i*r0 + J1i*r1; chi += rho0.
 *   summation order (part of this ABI): lane l of 64 sums the active edges l, l + 64, ... in index order from 0; the 64 partial sums meet in
 *       an xor butterfly over the distances 32, 16, 8, 4, 2, 1 (own + partner, a commutative add, so all lanes end with the same bits).
 *   Levenberg (optimization_algorithm_levenberg.cpp:61-189), per outer iteration: errors, currentChi = iniChi = chi, H and b at the estimate.
 *       At iteration 0 of EACH optimize(): lambda = 1e-5*max_j |H[j][j]|, ni = 2, nBad = 0.  Trial loop: solve (H + lambda*I) x = b;
 *       trial = exp(x)*estimate; tempChi = chi at the trial (DBL_MAX when the solve failed); scale = sum_j x[j]*(lambda*x[j] + b[j]) from 0 in
 *       j order, + 1e-3; rho = (currentChi - tempChi)/scale.  rho > 0 && isfinite(tempChi): alpha = 1 - pow(2*rho - 1, 3) written as
 *       1 - (c*c)*c, lambda *= max(1/3, min(alpha, 2/3)), ni = 2, currentChi = tempChi, the trial becomes the estimate.  Otherwise
 *       lambda *= ni, ni *= 2.  Repeated while (rho < 0 && trials < 10).  Terminate when trials == 10 || rho == 0; then the stop rule of
 *       :154-161: (iniChi - currentChi)*1e3 < iniChi counts up nBad (else resets it), Terminate at 3.  A NaN rho fails every comparison.
 *   exp (se3quat.h:223-257): theta = sqrt((o0*o0 + o1*o1) + o2*o2); Omega = skew(omega); Omega2 = Omega*Omega with every entry
 *       (a0*b0 + a1*b1) + a2*b2; theta < 1e-5: R = V = (I + Omega) + Omega2 (no 1/2, as the source has it); otherwise
 *       R = (I + (sin(theta)/theta)*Omega) + ((1 - cos(theta))/(theta*theta))*Omega2,
 *       V = (I + ((1 - cos(theta))/(theta*theta))*Omega) + ((theta - sin(theta))/pow(theta, 3))*Omega2;
 *       the update is (Quaterniond(R) normalised as at the start, V*upsilon) and the product (:104-110) is
 *       t = t_exp + q_exp*t_est, q = q_exp*q_est (Hamilton product, each coefficient summed left to right as w: aw*bw - ax*bx - ay*by - az*bz,
 *       x: aw*bx + ax*bw + ay*bz - az*by, y: aw*by + ay*bw + az*bx - ax*bz, z: aw*bz + az*bw + ax*by - ay*bx), normalised as at the start.
 *   the four rounds (Optimizer.cc:242-276): 10, 10, 7, 5 outer iterations at most; thresholds the FLOAT constants 9.210f, 7.378f, 5.991f,
 *       5.991f widened.  The chi2 an edge is classified by is the one of the error it LAST computed: for an active edge that of the last
 *       trial of the round, even a rejected one (nothing recomputes after pop()); for an outlier edge it is recomputed at the estimate
 *       (:258-259).  chi2 > th: outlier, counted in nbad; chi2 <= th: inlier; a NaN leaves the flag and is not counted.  After a round the
 *       loop ends when n < 10 (optimizer.edges().size()).  A round without an active edge iterates nothing (sparse_optimizer.cpp:356-359).
 *   output (se3quat.h:270-278): R = toRotationMatrix (tx = 2x, ..., twx = tx*w, txx = tx*x, txy = ty*x, txz = tz*x, tyy = ty*y, tyz = tz*y,
 *       tzz = tz*z; R00 = 1 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy, R10 = txy + twz, R11 = 1 - (txx + tzz), R12 = tyz - twx,
 *       R20 = txz - twy, R21 = tyz + twx, R22 = 1 - (txx + tyy)) and t, narrowed to float, last row 0 0 0 1.
 *
 * NOT PINNED TO EIGEN (Eigen is not part of the reference tree; next to the deviations of orbt.h, orbi.h, orbe.h and orbh.h):
 *   1. Quaterniond(R) is the standard trace / largest-diagonal branch form: tr = (R00 + R11) + R22; tr > 0: s = sqrt(tr + 1), w = 0.5*s,
 *      s = 0.5/s, (x, y, z) = ((R21 - R12)*s, (R02 - R20)*s, (R10 - R01)*s); otherwise i the largest diagonal entry (the first of equal
 *      ones), j, k the next two cyclically: s = sqrt(((Rii - Rjj) - Rkk) + 1), q[i] = 0.5*s, s = 0.5/s, w = (Rkj - Rjk)*s,
 *      q[j] = (Rji + Rij)*s, q[k] = (Rki + Rik)*s.
 *   2. LinearSolverDense's pivoted LDLT is a 6 x 6 LDL^T WITHOUT pivoting in a fixed order: for j = 0 .. 5,
 *      d[j] = A[j][j] - sum_{k<j} (L[j][k]*L[j][k])*d[k], L[i][j] = (A[i][j] - sum_{k<j} (L[i][k]*L[j][k])*d[k])/d[j], sums in k order;
 *      forward, diagonal and backward substitution in index order.  The solve FAILS (ok2 = false, tempChi = DBL_MAX) when a pivot d[j] is
 *      negative or not finite.
 * The device and the host route share this text and agree bit for bit up to sin, cos and pow of exp (the only libm calls; sqrt and the
 * division are IEEE on both), so byte equality of the two is NOT promised: tests/poseopt_checks.py holds the measured tolerances.
 *
 * ---- degenerate input ----
 *   n == 0: the result is the quaternion round trip of the input pose, ninitial = nbad = 0, rounds = 1, no iteration.
 *   n < 10: one round.  Every edge an outlier after a round: the following rounds iterate nothing and classify at the unchanged estimate.
 *   A point behind the camera (z < 0, finite) is an edge like any other: the reference has no depth test here.
 *   z == 0 or non-finite input gives a NaN chi2: such an edge keeps its flag.  While it is active the sums are NaN, the solve fails (x keeps its
 *   last value, zeros at the start), rho is NaN, every trial is rejected after one attempt (`rho < 0` is false) and the estimate stays.
 *
 * The trace (optional): one orbo_step per possible outer iteration, ORBO_MAX_ITERS per problem, round r at offset 0, 10, 20, 27.
 * At convergence currentChi - tempChi is rounding noise, so the accepted / rejected path, lambda and iters[] past that point are not
 * comparable between correct implementations; the pose, the flags and nbad are.
 *
 * ---- measured (tests/golden/poseopt_ref.md has every scene; NOTES.md §35 has the benchmark table) ----
 *   The host route equals the numpy restatement tests/poseopt_ref.py bit for bit on every scene of the suite (they share libm).  The device's
 *   q and t are held to 3.3e-10 absolute, four times the restatement's own spread under a reversed summation order (8.2e-11), and were measured
 *   at most 3.9e-16 from it; Tcw is held to one float ulp per entry (measured 0); flags, ninitial, nbad and rounds are equal.  The scenes keep
 *   every classification chi2 a relative 9.1e-3 or more from its threshold.  Against the host route on one core (this project's text, not g2o)
 *   one frame of 300 edges takes 0.39 against 0.19 ms, eight frames 0.45 against 1.35 ms, thirty-two 0.65 against 5.8 ms.
 *
 * Arguments are checked on the host before anything touches the GPU.  Status codes are orbx.h's; there is no CPU fallback.
 */
#ifndef ORBO_H
#define ORBO_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBO_MAX_PROBLEMS 64        /* frames of one call */
#define ORBO_MAX_EDGES    8192      /* correspondences of one frame */
#define ORBO_EDGE_ROWS    6         /* rows of a problem's edge table on the device */
#define ORBO_ROUNDS       4
#define ORBO_MAX_ITERS    32        /* 10 + 10 + 7 + 5 */
#define ORBO_WORDS(n)     (((n) + 63) / 64)   /* flag words of n edges: bit i % 64 of word i / 64 */

/* One frame's call. */
typedef struct orbo_problem {
    float fx, fy, cx, cy;           /* pFrame->fx .. cy */
    int32_t n;                      /* edges: 0 .. ORBO_MAX_EDGES */
} orbo_problem;

/* What PoseOptimization leaves. */
typedef struct orbo_result {
    float Tcw[16];                  /* what pose.copyTo(pFrame->mTcw) stores (row major) */
    double q[4], t[3];              /* the SE3Quat it was made from (x y z w) */
    int32_t ninitial, nbad;         /* nInitialCorrespondences, nBad: the return value is ninitial - nbad */
    int32_t rounds;                 /* rounds run (the break of :274-275) */
    int32_t iters[ORBO_ROUNDS];     /* outer iterations each optimize() made (cjIterations; 0 for a round without an active edge) */
    int32_t noutlier;               /* flags set in the outlier words: nbad, plus the edges a NaN chi2 left flagged */
} orbo_result;

/* One outer iteration of the trace. */
typedef struct orbo_step {
    double chi_in, chi_out;         /* currentChi when solve() was entered and when it returned */
    double lambda;                  /* _currentLambda when it returned */
    int32_t trials;                 /* qmax */
    int32_t status;                 /* 0 OK, 1 Terminate, 2 not run (everything else 0) */
} orbo_step;

/* The poses of nproblems frames.  `problems` is a HOST array (read during the call); the rest are device buffers with the shared cap
 * ncap >= every n, ncap >= 1.  Problem p's edges are a table of ORBO_EDGE_ROWS rows of ncap floats at d_edges + p*ORBO_EDGE_ROWS*ncap,
 * struct-of-arrays so that the lanes of a wave read consecutive floats:
 *   rows 0-2 X, Y, Z of GetWorldPos(); 3-4 u, v of mvKeysUn; 5 invSigma2 (mvInvLevelSigma2[octave]).
 * d_Tcw + p*12: the rows of [R | t] of mTcw.
 * Outputs: d_result[p]; d_outlier[p*ORBO_WORDS(ncap) + w] for w < ORBO_WORDS(n): mvbOutlier by edge, 64 per word in index order, zero
 * bits past n; d_trace + p*ORBO_MAX_ITERS (may be NULL).  Asynchronous on `stream`; allocates nothing. */
int orbo_pose_batch_device(const orbo_problem* problems, int nproblems, const float* d_edges, int ncap, const float* d_Tcw, orbo_result* d_result,
                           uint64_t* d_outlier, orbo_step* d_trace, void* stream);

/* One frame, synchronous, HOST arrays in and out: xyz[n*3], uv[n*2], inv_sigma2[n] (may be NULL when n == 0), Tcw[12]; result,
 * outlier[ORBO_WORDS(n)] (may be NULL when n == 0), trace[ORBO_MAX_ITERS] (may be NULL). */
int orbo_pose(const orbo_problem* problem, const float* xyz, const float* uv, const float* inv_sigma2, const float* Tcw, orbo_result* result,
              uint64_t* outlier, orbo_step* trace, int device);

/* The same for nproblems frames: ONE launch for all of them and one synchronisation.  Per frame p the arrays xyz[p] ... as in orbo_pose;
 * Tcw is nproblems*12 floats, results an array of nproblems; trace may be NULL, and so may its entries.  Every frame gets, byte for byte,
 * what orbo_pose gives it alone. */
int orbo_pose_batch(const orbo_problem* problems, int nproblems, const float* const* xyz, const float* const* uv, const float* const* inv_sigma2,
                    const float* Tcw, orbo_result* results, uint64_t* const* outlier, orbo_step* const* trace, int device);

#ifdef __cplusplus
}
#endif
#endif
