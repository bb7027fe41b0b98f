/* orbg.h — C ABI of loop closing's Sim3 refinement (part of liborbx.so).
 *
 * What Optimizer::OptimizeSim3 computes for LoopClosing::ComputeSim3 after the Sim3 RANSAC and SearchBySim3: the Levenberg iteration of g2o over
 * one free 7-dof similarity vertex and n pairs of fixed points, every pair seen from both sides, in two phases with an inlier check after each;
 * both phases and both checks of every loop candidate of a call inside one launch.
 *
 * Reference interface replaced (paths relative to the reference ORB_SLAM tree; g2o under Thirdparty/g2o/g2o):
 *   orbg_sim3[_batch[_device]]  <- Optimizer::OptimizeSim3                                               src/Optimizer.cc:789-987
 *                                  Converter::toCvMat(g2o::Sim3)                                         src/Converter.cc:56-62
 *                                  EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError          types/types_seven_dof_expmap.h:138-145, :160-167
 *                                  VertexSim3Expmap::oplusImpl, cam_map1, cam_map2                       types/types_seven_dof_expmap.h:60-88
 *                                  Sim3(R, t, s), Sim3(update), map, inverse, operator*                  types/sim3.h:64-67, :70-146, :233-236, :266-272
 *                                  BaseBinaryEdge::linearizeOplus (numeric), constructQuadraticForm      core/base_binary_edge.hpp:130-205, :91-113
 *                                  RobustKernelHuber                                                     core/robust_kernel_impl.cpp:65-91
 *                                  OptimizationAlgorithmLevenberg::solve                                 core/optimization_algorithm_levenberg.cpp:61-189
 *                                  SparseOptimizer::optimize                                             core/sparse_optimizer.cpp:354-419
 *                                  LinearSolverDense::solve                                              solvers/linear_solver_dense.h:104-112
 * What stays with the caller: the walk over vpMatches1 that makes the pairs (Optimizer.cc:844-923) and vnIndexEdge.  A PAIR is one iteration of
 * that loop that reached nCorrespondences++.  Pairs are COMPACT: pair i is the i-th such iteration, flag bit i belongs to pair i.
 *
 * ---- the arithmetic, in double, operation for operation with no contraction (orb_slam_amd/csrc/orbg_math.h over orbo_math.h) ----
 *   start (sim3.h:64-67, LoopClosing.cc:320): the float R, t, s widened; q = Quaterniond(R) in orbo.h's branch form, NOT normalised.
 *   q*X, the Hamilton product, Huber, toRotationMatrix: orbo.h's text.  conjugate: (-x, -y, -z, w).
 *   map (sim3.h:144-146): (x, y, z) = s*(q*X) + t, each component (s*r_i) + t_i.
 *   inverse (:233-236): q' = conjugate(q); m = -1.0/s; t' = q'*(m*t); s' = 1.0/s.
 *   product (:266-272): q = q_a*q_b (NOT normalised), t = s_a*(q_a*t_b) + t_a, s = s_a*s_b.
 *   edges (types_seven_dof_expmap.h:138-145, :160-167): with S the vertex estimate
 *       e12 = (u1 - ((x/z)*fx1 + cx1), v1 - ((y/z)*fy1 + cy1)) at (x, y, z) = S.map(P2c);
 *       e21 = (u2 - ((x/z)*fx2 + cx2), v2 - ((y/z)*fy2 + cy2)) at (x, y, z) = S.inverse().map(P1c).
 *       chi2 = w*(e0*e0 + e1*e1) with w the edge's information scalar (orbo.h's form of chi2()).
 *   THE INFORMATION IS NOT SYMMETRIC IN THE REFERENCE: edge 12 takes w1 = pKF1->GetInvSigma2(octave1) (Optimizer.cc:894), edge 21 takes
 *       w2 = pKF2->GetSigma2(octave2), the variance and NOT its inverse (:912, the variable is even called invSigmaSquare2).  This ABI reproduces
 *       that: row w2 of a pair holds what the reference passes, sigma2.  At octave 0 both are 1 and the two readings coincide.
 *   Huber (Optimizer.cc:840, robust_kernel_impl.cpp:65-91): delta = (double)(float)sqrt(th2) with the sqrt in double of the float th2 widened;
 *       dsqr = (double)(float)(delta*delta), the kernel's FLOAT member; rho as in orbo.h; no second-order term.
 *   THE JACOBIAN IS NUMERIC: linearizeOplus of both edge types is commented out (types_seven_dof_expmap.h:147, :169; .cpp:196 on), so
 *       BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:130-205) runs.  The fixed point vertex is skipped.  For d = 0 .. 6 the vertex is set to
 *       S(+d) = Sim3(+1e-9*e_d)*S, then to S(-d) = Sim3(-1e-9*e_d)*S (oplusImpl, _fix_scale false); column d of an edge's Jacobian is
 *       (1.0/(2*1e-9))*(e(+d) - e(-d)), e(.) the edge's error at that vertex.  Then _error is restored to the error at S.  The fourteen perturbed
 *       similarities and, for edge 21, their inverses do not depend on the edge and are computed once per linearisation.
 *   Sim3(update) (sim3.h:70-142): omega = x[0..2], upsilon = x[3..5], sigma = x[6]; theta = sqrt((o0*o0 + o1*o1) + o2*o2); Omega = skew(omega),
 *       Omega2 = Omega*Omega with every entry (a0*b0 + a1*b1) + a2*b2; s = exp(sigma) (also at +-1e-9); eps = 0.00001.  Four branches:
 *         |sigma| < eps, theta < eps:   C = 1, A = 1/2, B = 1/6, R = (I + Omega) + Omega2
 *         |sigma| < eps, otherwise:     C = 1, theta2 = theta*theta, A = (1 - cos(theta))/theta2, B = (theta - sin(theta))/(theta2*theta), R general
 *         otherwise, theta < eps:       C = (s - 1)/sigma, sigma2 = sigma*sigma, A = ((sigma - 1)*s + 1)/sigma2,
 *                                       B = (((0.5*sigma2 - sigma) + 1)*s)/(sigma2*sigma), R = (I + Omega) + Omega2
 *         otherwise:                    C = (s - 1)/sigma, a = s*sin(theta), b = s*cos(theta), theta2, sigma2, c = theta2 + sigma2,
 *                                       A = (a*sigma + (1 - b)*theta)/(theta*c), B = ((C - ((b - 1)*sigma + a*theta)/c)*1.0)/theta2, R general
 *       R general = (I + (sin(theta)/theta)*Omega) + ((1 - cos(theta))/(theta*theta))*Omega2.  q = Quaterniond(R), NOT normalised;
 *       W = (A*Omega + B*Omega2) + C*I entry by entry; t = W*upsilon, each row (a0*b0 + a1*b1) + a2*b2.
 *       The perturbations take the first branch (a rotation, a translation or a scale of 1e-9); Levenberg steps take whichever they meet.
 *   normal equations, Levenberg, stop rule: orbo.h's text at dimension 7: 28 upper entries of H row by row, 7 of b, chi; a Sim3 edge and an inverse
 *       edge are separate edges in the sums: r = ((-w)*e)*rho1, H[i][j] += (J0i*wr)*J0j + (J1i*wr)*J1j, b[i] += J0i*r0 + J1i*r1, chi += rho0.
 *       The trial is Sim3(x)*estimate.
 *   summation order (part of this ABI): lane l of 64 sums the active pairs l, l + 64, ... in index order from 0, edge 12 before edge 21 within a
 *       pair; the 64 partial sums meet in orbo.h's xor butterfly.
 *   the two phases (Optimizer.cc:927-986): optimize(5); a pair is removed when chi2_12 > th2 || chi2_21 > th2, th2 the float widened, each chi2
 *       that of the LAST error the edge computed: the last trial of the phase, even a rejected one (the numeric linearisation restores _error,
 *       nothing recomputes after pop()).  nMore = nbad > 0 ? 10 : 5.  ncorr - nbad < 10: the `return 0` of :957-958, g2oS12 untouched but the
 *       matches already cleared (ret0).  Otherwise optimize(nMore) over the survivors with lambda initialised afresh; the second check only sets
 *       flags and counts nin.
 *   output (Converter.cc:56-62): R = toRotationMatrix(q) (orbo.h), S12 = [s*R | t; 0 0 0 1] narrowed to float.
 *
 * NOT PINNED TO EIGEN (next to the deviations of orbo.h): Quaterniond(R) is orbo.h's branch form, and LinearSolverDense's pivoted
 *   LDLT is orbo.h's LDL^T WITHOUT pivoting at dimension 7 (for j = 0 .. 6), failing on a negative or non-finite pivot.
 * The device and the host route share this text and agree bit for bit up to exp, sin and cos (the only libm calls), so byte equality of the two is
 * NOT promised.  exp(+-1e-9) enters the scale column of every Jacobian divided by 2e-9: a last-bit difference there is a relative 5.6e-8 of that
 * column.  tests/sim3opt_checks.py holds the measured tolerances.
 *
 * ---- degenerate input ----
 *   n == 0: no vertex is active, optimize() iterates nothing (sparse_optimizer.cpp:356-359); ncorr = nbad = 0, 0 < 10: ret0, iters 0 0.
 *   n < 10: phase 1 runs, then ret0 whatever the check finds.
 *   A NaN chi2: neither `>` is true (Optimizer.cc:939, :973), so the pair STAYS and counts as an inlier in nin.  While it is active the sums are
 *   NaN, the solve fails, rho is NaN, every trial is rejected after one attempt and the estimate stays (as orbo.h).
 *   z == 0 gives such a NaN or an infinity; an infinite chi2 is > th2 and removes the pair.  A point behind a camera (z < 0, finite) is an edge
 *   like any other: the reference has no depth test here.
 *
 * The trace (optional): one orbo_step per possible outer iteration, ORBG_MAX_ITERS per problem, phase 1 at offset 0, phase 2 at offset 5.  As in
 * orbo.h the accepted / rejected path past convergence is not comparable between correct implementations; here the numeric Jacobian's noise
 * (rounding divided by 2e-9) makes that point come early.
 *
 * ---- measured (tests/golden/sim3opt_ref.md has every scene; NOTES.md §37 has the registers and the benchmark table) ----
 *   The host route and the device both equal the numpy restatement tests/sim3opt_ref.py bit for bit on every scene of the suite (measured 0 in q,
 *   t, s and in the float S12).  They are held to 2.52e-7 absolute, four times the restatement's own spread under a reversed summation order
 *   (6.3e-8; the central differences divide rounding noise by 2e-9), and S12 to one float ulp per entry; flags, ncorr, nbad, nin, ret0 are equal.
 *   The scenes keep every classification chi2 a relative 0.66 or more from th2.  Against the host route on one core (this project's text, NOT g2o)
 *   one candidate of 150 pairs takes 0.44 against 0.25 ms, eight candidates 0.53 against 1.83 ms, thirty-two 0.76 against 7.43 ms.
 *
 * Arguments are checked on the host before anything touches the GPU.  Status codes are orbx.h's; there is no CPU fallback.
 */
#ifndef ORBG_H
#define ORBG_H

#include <stddef.h>
#include <stdint.h>

#include "orbo.h"
#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBG_MAX_PROBLEMS 64        /* loop candidates of one call */
#define ORBG_MAX_PAIRS    8192      /* pairs of one candidate */
#define ORBG_PAIR_ROWS    12        /* rows of a problem's pair table on the device */
#define ORBG_MAX_ITERS    15        /* 5 + 10 */

/* One candidate's call. */
typedef struct orbg_problem {
    float fx1, fy1, cx1, cy1;       /* K1 (0,0) (1,1) (0,2) (1,2) */
    float fx2, fy2, cx2, cy2;       /* K2 */
    float th2;                      /* the argument th2 (LoopClosing passes 10) */
    int32_t n;                      /* pairs: 0 .. ORBG_MAX_PAIRS */
} orbg_problem;

/* What OptimizeSim3 leaves. */
typedef struct orbg_result {
    double q[4], t[3], s;           /* the g2o::Sim3 left in g2oS12 (x y z w); the INPUT's when ret0 */
    float S12[16];                  /* [sR | t; 0 0 0 1] narrowed, what Converter::toCvMat(Sim3) gives (row major) */
    int32_t ncorr, nbad, nin;       /* nCorrespondences, nBad of the first check, the return value */
    int32_t ret0;                   /* 1: the early `return 0` of :957-958 was taken */
    int32_t iters[2];               /* outer iterations each optimize() made */
} orbg_result;

/* The similarities of nproblems candidates.  `problems` is a HOST array (read during the call); the rest are device buffers with the shared cap
 * ncap >= every n, ncap >= 1.  Problem p's pairs are a table of ORBG_PAIR_ROWS rows of ncap floats at d_pairs + p*ORBG_PAIR_ROWS*ncap,
 * struct-of-arrays so that the lanes of a wave read consecutive floats:
 *   rows 0-2 P1c = R1w*P3D1w + t1w; 3-5 P2c = R2w*P3D2w + t2w; 6-8 u1, v1 of kpUn1 and w1 = pKF1->GetInvSigma2(octave1);
 *   9-11 u2, v2 of kpUn2 and w2 = pKF2->GetSigma2(octave2).
 * d_S12 + p*13: R row major (9), t (3), s: the arguments of g2o::Sim3(R, t, s).
 * Outputs: d_result[p]; d_removed[p*ORBO_WORDS(ncap) + w] for w < ORBO_WORDS(n): bit i set when vpMatches1[vnIndexEdge[i]] ends up NULL through
 * either check, 64 per word in index order, zero bits past n; d_trace + p*ORBG_MAX_ITERS (may be NULL).  Asynchronous on `stream`; allocates
 * nothing. */
int orbg_sim3_batch_device(const orbg_problem* problems, int nproblems, const float* d_pairs, int ncap, const float* d_S12, orbg_result* d_result,
                           uint64_t* d_removed, orbo_step* d_trace, void* stream);

/* One candidate, synchronous, HOST arrays in and out: P1c[n*3], P2c[n*3], obs1[n*3] (u1 v1 w1), obs2[n*3] (u2 v2 w2) (may be NULL when n == 0),
 * S12[13]; result, removed[ORBO_WORDS(n)] (may be NULL when n == 0), trace[ORBG_MAX_ITERS] (may be NULL). */
int orbg_sim3(const orbg_problem* problem, const float* P1c, const float* P2c, const float* obs1, const float* obs2, const float* S12,
              orbg_result* result, uint64_t* removed, orbo_step* trace, int device);

/* The same for nproblems candidates: ONE launch for all of them and one synchronisation.  Per candidate p the arrays P1c[p] ... as in orbg_sim3;
 * S12 is nproblems*13 floats, results an array of nproblems; trace may be NULL, and so may its entries.  Every candidate gets, byte for byte, what
 * orbg_sim3 gives it alone. */
int orbg_sim3_batch(const orbg_problem* problems, int nproblems, const float* const* P1c, const float* const* P2c, const float* const* obs1,
                    const float* const* obs2, const float* S12, orbg_result* results, uint64_t* const* removed, orbo_step* const* trace, int device);

#ifdef __cplusplus
}
#endif
#endif
