/* orbh.h — C ABI of loop closing's Sim3 RANSAC, Horn's closed form (part of liborbx.so).
 *
 * What Sim3Solver computes for LoopClosing::ComputeSim3 between SearchByBoW and SearchBySim3: every three-point hypothesis of every candidate
 * fitted and scored in one launch, and the walk of iterate() over the counts in a second.
 *
 * Reference interface replaced (paths relative to the reference ORB_SLAM tree):
 *   orbh_ransac_parameters          <- Sim3Solver::SetRansacParameters                                  src/Sim3Solver.cc:114-138
 *   orbh_max_errors                 <- the two push_backs into std::vector<size_t>                      src/Sim3Solver.cc:87-88, include/Sim3Solver.h:79-80
 *   orbh_hypotheses[_batch_device]  <- computeT with centroid                                           src/Sim3Solver.cc:215-332
 *                                      CheckInliers with Project                                        src/Sim3Solver.cc:335-359, :377-398
 *   orbh_select[_batch_device]      <- the decisions of Sim3Solver::iterate                             src/Sim3Solver.cc:140-207
 *   orbh_iterate[_batch]            <- calls of Sim3Solver::iterate after their draw (of several solvers)  src/Sim3Solver.cc:140-207
 * What stays with the caller: the correspondences (:37-112), FromCameraToImage (:400-418), the draw of the sets (:163-177; the sets are an
 * INPUT), vbInliers by index of vpMatched12.
 *
 * ---- the range of a call ----
 * The loop condition of :158 is `mnIterations<mRansacMaxIts && nCurrentIterations<nIterations`.  The caller passes a number of iterations
 * and one set per iteration; every hypothesis is independent of the others, so one launch computes what the reference computes serially.
 * The walk stops where the reference would have returned, or where mnIterations reaches mRansacMaxIts.
 *
 * ---- the fit: EXACT in float, operation for operation with no contraction, as the stand-in cv::Mat arithmetic this project pins its
 * projections to defines it (a product accumulates `float s = 0; s += a*b` in k order; Mat*double and Mat/double are (float)((double)p*s)
 * and (float)((double)p/s); dot() is a double sum from 0 in row-major order) ----
 *   centroid (:215-224): the row sum ((P[r][0] + P[r][1]) + P[r][2]) in float, C = (float)((double)sum/3), Pr = P - C;
 *   M = Pr2*Pr1.t();
 *   the ten entries of N (:251-260): sums of FLOAT operands and therefore float sums, left to right as written (`-M00+M11-M22` is
 *       ((-M00)+M11)-M22); their widening to double and narrowing into the float N (:262-265) changes nothing;
 *   P3 = R*Pr2; nom = Pr1.dot(P3); den = the double sum in row-major order of the float squares P3*P3 (cv::pow(P3,2)); ms12i = (float)(nom/den);
 *   sR = ms12i*R; t12 = O1 - sR*O2; sRinv = (1.0/ms12i)*R.t(); tinv = (-sRinv)*t12; T12 and T21 with the last row 0 0 0 1.
 *
 * NOT PINNED TO OPENCV (next to the deviations of orbt.h, orbi.h and orbe.h):
 *   cv::eigen of the float 4 x 4 N is the cyclic Jacobi iteration of orb_jacobi.h (rotate<P, Q>, the sweep order and the convergence rule of
 *       null_vector) in double on the widened N.  The quaternion q is the eigenvector of the LARGEST eigenvalue, the first of equal ones.
 *   Its sign is the one that makes q[0] >= 0 (q is negated when q[0] < 0): q and -q are the same rotation, but not the same floats.
 *   cv::Rodrigues of vec = 2*ang*vec/norm(vec), ang = atan2(norm(vec), q[0]) (:274-284) is the closed form of that rotation in double from
 *       the double quaternion, with a = q[0], (b, c, d) = q[1..3], aa = a*a, ..., vv = (bb + cc) + dd, n2 = aa + vv:
 *           R = [ (aa+bb)-(cc+dd)  2(bc-ad)         2(bd+ac)
 *                 2(bc+ad)         (aa+cc)-(bb+dd)  2(cd-ab)
 *                 2(bd-ac)         2(cd+ab)         (aa+dd)-(bb+cc) ] / n2.
 *       It is the rotation by 2*ang about vec/norm(vec); evaluated without atan2, sin and cos the device and the host route agree on it bit for
 *       bit.  The division by n2 stands for the reference's vec/norm(vec).
 *   R12 is rounded to float once.  Everything after it is the float text above.
 *
 * ---- degenerate input ----
 *   A set that names an index outside [0, N): NaN q and transforms, count 0, zero flags.
 *   norm(vec) == 0 (vv == 0: the two triples are equal, or N is zero or holds a NaN and the iteration leaves q = (1, 0, 0, 0)):
 *       the reference divides 0 by 0; here R12 is NaN in every entry, so is everything after it, every comparison fails and the count is 0.
 *   A repeated index in a set and three collinear points are legal input (the reference's draw produces the first): N then has a repeated
 *       largest eigenvalue and q is whichever of its eigenvectors the iteration leaves — arbitrary as the reference's, but a function of the
 *       inputs alone, the same on the device, the host route and the numpy restatement.
 *   Every NaN written is the canonical quiet NaN (0x7fc00000, 0x7ff8000000000000).
 *
 * ---- CheckInliers: EXACT ----
 *   Project (:377-398): x = ((0 + T00*X) + T01*Y) + T02*Z, then + T03; invz = 1/z; u = fx*(x*invz) + cx, all float.  err = (float)(the double
 *   sum d0*d0 + d1*d1 from 0).  mvnMaxError1/2 are std::vector<size_t>: 9.210*sigma2 is truncated to an integer (orbh_max_errors) and
 *   `err < (float)that` is the test.  An inlier passes both; a NaN passes neither.
 *
 * Arguments are checked on the host before anything touches the GPU.  Status codes are orbx.h's; there is no CPU fallback.
 */
#ifndef ORBH_H
#define ORBH_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBH_MAX_PROBLEMS 32        /* solvers of one call */
#define ORBH_MAX_POINTS   8192      /* N */
#define ORBH_MAX_ITERS    1024      /* iterations of one call */
#define ORBH_POINT_ROWS   12        /* rows of a problem's point table on the device */
#define ORBH_WORDS(n)     (((n) + 63) / 64)   /* flag words of n correspondences: bit i % 64 of word i / 64 */

/* One solver's call. */
typedef struct orbh_problem {
    float fx1, fy1, cx1, cy1;       /* mK1: pKF1's camera */
    float fx2, fy2, cx2, cy2;       /* mK2 */
    int32_t n;                      /* N: 3 .. ORBH_MAX_POINTS */
    int32_t iters;                  /* iterations of the call: 1 .. ORBH_MAX_ITERS */
    int32_t min_inliers;            /* mRansacMinInliers */
    int32_t max_its;                /* mRansacMaxIts (after SetRansacParameters) */
} orbh_problem;

/* One hypothesis: what computeT leaves in the members (row major). */
typedef struct orbh_hyp {
    double q[4];                    /* the quaternion R12 was made from (not a member of the reference) */
    float R[9], t[3], s;            /* mR12i, mt12i, ms12i */
    float T12[16], T21[16];         /* mT12i, mT21i */
    int32_t count;                  /* mnInliersi */
} orbh_hyp;

/* What a solver carries from call to call (next to its best flags, ORBH_WORDS(n) words). */
typedef struct orbh_state {
    int32_t iterations;             /* mnIterations */
    int32_t best_inliers;           /* mnBestInliers */
    float best_T12[16];             /* mBestT12 */
    float best_R[9], best_t[3];     /* mBestRotation, mBestTranslation */
    float best_s;                   /* mBestScale */
} orbh_state;

/* What one call of iterate() returns. */
typedef struct orbh_result {
    int32_t found;                  /* 1: mBestT12 is returned (:192-199); 0: an empty matrix */
    int32_t stop;                   /* the iteration of the range (0-based) at which the call returned; the number walked when it ran to its end */
    int32_t no_more;                /* bNoMore */
    int32_t ninliers;               /* nInliers */
    float T12[16];                  /* the returned matrix; zeros when found == 0 */
} orbh_result;

/* SetRansacParameters (:114-138) with the source's types: the float epsilon = (float)min_inliers/n, pow(epsilon, 3) in double, one iteration
 * when min_inliers == n, max(1, min(nIterations, max_iterations)).  n >= 0.  Host only. */
int orbh_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int32_t* max_its_out);

/* mvnMaxError (:87-88): maxerr[i] = (float)(size_t)(9.210*sigma2[i]), the value the comparisons of :351 see.  Host only. */
int orbh_max_errors(int n, const float* sigma2, float* maxerr);

/* The hypotheses of nproblems calls.  `problems` is a HOST array (read during the call); the rest are device buffers with shared caps
 * ncap >= every n, icap >= every iters.  Problem p's points are a table of ORBH_POINT_ROWS rows of ncap floats at
 * d_points + p*ORBH_POINT_ROWS*ncap, struct-of-arrays so that the lanes of a wave read consecutive floats:
 *   rows 0-2 x, y, z of mvX3Dc1; 3-5 of mvX3Dc2; 6-7 u, v of mvP1im1; 8-9 of mvP2im2; 10 maxerr1; 11 maxerr2.
 * d_sets + (p*icap + it)*3: the three indices of iteration it.
 * Outputs of (problem p, iteration it < iters) at s = p*icap + it (entries past a problem's own counts are left alone):
 *   d_hyp[s]; d_flags[s*ORBH_WORDS(ncap) + w] for w < ORBH_WORDS(n): mvbInliersi, 64 per word in index order, zero bits past n.
 * Asynchronous on `stream`; allocates nothing. */
int orbh_hypotheses_batch_device(const orbh_problem* problems, int nproblems, const float* d_points, int ncap, const int32_t* d_sets, int icap,
                                 orbh_hyp* d_hyp, uint64_t* d_flags, void* stream);

/* One problem, synchronous, HOST arrays in and out (ncap = n, icap = iters): x3dc1[n*3], x3dc2[n*3], p1im1[n*2], p2im2[n*2], maxerr1[n],
 * maxerr2[n], sets[iters*3]; hyp[iters], flags[iters*ORBH_WORDS(n)]. */
int orbh_hypotheses(const orbh_problem* problem, const float* x3dc1, const float* x3dc2, const float* p1im1, const float* p2im2, const float* maxerr1,
                    const float* maxerr2, const int32_t* sets, orbh_hyp* hyp, uint64_t* flags, int device);

/* The walk of :140-207 over the hypotheses.  Per problem p: the state d_state[p] with its best flags d_best_flags + p*ORBH_WORDS(ncap), updated in
 * place so that a later call continues where this one stopped.  n < min_inliers: no_more, nothing walked (:146-150).  Otherwise, in iteration
 * order while iterations < max_its: iterations advances by one; a count >= best_inliers is taken as the best (count, flags, T12, R, t, s — the
 * source's `>=`); if it is also > min_inliers the call returns there with found = 1.  At the end no_more = iterations >= max_its.
 * Outputs: d_result[p], d_result_flags[p*ORBH_WORDS(ncap) + w] for w < ORBH_WORDS(n) (by correspondence; zeros when found == 0).
 * Asynchronous on `stream`; allocates nothing. */
int orbh_select_batch_device(const orbh_problem* problems, int nproblems, int ncap, int icap, const orbh_hyp* d_hyp, const uint64_t* d_flags,
                             orbh_state* d_state, uint64_t* d_best_flags, orbh_result* d_result, uint64_t* d_result_flags, void* stream);
int orbh_select(const orbh_problem* problem, const orbh_hyp* hyp, const uint64_t* flags, orbh_state* state, uint64_t* best_flags, orbh_result* result,
                uint64_t* result_flags, int device);

/* One call of iterate() for one solver, HOST arrays, synchronous: the two device calls above on one stream with one synchronisation.
 * state and best_flags[ORBH_WORDS(n)] are read and updated.  hyp[iters] and flags[iters*ORBH_WORDS(n)] receive every hypothesis of the range,
 * also those past the iteration at which the walk stopped (either may be NULL). */
int orbh_iterate(const orbh_problem* problem, const float* x3dc1, const float* x3dc2, const float* p1im1, const float* p2im2, const float* maxerr1,
                 const float* maxerr2, const int32_t* sets, orbh_state* state, uint64_t* best_flags, orbh_result* result, uint64_t* result_flags,
                 orbh_hyp* hyp, uint64_t* flags, int device);

/* The same for nproblems solvers: ONE chain of the two device calls for all of them and one synchronisation (what Sim3Solver::Prefetch uses).
 * Per solver p the arrays x3dc1[p] ... as in orbh_iterate; states[p] and results[p] are arrays of nproblems; hyp and flags may be NULL, and so may
 * their entries.  Every solver gets, bit for bit, what orbh_iterate gives it alone. */
int orbh_iterate_batch(const orbh_problem* problems, int nproblems, const float* const* x3dc1, const float* const* x3dc2, const float* const* p1im1,
                       const float* const* p2im2, const float* const* maxerr1, const float* const* maxerr2, const int32_t* const* sets,
                       orbh_state* states, uint64_t* const* best_flags, orbh_result* results, uint64_t* const* result_flags, orbh_hyp* const* hyp,
                       uint64_t* const* flags, int device);

#ifdef __cplusplus
}
#endif
#endif
