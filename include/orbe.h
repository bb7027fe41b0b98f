/* orbe.h — C ABI of the relocalisation's EPnP RANSAC (part of liborbx.so).
 *
 * What PnPsolver computes for Tracking::Relocalisation between the searches: every four-point EPnP hypothesis of one iterate() call fitted and
 * scored in one launch, Refine (EPnP over all inliers) for every iteration that sets a new best in a second, and the walk of iterate() over
 * both in a third.
 *
 * Reference interface replaced (paths relative to the reference ORB_SLAM tree):
 *   orbe_ransac_parameters          <- PnPsolver::SetRansacParameters                                   src/PnPsolver.cc:122-158
 *   orbe_hypotheses[_batch_device]  <- the body of the loop of PnPsolver::iterate after the draw        src/PnPsolver.cc:204-208
 *                                      compute_pose and everything it calls                             src/PnPsolver.cc:376-951
 *                                      CheckInliers                                                     src/PnPsolver.cc:309-340
 *   orbe_refine[_batch_device]      <- PnPsolver::Refine                                                src/PnPsolver.cc:261-306
 *   orbe_refit[_batch_device]       <- the same over planted flag arrays (the n-point fit on its own)
 *   orbe_select[_batch_device]      <- the decisions of PnPsolver::iterate                              src/PnPsolver.cc:183-258
 *   orbe_iterate[_batch]            <- one call of PnPsolver::iterate after its draw (of several solvers)  src/PnPsolver.cc:166-259
 * What stays with the caller: the correspondences (:68-111), the draw of the sets (:189-202; the sets are an INPUT), vbInliers by key point.
 *
 * ---- the range of a call ----
 * The loop condition of :183 is `mnIterations<mRansacMaxIts || nCurrentIterations<nIterations`: a call covers the iterations
 * [mnIterations, max(mRansacMaxIts, mnIterations + nIterations)) unless a Refine succeeds earlier.  The caller passes the length of that
 * range as orbe_problem.iters and one set per iteration.  Every hypothesis of the range is independent of the others, so one launch
 * computes what the reference computes serially; the walk then stops where the reference would have returned.
 *
 * ---- the fit ----
 * EXACT, operation for operation in double with no contraction: fill_M, compute_L_6x10 (with its `2.0f *`), compute_rho, the sign and branch
 * logic of find_betas_approx_1/2/3, compute_A_and_b_gauss_newton, qr_solve (with its `eta == 0` return that leaves X as it was; X starts as
 * zeros here, the source leaves it uninitialised), the five Gauss-Newton steps, compute_ccs, compute_pcs, solve_for_sign (pcs[2] of the first
 * correspondence), the determinant fix and t of estimate_R_and_t, reprojection_error, and the two `<` that choose among the three branches
 * (a NaN error loses).
 *
 * THE DEVIATION (next to the ones of orbt.h and orbi.h): the decompositions.
 *   cvSVD of the symmetric PW0'PW0 (3 x 3) and M'M (12 x 12) is the cyclic Jacobi iteration of orb_jacobi.h in double; eigenvalues sorted
 *       descending, the first of equal ones first; dc = |eigenvalue|; row r of ut = the eigenvector of the r-th eigenvalue with whatever
 *       sign the iteration leaves, except that each row of uct (the three axes of the control points) is given the sign that makes its
 *       component of largest magnitude (the first of equal ones) positive, so that two decompositions choose the same control points.  The
 *       four vectors the fit uses are v[i] = ut + 12*(11 - i), i = 0..3.
 *   cvSVD of ABt is orbj::svd3 (R = U*V').  Where its smallest singular value is below 1e-4 of the largest (four nearly coplanar points) svd3
 *       takes the cross product of the first two left vectors for the third; the fit gives that vector the sign of ABt*v3, as a decomposition has it.
 *   cvInvert(CV_SVD) of the 3 x 3 CC and cvSolve(CV_SVD) of the 6 x 3/4/5 systems are minimum-norm least-squares solutions in double:
 *       with G = A'A = V diag(l) V' from the same iteration, x = sum over the columns i (in the iteration's order) with
 *       l[i] > ORBE_LSQ_CUT * max(l) of v_i * ((v_i . A'b) / l[i]); the inverse is the same with A' in place of A'b.
 *   WITH n = 4 THE FIT IS NOT DETERMINED BY ITS INPUTS: M is 8 x 12, M'M has an exact four-dimensional null space, and the four vectors are
 *       whichever basis of it the decomposition leaves.  Another basis changes most poses by more than 1e-6 and some inlier flags.  The
 *       RANSAC therefore equals the reference's in distribution, never iteration by iteration.  From the same four vectors everything
 *       downstream is stable.  With n = 5 two dimensions of the null space remain (M is 10 x 12) and v[0], v[1] are free in the same way; from
 *       n = 6 on Refine has distinct small eigenvalues and does not depend on the signs of its vectors.
 *   The sums over correspondences (the centroid, PW0'PW0, M'M, pc0 / pw0, ABt, the reprojection error) are double sums in ONE FIXED ORDER
 *       shared by the device, the host route and the numpy restatement: partial l (l = 0..63) = 0.0 + the terms of the correspondences at
 *       positions l, l + 64, l + 128, ... of the fit's list in that order; the sum = 0.0 + partial 0 + partial 1 + ... + partial
 *       (min(n, 64) - 1), left to right.  For n <= 64, and so for n = 4, that is index order.  The term of M'M[i][j] of one correspondence
 *       is M1[i]*M1[j] + M2[i]*M2[j] over its two rows of fill_M; that of PW0'PW0[i][j] is (pw[i] - c[i])*(pw[j] - c[j]); that of ABt is
 *       the source's product; that of the error is the source's sqrt.
 *
 * ---- CheckInliers: EXACT, with the source's mix (:318-330) ----
 *   Xc, Yc = double sums left to right, rounded to float; invZc = (float)(1/(double sum)); ue = uc + (fu*Xc)*invZc in double;
 *   distX = (float)(P2D.x - ue); error2 = distX*distX + distY*distY in float; inlier when error2 < maxerr[i].  A NaN is never an inlier.
 *
 * A set that names an index outside [0, N) gets a NaN pose, NaN errors, branch 0, count 0 and zero flags.  Repeated indices in a set are
 * legal input: the reference's draw produces them.
 *
 * Arguments are checked on the host before anything touches the GPU.  Status codes are orbx.h's; there is no CPU fallback.
 */
#ifndef ORBE_H
#define ORBE_H

#include <stddef.h>
#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBE_MAX_PROBLEMS 32        /* solvers of one call */
#define ORBE_MAX_POINTS   8192      /* N */
#define ORBE_MAX_ITERS    1024      /* iterations of one call */
#define ORBE_LSQ_CUT      1e-12     /* relative cut-off on the eigenvalues of A'A in the least-squares solves */

#define ORBE_KIND_NONE    0         /* iterate() returns an empty matrix */
#define ORBE_KIND_BEST    1         /* mBestTcw (:242-255) */
#define ORBE_KIND_REFINED 2         /* mRefinedTcw (:227-237) */

/* One solver's call. */
typedef struct orbe_problem {
    float fu, fv, uc, vc;           /* F.fx, F.fy, F.cx, F.cy (widened to double as :105-108) */
    int32_t n;                      /* N: 4 .. ORBE_MAX_POINTS */
    int32_t iters;                  /* length of the call's range: 1 .. ORBE_MAX_ITERS */
    int32_t min_inliers;            /* mRansacMinInliers (after SetRansacParameters) */
    int32_t max_its;                /* mRansacMaxIts (after SetRansacParameters) */
} orbe_problem;

/* What a solver carries from call to call (next to its two flag arrays of N bytes: the best's and its Refine's). */
typedef struct orbe_state {
    int32_t iterations;             /* mnIterations */
    int32_t best_inliers;           /* mnBestInliers */
    int32_t refine_ok;              /* Refine() of the current best returned true */
    int32_t refined_inliers;        /* mnRefinedInliers of that Refine */
    float best_tcw[12];             /* rows 0-2 of mBestTcw, row major 3 x 4 */
    float refined_tcw[12];          /* rows 0-2 of mRefinedTcw of that Refine */
} orbe_state;

/* What one call of iterate() returns. */
typedef struct orbe_result {
    int32_t kind;                   /* ORBE_KIND_* */
    int32_t stop;                   /* the iteration of the range (0-based) at which the call returned; iters when it ran to the end */
    int32_t no_more;                /* bNoMore */
    int32_t ninliers;               /* nInliers */
    float tcw[12];                  /* rows 0-2 of the returned matrix: each double rounded once, as convertTo(CV_32F); zeros for NONE */
} orbe_result;

/* SetRansacParameters (:122-158) with the source's types.  sigma2[n] = mvSigma2.  Outputs: *min_inliers_out = mRansacMinInliers,
 * *max_its_out = mRansacMaxIts, *epsilon_out = mRansacEpsilon, maxerr[n] = sigma2[i]*th2 in float.  n >= 1.  Host only. */
int orbe_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2,
                           const float* sigma2, int32_t* min_inliers_out, int32_t* max_its_out, float* epsilon_out, float* maxerr);

/* The hypotheses of nproblems calls.  `problems` is a HOST array (read during the call); the rest are device buffers with shared caps
 * ncap >= every n, icap >= every iters.  Problem p: d_p3d + p*ncap*3 (float x, y, z), d_p2d + p*ncap*2, d_maxerr + p*ncap,
 * d_sets + p*icap*4 (int32 indices into the correspondences).
 * Outputs of (problem p, iteration it < iters) at s = p*icap + it (entries past a problem's own counts are left alone):
 *   d_R[s*9] (row major), d_t[s*3], d_err[s*3] the reprojection errors of the three branches, d_branch[s] the branch chosen (1..3),
 *   d_vecs[s*48] the four vectors v[0..3] (may be NULL), d_count[s] mnInliersi, d_flags[s*ncap + i] mvbInliersi for i < n.
 * Asynchronous on `stream`; allocates nothing. */
int orbe_hypotheses_batch_device(const orbe_problem* problems, int nproblems, const float* d_p3d, const float* d_p2d, const float* d_maxerr, int ncap,
                                 const int32_t* d_sets, int icap, double* d_R, double* d_t, double* d_err, int32_t* d_branch, double* d_vecs,
                                 int32_t* d_count, uint8_t* d_flags, void* stream);

/* One problem, synchronous, HOST arrays in and out (ncap = n, icap = iters). */
int orbe_hypotheses(const orbe_problem* problem, const float* p3d, const float* p2d, const float* maxerr, const int32_t* sets, double* R, double* t,
                    double* err, int32_t* branch, double* vecs, int32_t* count, uint8_t* flags, int device);

/* Refine for every iteration that is a RECORD: d_count[s] >= min_inliers, greater than every earlier d_count of the problem's range and
 * greater than d_state[p].best_inliers.  The fit runs over the flagged correspondences of d_flags[s*ncap ..] in index order, then
 * CheckInliers over all n.  Outputs per record: d_rR[s*9], d_rt[s*3], d_rcount[s], d_rflags[s*ncap + i], d_rok[s] = d_rcount[s] > min_inliers
 * (the strict `>` of :293).  Non-records are left alone.  A record with fewer than 4 flagged correspondences cannot occur
 * (min_inliers >= 4).  Asynchronous on `stream`; allocates nothing. */
int orbe_refine_batch_device(const orbe_problem* problems, int nproblems, const float* d_p3d, const float* d_p2d, const float* d_maxerr, int ncap,
                             int icap, const int32_t* d_count, const uint8_t* d_flags, const orbe_state* d_state, double* d_rR, double* d_rt,
                             int32_t* d_rcount, uint8_t* d_rflags, int32_t* d_rok, void* stream);

/* One problem, synchronous, HOST arrays; best_in = the best count carried in. */
int orbe_refine(const orbe_problem* problem, const float* p3d, const float* p2d, const float* maxerr, const int32_t* count, const uint8_t* flags,
                int best_in, double* rR, double* rt, int32_t* rcount, uint8_t* rflags, int32_t* rok, int device);

/* The same fit over PLANTED flag arrays, one per (problem, slot < iters): d_flags_in[s*ncap + i].  Outputs as above plus d_rvecs[s*48] (may be
 * NULL).  An array with fewer than 4 flags set gets a NaN pose, count 0 and ok 0. */
int orbe_refit_batch_device(const orbe_problem* problems, int nproblems, const float* d_p3d, const float* d_p2d, const float* d_maxerr, int ncap,
                            int icap, const uint8_t* d_flags_in, double* d_rR, double* d_rt, double* d_rvecs, int32_t* d_rcount, uint8_t* d_rflags,
                            int32_t* d_rok, void* stream);
int orbe_refit(const orbe_problem* problem, const float* p3d, const float* p2d, const float* maxerr, const uint8_t* flags_in, double* rR, double* rt,
               double* rvecs, int32_t* rcount, uint8_t* rflags, int32_t* rok, int device);

/* The walk of :183-258 over the results of the two calls above.  Per problem p: the state d_state[p] with its flag arrays
 * d_best_flags + p*ncap and d_refined_flags + p*ncap, all updated in place so that a later call continues where this one stopped.
 * In iteration order, for a count >= min_inliers: take it as best (count, flags, float Tcw, and its Refine's ok, pose, count, flags) when it
 * is > the best; then return at this iteration with the best's refined result if the best's Refine is ok.  iterations advances by one per
 * iteration walked.  At the end of the range no_more = iterations >= max_its; then the best is returned if best_inliers >= min_inliers.
 * Outputs: d_result[p], d_result_flags[p*ncap + i] for i < n (by correspondence; zeros for NONE).
 * Asynchronous on `stream`; allocates nothing. */
int orbe_select_batch_device(const orbe_problem* problems, int nproblems, int ncap, int icap, const double* d_R, const double* d_t,
                             const int32_t* d_count, const uint8_t* d_flags, const double* d_rR, const double* d_rt, const int32_t* d_rcount,
                             const uint8_t* d_rflags, const int32_t* d_rok, orbe_state* d_state, uint8_t* d_best_flags, uint8_t* d_refined_flags,
                             orbe_result* d_result, uint8_t* d_result_flags, void* stream);
int orbe_select(const orbe_problem* problem, const double* R, const double* t, const int32_t* count, const uint8_t* flags, const double* rR,
                const double* rt, const int32_t* rcount, const uint8_t* rflags, const int32_t* rok, orbe_state* state, uint8_t* best_flags,
                uint8_t* refined_flags, orbe_result* result, uint8_t* result_flags, int device);

/* One call of iterate() for one solver, HOST arrays, synchronous: the three device calls above on one stream with one synchronisation.
 * state, best_flags[n] and refined_flags[n] are read and updated. */
int orbe_iterate(const orbe_problem* problem, const float* p3d, const float* p2d, const float* maxerr, const int32_t* sets, orbe_state* state,
                 uint8_t* best_flags, uint8_t* refined_flags, orbe_result* result, uint8_t* result_flags, int device);

/* The next iterate() of nproblems solvers, HOST arrays, synchronous: ONE chain of the three device calls for all of them and one synchronisation (what
 * PnPsolver::Prefetch uses).  Per solver p: p3d[p], p2d[p], maxerr[p], sets[p], best_flags[p], refined_flags[p], result_flags[p] as in orbe_iterate;
 * states[p] and results[p] are arrays of nproblems.  Every solver gets, bit for bit, what orbe_iterate gives it alone. */
int orbe_iterate_batch(const orbe_problem* problems, int nproblems, const float* const* p3d, const float* const* p2d, const float* const* maxerr,
                       const int32_t* const* sets, orbe_state* states, uint8_t* const* best_flags, uint8_t* const* refined_flags, orbe_result* results,
                       uint8_t* const* result_flags, int device);

#ifdef __cplusplus
}
#endif
#endif
