/* orbi.h — C ABI of the monocular initialisation (part of liborbx.so).
 *
 * What Initializer::Initialize computes between ORBmatcher::SearchForInitialization and the first map: the RANSAC over homographies and
 * fundamental matrices (every hypothesis fitted and scored in one launch, the winners selected in a second) and CheckRT (the
 * triangulation and the tests of every inlier under every motion hypothesis in one launch).
 *
 * Reference interface replaced (paths relative to the reference ORB_SLAM tree):
 *   orbi_normalize                  <- Initializer::Normalize                                           src/Initializer.cc:747-793
 *   orbi_models[_batch_device]      <- Initializer::FindHomography, FindFundamental                     src/Initializer.cc:122-170, :173-221
 *                                      ComputeH21, ComputeF21                                           src/Initializer.cc:224-264, :266-301
 *                                      CheckHomography, CheckFundamental                                src/Initializer.cc:303-386, :388-466
 *   orbi_pose_from_rt               <- the head of CheckRT (P2 = K*[R|t], O2 = -R.t()*t)                src/Initializer.cc:812-824
 *   orbi_check_rt[_batch_device]    <- Initializer::CheckRT with Triangulate                            src/Initializer.cc:796-905, :732-745
 *                                      for the 4 calls of ReconstructF (:492-495) or the 8 of ReconstructH (:696-716)
 * What stays with the caller: the match list and the RANSAC sets (:51-95; the sets are an INPUT, drawn as :80-95 draws them),
 * RH = SH/(SH+SF) and the 0.40 rule (:110-116), DecomposeE and the Faugeras decomposition, the sort of vCosParallax and
 * acos(...)*180/CV_PI (:896-899), and the acceptance rules of :497-567 and :719-729.
 *
 * ---- models ----
 * Per problem: the undistorted key points of both frames, the match list mvMatches12 as int32 [N][2] = (index in frame 1, index in
 * frame 2), the sets as int32 [iters][8] of indices into the match list, norm1 / norm2 = {sX, sY, meanX, meanY} of Normalize over ALL key
 * points of the frame, and sigma.
 *
 * Per iteration, the fit.  THE DEVIATION (next to the one of orbt.h): the reference takes vt.row(8) of OpenCV's single-precision
 * cv::SVDecomp of its 16 x 9 (ComputeH21) and 8 x 9 (ComputeF21) matrices, a second cv::SVDecomp of the 3 x 3 Fpre, and float cv::Mat
 * products and inverses around them.  That routine is not restated here.  Instead:
 *   the normalised points of the set are (x - meanX)*sX, (y - meanY)*sY: two float operations each, as :769-785;
 *   A is filled in float exactly as the source does (:237-255, :279-287);
 *   Hn = the unit right singular vector of A for its smallest singular value, computed in DOUBLE (cyclic Jacobi on the 9 x 9 matrix
 *       A'A, whose entries are double sums of double products of the float entries in row order) and rounded to float; its sign is
 *       whatever the iteration leaves;
 *   H21i = inv(T2)*Hn*T1 evaluated in double from the float T1, T2 (T = [sX 0 -meanX*sX; 0 sY -meanY*sY; 0 0 1], the two products in
 *       float as :791-792) and the float Hn, rounded once to float; inv(T2) = [1/sX 0 -T02/sX; 0 1/sY -T12/sY; 0 0 1] in double;
 *   H12i = the inverse in double (adjugate over determinant) of the float H21i, rounded to float;
 *   Fpre is taken from its A as Hn is; Fn = Fpre with its smallest singular value set to zero, from a 3 x 3 decomposition in double
 *       (Fn = Fpre - (Fpre*v)*v' with v the eigenvector of Fpre'Fpre for its smallest eigenvalue); F21i = T2'*Fn*T1 in double, rounded
 *       to float.
 * A caller may see last-bit differences of the matrices against an OpenCV build, and more than that for 8-point sets whose A is nearly
 * rank-deficient, where the reference's own answer is ill-determined too.
 *
 * Per iteration, the scores: EXACT.  From the float H21i, H12i, F21i, one IEEE operation per operation of :335-383 and :411-463, in the
 * source's order, no contraction, with the source's promotions: `1.0/(...)` is a double division of the float sum, assigned to float;
 * invSigmaSquare = (float)(1.0/(double)(sigma*sigma)); th = 5.991f, 3.841f, thScore = 5.991f.  score is a FLOAT SUM IN MATCH ORDER, for
 * each match the term of image 1 before the term of image 2; an excluded term adds nothing.  As in the source a NaN chi-square is not
 * `> th`: it is added, the score becomes NaN and the flag stays set.
 * Selection: best = the first iteration whose score exceeds every earlier one, from score = 0 with the strict `>` of :163 / :214; a NaN
 * score never wins; best = -1 (S = 0, flags all zero) when no score exceeds 0.
 * A match entry whose indices lie outside the frames is never dereferenced: both its terms are excluded.  An iteration whose set names
 * an index outside [0, N) or such a match gets zero matrices and score 0.
 *
 * ---- CheckRT ----
 * Per (hypothesis h, match entry i with flag[i] != 0), with kp1, kp2 the key points of the match:
 *   P1 = K*[I|0] = [fx 0 cx 0; 0 fy cy 0; 0 0 1 0]; A[0][c] = kp1.x*P1[2][c] - P1[0][c], A[1][c] = kp1.y*P1[2][c] - P1[1][c], rows 2 and
 *       3 the same with kp2 and the pose's P2: a float multiply followed by a float subtract;
 *   v = the null vector of A as in orbt.h (the same routine, THE ONE DEVIATION there); x3D[j] = v[j] / v[3] (float);
 *   a non-finite x3D: ORBI_RT_NONFINITE;
 *   dist1 = (float)sqrt(sum of (double)x3D[j]^2), normal2 = x3D - O2 (float), dist2 likewise; cosParallax =
 *       (float)(dot / (double)(dist1*dist2)) with dot the double sum of (double)x3D[j]*(double)normal2[j] in index order;
 *   x3D[2] <= 0 && (double)cosParallax < 0.99998: ORBI_RT_DEPTH1;
 *   p2 = R*x3D + t: p2[r] = (((0.0f + R[r][0]*x3D[0]) + R[r][1]*x3D[1]) + R[r][2]*x3D[2]) + t[r] (float);
 *   p2[2] <= 0 && (double)cosParallax < 0.99998: ORBI_RT_DEPTH2;
 *   invZ1 = (float)(1.0/(double)x3D[2]); im1x = fx*x3D[0]*invZ1 + cx, im1y = fy*x3D[1]*invZ1 + cy (float, left to right);
 *       (im1x-kp1.x)*(im1x-kp1.x) + (im1y-kp1.y)*(im1y-kp1.y) > th2: ORBI_RT_REPROJ1; the same with p2 and kp2: ORBI_RT_REPROJ2;
 *   otherwise the entry is counted in ngood[h] (the reference's nGood and vCosParallax.push_back): ORBI_RT_GOOD with good = 1 when
 *       (double)cosParallax < 0.99998, else ORBI_RT_COUNTED with good = 0.
 * As in the source, a NaN that is not in x3D fails every comparison and walks through.
 * An entry whose flag is zero: ORBI_RT_NONE; one whose indices lie outside the frames: ORBI_RT_SKIP_INDEX; both with zero outputs.
 *
 * Arguments are checked on the host before anything touches the GPU.  Status codes are orbx.h's; there is no CPU fallback.
 */
#ifndef ORBI_H
#define ORBI_H

#include <stddef.h>
#include <stdint.h>

#include "orbf.h"
#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBI_MAX_PROBLEMS 32        /* frame pairs of one call */
#define ORBI_MAX_MATCHES  16384     /* N */
#define ORBI_MAX_ITERS    1024
#define ORBI_MAX_HYP      8         /* motion hypotheses of one CheckRT call */

/* d_status values of orbi_check_rt* */
#define ORBI_RT_NONE       0        /* the flag of the entry is zero */
#define ORBI_RT_GOOD       1        /* counted, vbGood set */
#define ORBI_RT_COUNTED    2        /* counted (nGood, vCosParallax, vP3D), vbGood not set: cosParallax >= 0.99998 */
#define ORBI_RT_NONFINITE  3
#define ORBI_RT_DEPTH1     4
#define ORBI_RT_DEPTH2     5
#define ORBI_RT_REPROJ1    6
#define ORBI_RT_REPROJ2    7
#define ORBI_RT_SKIP_INDEX 8

/* One frame pair of orbi_models*. */
typedef struct orbi_problem {
    float norm1[4], norm2[4];       /* {sX, sY, meanX, meanY} of Normalize(mvKeys1), Normalize(mvKeys2): orbi_normalize */
    float sigma;
    int32_t n1, n2;                 /* key points of frame 1, frame 2 */
    int32_t nmatches;               /* N: 8 .. ORBI_MAX_MATCHES */
    int32_t iters;                  /* 1 .. ORBI_MAX_ITERS */
    int32_t reserved;               /* 0 */
} orbi_problem;

/* One motion hypothesis of orbi_check_rt*. */
typedef struct orbi_pose {
    float R[9];                     /* row major */
    float t[3];
    float P2[12];                   /* K*[R|t], row major 3 x 4 */
    float O2[3];                    /* -R.t()*t */
} orbi_pose;

/* Normalize (:747-793) over the n >= 1 key points of one frame, float sums in index order: out[4] = {sX, sY, meanX, meanY}.  Host only. */
int orbi_normalize(const orbx_keypoint* kps, int n, float* out);

/* Fills *pose from K = [fx 0 cx; 0 fy cy; 0 0 1], R[9] (row major) and t[3] with the cv::Mat evaluation order of DESIGN.md §2:
 * P2[i][j] = ((0.0f + K[i][0]*M[0][j]) + K[i][1]*M[1][j]) + K[i][2]*M[2][j] with M = [R|t]; O2[i] = ((0.0f + (-R[0][i])*t[0]) +
 * (-R[1][i])*t[1]) + (-R[2][i])*t[2].  Host only. */
int orbi_pose_from_rt(float fx, float fy, float cx, float cy, const float* R, const float* t, orbi_pose* pose);

/* Fits, scores and selects for nproblems independent frame pairs.  `problems` is a HOST array (read during the call); the rest are
 * device buffers with shared caps: kcap1 >= every n1, kcap2 >= every n2, mcap >= every nmatches, icap >= every iters.
 *   problem p: key points d_kps1 + p*kcap1 and d_kps2 + p*kcap2, matches d_matches + p*mcap*2, sets d_sets + p*icap*8.
 * Outputs of problem p (entries past the problem's own counts are left alone):
 *   d_scoreH[p*icap + it], d_scoreF[p*icap + it]; d_H21, d_H12, d_F21 [(p*icap + it)*9]; d_hn, d_fpre likewise (both may be NULL);
 *   d_best[p*2] = {bestH, bestF}; d_S[p*2] = {SH, SF}; d_inlH[p*mcap + i], d_inlF[p*mcap + i] the winners' flags for i < N.
 * Asynchronous on `stream`; allocates nothing. */
int orbi_models_batch_device(const orbi_problem* problems, int nproblems, const orbx_keypoint* d_kps1, int kcap1, const orbx_keypoint* d_kps2,
                             int kcap2, const int32_t* d_matches, int mcap, const int32_t* d_sets, int icap, float* d_scoreH, float* d_scoreF,
                             float* d_H21, float* d_H12, float* d_F21, float* d_hn, float* d_fpre, int32_t* d_best, float* d_S,
                             uint8_t* d_inlH, uint8_t* d_inlF, void* stream);

/* One frame pair, synchronous, HOST arrays in and out: matches[N*2], sets[iters*8]; scoreH[iters], scoreF[iters], H21, H12, F21
 * [iters*9], hn, fpre [iters*9] (both may be NULL), best[2], S[2], inlH[N], inlF[N]. */
int orbi_models(const orbi_problem* problem, const orbx_keypoint* kps1, const orbx_keypoint* kps2, const int32_t* matches, const int32_t* sets,
                float* scoreH, float* scoreF, float* H21, float* H12, float* F21, float* hn, float* fpre, int32_t* best, float* S,
                uint8_t* inlH, uint8_t* inlF, int device);

/* CheckRT for nhyp <= ORBI_MAX_HYP poses of nproblems <= ORBI_MAX_PROBLEMS frame pairs.  HOST arrays: n1[nproblems], n2[nproblems],
 * nmatches[nproblems] (0 .. ORBI_MAX_MATCHES).  Device buffers: d_poses[nproblems*nhyp]; key points and matches as in
 * orbi_models_batch_device; d_flags + p*mcap one byte per match entry (vbMatchesInliers).
 * Outputs of (problem p, hypothesis h), by match entry, at e = (p*nhyp + h)*mcap + i for i < nmatches[p]:
 *   d_status[e] ORBI_RT_*; d_x3d[e*3] x3D of every entry that got past ORBI_RT_NONFINITE, zeros otherwise; d_cos[e] cosParallax of
 *   the same entries; d_good[e] vbGood; d_v[e*4] (may be NULL; 16-byte aligned) the null vector of every flagged entry whose indices lie inside the frames
 *   (zeros for ORBI_RT_NONE and ORBI_RT_SKIP_INDEX);
 *   d_ngood[p*nhyp + h] nGood (every thread counts its own entries, thread 0 adds the workgroup's 256 counts from LDS: no atomics).
 * Asynchronous on `stream`; allocates nothing. */
int orbi_check_rt_batch_device(float fx, float fy, float cx, float cy, const orbi_pose* d_poses, int nhyp, int nproblems, const int32_t* n1,
                               const int32_t* n2, const int32_t* nmatches, const orbx_keypoint* d_kps1, int kcap1, const orbx_keypoint* d_kps2,
                               int kcap2, const int32_t* d_matches, int mcap, const uint8_t* d_flags, float th2, uint8_t* d_status,
                               float* d_x3d, float* d_cos, uint8_t* d_good, float* d_v, int32_t* d_ngood, void* stream);

/* One frame pair, synchronous, HOST arrays in and out: poses[nhyp], matches[N*2], flags[N]; status[nhyp*N], x3d[nhyp*N*3], cosp[nhyp*N],
 * good[nhyp*N], v[nhyp*N*4] (may be NULL), ngood[nhyp], and parallax[nhyp] = acos(c)*180/CV_PI (:896-902; 0 when nothing is counted)
 * with c the entry min(50, ngood - 1) of the sorted cosines of the counted entries. */
int orbi_check_rt(float fx, float fy, float cx, float cy, const orbi_pose* poses, int nhyp, const orbx_keypoint* kps1, int n1,
                  const orbx_keypoint* kps2, int n2, const int32_t* matches, int nmatches, const uint8_t* flags, float th2, uint8_t* status,
                  float* x3d, float* cosp, uint8_t* good, float* v, int32_t* ngood, float* parallax, int device);

#ifdef __cplusplus
}
#endif
#endif
