/* orbt.h — C ABI of the triangulation of new map points (part of liborbx.so).
 *
 * The loop behind ORBmatcher::SearchForTriangulation in LocalMapping::CreateNewMapPoints: for every match of a key-frame pair the
 * parallax of the two rays, the linear triangulation (the null vector of a 4 x 4 matrix) and the six tests in front of
 * `new MapPoint(x3D, ...)`.  The matches are read where orbs_triangulation_search_batch_device leaves them, the key points are the
 * device-resident undistorted ones, and the "has a MapPoint" flags both sides of the search read can be updated in place, so
 * search -> triangulate -> search -> ... over the neighbours of one key frame is one stream-ordered chain.
 *
 * Reference interface replaced (paths relative to the reference ORB_SLAM tree):
 *   orbt_triangulate[_batch_device] <- the body of the match loop of LocalMapping::CreateNewMapPoints   src/LocalMapping.cc:269-353
 *                                      and what its AddMapPoint calls (:360-361) mean to the NEXT search: idx1 holds a map point now
 *                                      (d_qvalid cleared), idx2 holds one now (d_claimed set)
 * What stays with the caller: the choice of neighbours and the baseline test (:230-243), ComputeF12, `new MapPoint`, AddObservation.
 * ComputeDistinctiveDescriptors and UpdateNormalAndDepth of the new points are orbp_refresh* (orbp.h), from the observation lists.
 *
 * Arithmetic, per match (idx1, idx2) with kp1 = KF1's undistorted key point idx1 and kp2 = KF2's idx2.  Every step is ONE IEEE
 * operation in the reference's order, no contraction; the cv::Mat primitives are evaluated as DESIGN.md §2 lists them:
 *   invfx = 1.0f / fx, invfy = 1.0f / fy (float);
 *   xn = ((x - cx) * invfx, (y - cy) * invfy, 1.0f) (float);
 *   ray = Rwc * xn with Rwc = the transpose of Rcw: ray[i] = ((0.0f + Rcw[0][i]*xn[0]) + Rcw[1][i]*xn[1]) + Rcw[2][i]*xn[2] (float);
 *   dot = sum of (double)ray1[i]*(double)ray2[i], norm = sqrt(sum of (double)ray[i]*(double)ray[i]), double sums from 0.0 in index order;
 *   cosParallax = (float)(dot / (norm1 * norm2));   cosParallax < 0 || (double)cosParallax > 0.9998 rejects (ORBT_PARALLAX);
 *   A[0][c] = xn1[0]*T1[2][c] - T1[0][c], A[1][c] = xn1[1]*T1[2][c] - T1[1][c], rows 2 and 3 the same with xn2 and T2, where
 *       T = [Rcw | tcw] (3 x 4): a float multiply followed by a float subtract;
 *   v = the right singular vector of A for its smallest singular value (see THE ONE DEVIATION below);
 *   v[3] == 0 rejects (ORBT_W_ZERO); x3D[i] = v[i] / v[3] (float division);
 *   z1 = (float)(((0.0 + (double)Rcw1[2][0]*(double)x3D[0]) + (double)Rcw1[2][1]*(double)x3D[1]) + (double)Rcw1[2][2]*(double)x3D[2] + (double)tcw1[2]);
 *       z1 <= 0 rejects (ORBT_DEPTH1); z2 likewise with KF2 (ORBT_DEPTH2);
 *   x1, y1 the same with rows 0 and 1; invz1 = (float)(1.0 / (double)z1); u1 = fx1*x1*invz1 + cx1, v1 = fy1*y1*invz1 + cy1, float, left
 *       to right; errX1 = u1 - kp1.x, errY1 = v1 - kp1.y; (double)(errX1*errX1 + errY1*errY1) > 5.991 * (double)sigma2_1[kp1.octave]
 *       rejects (ORBT_REPROJ1); the same in KF2 (ORBT_REPROJ2);
 *   dist1 = (float)sqrt(sum of (double)d[i]*(double)d[i]) with d = x3D - Ow1 in float; dist2 likewise; dist1 == 0 || dist2 == 0
 *       rejects (ORBT_ZERO_DIST);
 *   ratioDist = dist1 / dist2; ratioOctave = factors1[kp1.octave] / factors2[kp2.octave]; ratioFactor = 1.5f * scale_factor (floats);
 *   ratioDist*ratioFactor < ratioOctave || ratioDist > ratioOctave*ratioFactor rejects (ORBT_SCALE); otherwise ORBT_ACCEPTED.
 *
 * THE ONE DEVIATION: the null vector.  The reference takes vt.row(3) of OpenCV's single-precision cv::SVD::compute; that routine is
 * not restated here (DESIGN.md §2 lists it among the unpinned OpenCV primitives).  This library computes the null vector in DOUBLE
 * from the float A (cyclic Jacobi on the 4 x 4 matrix A'A, one lane per match) and rounds its four components to float; its sign is
 * whatever the iteration leaves.  Since x3D = v[0..2] / v[3], neither the sign nor the scale of v reaches x3D, but its last bits do: a
 * caller may see last-bit differences of x3D against an OpenCV build, and a different decision only where a tested quantity lies
 * within rounding of its threshold.  The iteration is exact to about 2^-52 * s1^2 / (s3^2 - s4^2) (s1 >= .. >= s4 the singular
 * values of A); where s3 and s4 nearly coincide the null vector is ill-determined in ANY precision.
 *
 * NaN (next to the NaN rule of orbp.h): the reference's comparisons all fail on a NaN, so a NaN would walk through its tests.  Here a
 * NaN anywhere in a match's chain rejects the match, with the status of the FIRST test whose quantity is NaN.
 *
 * Matches that cannot be evaluated are passed over, never dereferenced: idx2 outside [-1, n2) gets ORBT_SKIP_INDEX, an octave of
 * either key point outside [0, nlevels) ORBT_SKIP_OCTAVE (tested before the arithmetic: the reference would index mvLevelSigma2 out
 * of bounds after its depth tests).  A match entry whose idx1 is outside [0, n1) has no status slot and is ignored.
 *
 * Arguments are checked on the host before anything touches the GPU.  Status codes are orbx.h's; there is no CPU fallback.
 */
#ifndef ORBT_H
#define ORBT_H

#include <stddef.h>
#include <stdint.h>

#include "orbf.h"
#include "orbs.h"
#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBT_MAX_PAIRS (1 << 16)    /* pairs of one call */

/* d_status values */
#define ORBT_NONE        0          /* idx1 has no match */
#define ORBT_ACCEPTED    1          /* the reference reaches `new MapPoint(x3D, ...)` */
#define ORBT_PARALLAX    2
#define ORBT_W_ZERO      3
#define ORBT_DEPTH1      4
#define ORBT_DEPTH2      5
#define ORBT_REPROJ1     6
#define ORBT_REPROJ2     7
#define ORBT_ZERO_DIST   8
#define ORBT_SCALE       9
#define ORBT_SKIP_INDEX  10
#define ORBT_SKIP_OCTAVE 11

/* One key frame's pose and camera (the orbp_view fields the triangulation reads). */
typedef struct orbt_camera {
    float Rcw[9];                   /* GetRotation(), row major */
    float tcw[3];                   /* GetTranslation() */
    float Ow[3];                    /* GetCameraCenter() */
    float fx, fy, cx, cy;
} orbt_camera;

/* One (mpCurrentKeyFrame, pKF2) pair. */
typedef struct orbt_pair {
    orbt_camera kf1, kf2;
    float scale_factor;             /* mpCurrentKeyFrame->GetScaleFactor() (mfScaleFactor): ratioFactor = 1.5f * scale_factor */
    int32_t reserved;               /* 0 */
} orbt_pair;

/* Triangulates the matches of npairs independent pairs.  All arrays are device buffers except the four level tables (HOST pointers:
 * mvScaleFactors and mvLevelSigma2 of KF1 and of KF2, 1 <= nlevels <= ORBS_MAX_LEVELS; the same pointer may be passed for both).
 *   d_pairs[npairs].
 *   KF1 of pair p: key points d_kps1 + p*stride1 (undistorted, feature order), d_n1[stride1 ? p : 0] of them (clamped to [0, cap1]),
 *       flags d_qvalid + p*stride1.  stride1 == 0: every pair shares one KF1; otherwise stride1 >= cap1.
 *   KF2 of pair p: d_kps2 + p*cap2, d_n2[p] (clamped to [0, cap2]), flags d_claimed + p*cap2.
 *   Matches of pair p, as orbs_triangulation_search_batch_device leaves them: entry q < d_nq[p] (clamped to [0, qcap]) says that
 *       feature idx1 = d_qindex[p*qcap + q] of KF1 is matched to feature d_q2t[p*qcap + q] of KF2 (-1: none).  d_qindex == NULL: idx1 = q,
 *       that is d_q2t is vMatches12.  An idx1 must not be listed twice with a match (true of a FeatureVector's feature list).
 * Outputs of pair p, by feature of KF1 (entries idx1 < n1 are all written, the rest is left alone):
 *   d_status[p*cap1 + idx1]   ORBT_*;
 *   d_x3d[(p*cap1 + idx1)*3]  x3D of every match that got past ORBT_W_ZERO, zeros otherwise;
 *   d_v[(p*cap1 + idx1)*4]    (may be NULL) the null vector of every match that got past ORBT_PARALLAX, zeros otherwise;
 *   d_match12[p*cap1 + idx1]  the idx2 examined (vMatches12; -1 none): the kernel's own table between its passes, and of use to the caller.
 * The accepted matches of pair p, compacted in ascending idx1 (the order of the reference's vMatchedIndices when it is built from
 * vMatches12): d_acc_idx[(p*ocap + k)*2] = {idx1, idx2}, d_acc_x3d[(p*ocap + k)*3], k < d_count[p].  d_count[p] is always the true
 * number; when it exceeds ocap only the first ocap entries are written and d_overflow[p] = 1 (else 0).  Deterministic: ranks come from
 * ballots, not from atomics.
 * In place, either may be NULL: d_qvalid[idx1] = 0 ("has no MapPoint yet" of the search) at every accepted idx1, d_claimed[idx2] = 1 at
 * every accepted idx2, beyond ocap too; no other byte is written.  With stride1 == 0 all pairs of ONE call still see the flags as they
 * were on entry of their search: chain the calls (search p, triangulate p, search p + 1, ...) on one stream for the reference's order.
 * Asynchronous on `stream`; allocates nothing. */
int orbt_triangulate_batch_device(const orbt_pair* d_pairs, int npairs, const float* factors1, const float* sigma2_1, const float* factors2,
                                  const float* sigma2_2, int nlevels, const orbx_keypoint* d_kps1, const int32_t* d_n1, int cap1, int stride1,
                                  const orbx_keypoint* d_kps2, const int32_t* d_n2, int cap2, const int32_t* d_q2t, const int32_t* d_qindex,
                                  const int32_t* d_nq, int qcap, uint8_t* d_status, float* d_x3d, float* d_v, int32_t* d_match12,
                                  int32_t* d_acc_idx, float* d_acc_x3d, int32_t* d_count, int32_t* d_overflow, int ocap, uint8_t* d_qvalid,
                                  uint8_t* d_claimed, void* stream);

/* One pair, synchronous, HOST arrays in and out: the latency form.  match12[n1] is vMatches12; status[n1], x3d[3*n1], v[4*n1] (may be
 * NULL), acc_idx[2*ocap], acc_x3d[3*ocap], *count as above.  ORBX_ERR_CAPACITY when more than ocap matches are accepted (*count then
 * holds the number, the first ocap entries are written). */
int orbt_triangulate(const orbt_pair* pair, const float* factors1, const float* sigma2_1, const float* factors2, const float* sigma2_2,
                     int nlevels, const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, const int32_t* match12,
                     uint8_t* status, float* x3d, float* v, int32_t* acc_idx, float* acc_x3d, int ocap, int* count, int device);

/* ---- LocalMapping::CreateNewMapPoints over the rows of a resident key-frame store (orbs_tri_rows.hip): the whole neighbour loop in one call ----
 *
 * For p = 0 .. npairs-1, on `stream`, with no allocation, upload or synchronisation in between: the search of
 * orbs_tri_rows_search_batch_device for pair p, then orbt_triangulate_batch_device for pair p with d_qindex = NULL (d_q2t IS vMatches12).  The
 * triangulation of pair p clears d_qvalid and sets d_claimed at what it accepted, so the search of pair p + 1 is not offered those features: the
 * order the reference's `mpCurrentKeyFrame->AddMapPoint` (src/LocalMapping.cc:360) gives its neighbour loop.
 *   pair: a HOST list of (query row, train row), all with ONE query row (mpCurrentKeyFrame) and with train rows distinct from each other and from
 *       the query row; d_pairs[npairs], d_F12[9*npairs] on the device; the four level tables are HOST pointers (sigma2_2 is what the search's
 *       epipolar test reads); rows as in orbs_tri_rows_search_batch_device.
 *   d_qvalid[cap]: "mpCurrentKeyFrame's feature holds no map point yet", shared by the pairs, updated in place; d_claimed[npairs*cap]: "the
 *       neighbour's feature holds a map point", pair p at + p*cap, updated in place.
 *   d_q2t, d_t2q (may be NULL), d_nmatches: the search's outputs, pair p at + p*cap; the other arrays are those of orbt_triangulate_batch_device with
 *       cap1 = qcap = cap (pair p at + p*cap resp. + p*ocap).
 * ORBX_ERR_ARG before anything touches the GPU for what the two functions refuse, for a pair list that breaks the rule above, npairs outside
 * [0, ORBT_MAX_PAIRS], a NULL d_qvalid, d_claimed or d_q2t. */
int orbt_new_points_rows_device(const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* d_pairs, const float* d_F12,
                                const float* factors1, const float* sigma2_1, const float* factors2, const float* sigma2_2, int nlevels,
                                const orbx_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nt, const uint32_t* d_fv_node,
                                const int32_t* d_fv_off, const uint32_t* d_fv_feat, const int32_t* d_nfv, int nrows, int cap, uint8_t* d_qvalid,
                                uint8_t* d_claimed, int32_t* d_q2t, int32_t* d_t2q, int32_t* d_nmatches, uint8_t* d_status, float* d_x3d, float* d_v,
                                int32_t* d_match12, int32_t* d_acc_idx, float* d_acc_x3d, int32_t* d_count, int32_t* d_overflow, int ocap,
                                void* stream);

/* The same, synchronous, over host arrays: one pinned copy up, the chain, one copy down.  The rows' arrays are host memory, or device memory read in
 * place when rows_on_device != 0 (nt and nfv are host arrays either way).  qvalid[cap] and claimed[npairs*cap] are updated in place; entries of
 * the outputs that the kernels leave alone come back as zeros.  overflow[p] = 1 where pair p accepted more than ocap matches (count[p] holds the
 * number). */
int orbt_new_points_rows(const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* pairs, const float* F12, const float* factors1,
                         const float* sigma2_1, const float* factors2, const float* sigma2_2, int nlevels, const orbx_keypoint* kps,
                         const uint8_t* desc, const int32_t* nt, const uint32_t* fv_node, const int32_t* fv_off, const uint32_t* fv_feat,
                         const int32_t* nfv, int nrows, int cap, int rows_on_device, uint8_t* qvalid, uint8_t* claimed, int32_t* q2t, int32_t* t2q,
                         int32_t* nmatches, uint8_t* status, float* x3d, float* v, int32_t* match12, int32_t* acc_idx, float* acc_x3d, int32_t* count,
                         int32_t* overflow, int ocap, void* stream);

#ifdef __cplusplus
}
#endif
#endif
