/* orbp.h — C ABI of the MI355X-native local map-point table (part of liborbx.so).
 *
 * The per-frame host walk in front of Tracking's local-map search: the map points' position, mean viewing direction,
 * scale-invariance distances and descriptor live in HBM, and one call per frame (or per batch of frames) does
 * "pose in -> visible points, their search windows and their matches out" with nothing but the pose uploaded.
 *
 * Reference interfaces replaced (paths relative to the reference ORB_SLAM tree):
 *   orbp_put / orbp_erase        <- the MapPoint getters the search reads (GetWorldPos, GetNormal,
 *                                   Get{Min,Max}DistanceInvariance, GetDescriptor)                include/MapPoint.h
 *   orbp_project_batch_device    <- bool Frame::isInFrustum(MapPoint*, float)                     src/Frame.cc:137-198
 *                                   and the windows of ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
 *                                   (RadiusByViewingCos, th, scale factor, levels)               src/ORBmatcher.cc:57-72, :127-133
 *   orbp_track[_batch_device]    <- the loop of Tracking::SearchReferencePointsInFrustum          src/Tracking.cc:699-726
 *                                   (projection + orbs_window_search_batch_device with ORBS_RULE_MAPPOINTS, TH_HIGH)
 *   orbp_project_source_batch_device, orbp_track_source[_batch_device]
 *                                <- int ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, float th)   src/ORBmatcher.cc:1507-1620
 *                                   (Tracking::TrackWithMotionModel, src/Tracking.cc:565; ORBP_MODE_LAST_FRAME)
 *                                   int ORBmatcher::SearchByProjection(Frame& Current, KeyFrame*, const set<MapPoint*>&, float th, int ORBdist)
 *                                   src/ORBmatcher.cc:1622-1746 (Tracking::Relocalisation, src/Tracking.cc:960, :974; ORBP_MODE_KEYFRAME)
 *                                   (projection + orbs_window_search_batch_device with ORBS_RULE_BEST and the rotation check)
 *   orbp_refresh[_batch_device]  <- void MapPoint::UpdateNormalAndDepth()                         src/MapPoint.cc:273-312
 *                                   void MapPoint::ComputeDistinctiveDescriptors()               src/MapPoint.cc:185-250
 *                                   (the producer of what orbp_put takes from the caller; stated with the entry points below)
 *   orbp_fuse[_batch_device]     <- the search of int ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th)   src/ORBmatcher.cc:1016-1134
 *                                   for every call LocalMapping::SearchInNeighbors makes (src/LocalMapping.cc:373-450; ORBP_MODE_FUSE);
 *                                   Replace / AddObservation / AddMapPoint stay with the caller
 *                                   and, through views made by orbp_view_from_sim3, the search of
 *                                   int ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, float th)   src/ORBmatcher.cc:1136-1265
 *                                   for every call of LoopClosing::SearchAndFuse (src/LoopClosing.cc:557-570)
 *   orbp_view_from_sim3          <- the decomposition of Scw                                      src/ORBmatcher.cc:298-302 (= :1145-1149)
 *   orbp_loop_project_batch_device, orbp_loop_search[_batch_device]
 *                                <- int ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>& vpMatched, int th)
 *                                   src/ORBmatcher.cc:286-407 (LoopClosing::ComputeSim3, src/LoopClosing.cc:370; ORBP_MODE_LOOP)
 *                                   (projection + orbs_window_search_batch_device with ORBS_RULE_BEST, TH_LOW, no rotation check)
 *   orbp_sim3_from_pair, orbp_sim3_search[_batch_device]
 *                                <- int ORBmatcher::SearchBySim3(KeyFrame*, KeyFrame*, vector<MapPoint*>&, const float& s12, const cv::Mat& R12, const cv::Mat& t12, float th)
 *                                   src/ORBmatcher.cc:1267-1505, for every candidate whose RANSAC converged in LoopClosing::ComputeSim3
 *                                   (src/LoopClosing.cc: `matcher.SearchBySim3(mpCurrentKF, pKF, vpMapPointMatches, s, R, t, 7.5)`; ORBP_MODE_SIM3):
 *                                   both directions of every pair in one launch, the agreement (:1486-1502) in a second
 *   orbp_local_votes[_batch_device]
 *                                <- the counting of void Tracking::UpdateReferenceKeyFrames()      src/Tracking.cc:768-783
 *                                   and of void KeyFrame::UpdateConnections()                     src/KeyFrame.cc:334-363
 *   orbp_local_points[_batch_device]
 *                                <- void Tracking::UpdateReferencePoints()                         src/Tracking.cc:738-761
 *                                   and the stamps of Tracking::SearchReferencePointsInFrustum's first loop   src/Tracking.cc:678-694
 *   orbp_rows_purge_device       <- what MapPoint::SetBadFlag / KeyFrame::EraseMapPointMatch do to mvpMapPoints, for the resident columns
 *   orbp_cull[_batch_device]     <- the decisions of void LocalMapping::KeyFrameCulling()          src/LocalMapping.cc:524-578
 *                                   with the observations KeyFrame::SetBadFlag erases in between  src/KeyFrame.cc:497-515, src/MapPoint.cc:71-122
 *
 * Map points are named by caller-chosen slots 0 <= slot < capacity.
 *
 * Arithmetic of the frustum test: the float / double mix of src/Frame.cc:137-198, bit for bit, with the cv::Mat
 * primitives evaluated as DESIGN.md §2 lists them:
 *   Pc[r] = (((0.0f + R[r][0]*P[0]) + R[r][1]*P[1]) + R[r][2]*P[2]) + t[r] in float (so a zero PcZ is +0);
 *   PcZ < 0 rejects; invz = (float)(1.0 / (double)PcZ); u = fx*PcX*invz + cx, v likewise, float, left to right;
 *   u < (float)mnMinX || u > (float)mnMaxX rejects, same for v (the bounds are inclusive);
 *   PO = P - Ow in float; dist = (float)sqrt(sum of (double)PO[i]*(double)PO[i]); dist < minDistance || dist > maxDistance rejects;
 *   viewCos = (float)(sum of (double)PO[i]*(double)Pn[i] / (double)dist); viewCos < view_cos_limit rejects;
 *   level = lower_bound(factors, dist / minDistance) (float division), clipped to nlevels - 1.
 * The window of a visible point: r = viewCos > 0.998 (as double) ? 2.5f : 4.0f; r *= th unless th == 1; radius
 * r * factors[level]; levels [level - 1, level].
 *
 *
 * Arithmetic of the two source-frame modes (src/ORBmatcher.cc:1529-1542 and :1647-1660 are the same text), every step a single IEEE
 * operation:
 *   Pc as above; there is NO depth test (the reference has none here: a point behind the camera that lands inside the bounds is
 *   searched); invz = (float)(1.0 / (double)PcZ); u = fx*PcX*invz + cx, v likewise, float, left to right;
 *   u < (float)mnMinX || u > (float)mnMaxX rejects, same for v (inclusive bounds).
 *   ORBP_MODE_LAST_FRAME (:1544-1554): level = the source key point's octave; an octave outside [0, nlevels) is passed over (the
 *   reference would index mvScaleFactors out of bounds); the query's descriptor is the SOURCE FRAME's row.
 *   ORBP_MODE_KEYFRAME (:1662-1679): PO = P - Ow in float; dist3D = (float)sqrt(sum of (double)PO[i]*(double)PO[i]);
 *   ratio = dist3D / minDistance (float); level = min(lower_bound(factors, ratio), nlevels - 1); the query's descriptor is the TABLE's
 *   (pMP->GetDescriptor()).
 *   Both: radius th * factors[level] (float), levels [level - 1, level + 1], angle = the source key point's angle.
 *
 * Arithmetic of ORBP_MODE_FUSE (src/ORBmatcher.cc:1040-1113), per list entry, the first rejection that applies names its status:
 *   the entry is skipped, or its slot out of range or free -> ORBP_FUSE_SKIPPED;
 *   Pc as above; PcZ < 0.0f -> ORBP_FUSE_DEPTH;
 *   invz = 1.0f / PcZ (which rounds as the reference's (float)(1.0 / (double)PcZ) does); x = PcX*invz; y = PcY*invz; u = fx*x + cx;
 *   v = fy*y + cy, floats, left to right: NOT the association of the modes above;
 *   KeyFrame::IsInImage: u >= (float)min_x && u < (float)max_x && v >= (float)min_y && v < (float)max_y, else ORBP_FUSE_IMAGE.  The upper
 *   bounds are EXCLUSIVE here.  A NaN or infinite u or v fails this test in the reference too: this mode has no deviation;
 *   PO = P - Ow in float; dist = (float)sqrt(sum of (double)PO[i]*(double)PO[i]); dist < minDistance || dist > maxDistance -> ORBP_FUSE_DISTANCE;
 *   dot = sum of (double)PO[i]*(double)Pn[i]; dot < 0.5 * (double)dist, compared as doubles -> ORBP_FUSE_ANGLE (view_cos_limit is not read);
 *   level = min(lower_bound(factors, dist / minDistance), nlevels - 1) (float division); radius = th * factors[level] (float);
 *   the window of Frame::GetFeaturesInArea(u, v, radius, level - 1, level) over the key frame's grid: cells ix outer, iy inner, cell
 *   ix*48 + iy, the cell's features in CSR order; a feature is kept when |kx - u| <= radius && |ky - v| <= radius and
 *   level - 1 <= octave <= level; a strictly smaller Hamming distance wins, so among equal distances the FIRST feature in that order wins (not
 *   the lowest index); no cell window or no feature kept -> ORBP_FUSE_EMPTY;
 *   best distance <= orb_dist -> ORBP_FUSE_FUSED with that feature, else ORBP_FUSE_FAR and no feature.
 * Nothing is claimed and there is no ratio, second distance or rotation check: every entry is on its own.
 * The Scw overload of Fuse (src/ORBmatcher.cc:1160-1245) is this text word for word over the view of orbp_view_from_sim3 (its `1.0/z`, a float
 * division too, rounds as 1.0f / PcZ does), so LoopClosing::SearchAndFuse is orbp_fuse as it stands: one ORBP_MODE_FUSE view per corrected key
 * frame, every list the loop map points, all views in one launch.
 *
 * Arithmetic of orbp_view_from_sim3 (src/ORBmatcher.cc:298-302 = :1145-1149), Scw = [sR | st] being rows 0..2 of the 4 x 4 matrix:
 *   scw = (float)sqrt(sum of (double)sR[0][k]*(double)sR[0][k]), a double sum from 0.0 in index order (`sRcw.row(0).dot(sRcw.row(0))`);
 *   Rcw[i] = (float)((double)sR[i] / (double)scw), tcw[i] = (float)((double)st[i] / (double)scw) (`Mat / double`);
 *   Ow[c] = ((0.0f + (-Rcw[0][c])*tcw[0]) + (-Rcw[1][c])*tcw[1]) + (-Rcw[2][c])*tcw[2] in float (`-Rcw.t()*tcw`: the product of the negated transpose).
 *
 * Arithmetic of ORBP_MODE_LOOP (src/ORBmatcher.cc:311-363), per list entry: the steps of ORBP_MODE_FUSE above, word for word, up to and including
 * radius = th * factors[level], with the same statuses for the five rejections (the reference's `int th` enters as the float view.th).  An entry
 * that passes them all has the status ORBP_LOOP_QUERY and becomes a query: window (u, v, radius), levels [level - 1, level], the table's
 * descriptor, no angle.  The queries of a view are searched IN LIST ORDER by orbs_window_search_batch_device with ORBS_RULE_BEST, th = orb_dist
 * (TH_LOW in the reference, accepted when <=), no rotation check and d_claimed = `vpMatched[idx] != NULL` on entry: a match takes its feature,
 * and later entries pass that feature over (:378, :398-402).
 *
 * Arithmetic of orbp_sim3_from_pair (src/ORBmatcher.cc:1284-1286), the cv::Mat primitives as DESIGN.md §2 lists them:
 *   sR12[i] = (float)((double)R12[i] * (double)s12) (`float * Mat`: the scalar is a double inside the expression);
 *   inv = 1.0 / (double)s12, a DOUBLE; sR21[r][c] = (float)((double)R12[c][r] * inv) (`double * Mat::t()`);
 *   t21[r] = ((0.0f + (-sR21[r][0])*t12[0]) + (-sR21[r][1])*t12[1]) + (-sR21[r][2])*t12[2] in float (`-sR21*t12`: the product of the negated matrix).
 *
 * Arithmetic of ORBP_MODE_SIM3 (src/ORBmatcher.cc:1319-1399 for direction 1 -> 2, :1402-1484 for 2 -> 1: the same text with the key frames swapped),
 * one direction a -> b: the points of key frame a are searched in key frame b.  List entry i is feature i of key frame a; the first rejection that
 * applies names its status:
 *   the entry is skipped, or its slot out of range or free -> ORBP_FUSE_SKIPPED;
 *   Pa = Raw*P + taw, exactly Pc above (the `0.0f +` included);
 *   Pb[r] = (((0.0f + S[r][0]*Pa[0]) + S[r][1]*Pa[1]) + S[r][2]*Pa[2]) + t[r] in float; S, t = sR21, t21 for 1 -> 2 and sR12, t12 for 2 -> 1;
 *   Pb[2] < 0.0f -> ORBP_FUSE_DEPTH;
 *   invz = 1.0f / Pb[2] (rounds as the reference's `float invz = 1.0/z` does); x = Pb[0]*invz; y = Pb[1]*invz; u = fx*x + cx; v = fy*y + cy;
 *   KeyFrame::IsInImage as in ORBP_MODE_FUSE: half-open, a NaN or infinite u or v fails it -> ORBP_FUSE_IMAGE.  No deviation;
 *   dist3D = (float)sqrt(sum of (double)Pb[k]*(double)Pb[k]), a double sum from 0.0 in index order (`cv::norm(p3Dc2)`: the norm in camera b's
 *   frame, NOT the distance to a camera centre); dist3D < minDistance || dist3D > maxDistance -> ORBP_FUSE_DISTANCE;
 *   there is NO viewing-angle test: the slot's normal is not read and ORBP_FUSE_ANGLE never occurs;
 *   level = min(lower_bound(factors, dist3D / minDistance), nlevels - 1); radius = th * factors[level];
 *   the window, the octave rule [level - 1, level], the candidate order and "a strictly smaller distance wins" are ORBP_MODE_FUSE's, the same
 *   statement on the device; no cell window or no feature kept -> ORBP_FUSE_EMPTY;
 *   best distance <= orb_dist (TH_HIGH in the reference) -> ORBP_FUSE_FUSED with that feature, which is vnMatch of the entry; else ORBP_FUSE_FAR and -1.
 * Nothing is claimed: every entry is on its own.  The factors are those of the one extractor, as everywhere in this header.
 * The agreement (:1486-1502): match12[i1] = idx2 iff vnMatch1[i1] = idx2 >= 0, idx2 lies inside direction 2 -> 1's list and vnMatch2[idx2] == i1;
 * otherwise -1.  nfound counts the entries that are not -1.  An entry that was matched on entry (vbAlreadyMatched1 / 2) is marked skipped by the
 * host, so it never agrees.
 *
 * ONE DELIBERATE DEVIATION.  Where the reference leaves u or v NaN (PcZ == 0 together with PcX == 0 or PcY == 0: a point at
 * the camera centre) all its comparisons fail, the point passes with a NaN window and GetFeaturesInArea converts NaN to
 * int, which is undefined.  Here a point whose u or v is NaN is not visible, and is not a query in the source-frame modes.
 * The reference built with -march=native lets GCC fuse some of these expressions (fp_contract); this stage
 * implements the unfused evaluation only.
 *
 * Thread safety and streams as orbd.h: a handle is guarded by one mutex, device work on it is chained across the callers'
 * streams with an event, every entry point selects the map's device itself and restores the caller's.  Arguments are
 * checked on the host before anything touches the GPU.  Status codes are orbx.h's; there is no CPU fallback.
 */
#ifndef ORBP_H
#define ORBP_H

#include <stddef.h>
#include <stdint.h>

#include "orbf.h"
#include "orbs.h"
#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBP_MAX_CAPACITY (1 << 24)   /* slots of one table */
#define ORBP_MAX_VIEWS    (1 << 16)   /* problems of one call */

#define ORBP_MODE_FRAME 0             /* Frame::isInFrustum */
#define ORBP_MODE_LAST_FRAME 1        /* orbp_*_source*: the list is the last frame's features (motion-model tracking) */
#define ORBP_MODE_KEYFRAME 2          /* orbp_*_source*: the list is a key frame's features (relocalisation) */
#define ORBP_MODE_FUSE 3              /* orbp_fuse*: map points into key frames (LocalMapping's Fuse, and the Scw overload of LoopClosing's through
                                         orbp_view_from_sim3).  To orbp_project* / orbp_track* it is an unknown mode */
#define ORBP_MODE_LOOP 4              /* orbp_loop_*: the loop map points into one key frame through a similarity (LoopClosing's SearchByProjection).  To
                                         every other entry point it is an unknown mode */
#define ORBP_MODE_SIM3 5              /* orbp_sim3_*: the map points of one key frame into another through a similarity and back (LoopClosing's SearchBySim3);
                                         the mode of an orbp_sim3_dir.  To every other entry point it is an unknown mode */

typedef struct orbp_map orbp_map;

/* One search problem: a frame pose, its camera and the two parameters of Tracking's call. */
typedef struct orbp_view {
    float Rcw[9];                            /* mRcw, row major */
    float tcw[3];                            /* mtcw */
    float Ow[3];                             /* mOw (Frame::UpdatePoseMatrices) */
    float fx, fy, cx, cy;
    int32_t min_x, max_x, min_y, max_y;      /* Frame::mnMinX, mnMaxX, mnMinY, mnMaxY */
    float view_cos_limit;                    /* 0.5 in Tracking */
    float th;                                /* SearchByProjection's th: 1 or 5 in Tracking */
    int32_t mode;                            /* ORBP_MODE_*; view_cos_limit is not read by the source-frame modes */
    int32_t reserved;                        /* 0 */
} orbp_view;

/* What isInFrustum writes into a MapPoint: mbTrackInView, mTrackProjX, mTrackProjY, mTrackViewCos, mnTrackScaleLevel.
 * All zero for an entry that is skipped, not live or not visible. */
typedef struct orbp_record {
    uint8_t in_view;
    uint8_t pad[3];
    float u, v, view_cos;
    int32_t level;
} orbp_record;

/* ORBX_ERR_ARG for capacity outside [1, ORBP_MAX_CAPACITY] or a NULL `out`; ORBX_ERR_DEVICE without a usable GPU.
 * Device memory: 65 bytes per slot; the scratch of orbp_track* and orbp_loop_* and the block of orbp_refresh, orbp_fuse and orbp_sim3_search are allocated on first use and kept. */
int orbp_create(int capacity, int device, orbp_map** out);
void orbp_destroy(orbp_map* map);
int orbp_capacity(const orbp_map* map);
/* live slots */
int orbp_size(const orbp_map* map);
int orbp_clear(orbp_map* map);

/* Stores n map points from host arrays (pos, normal: 3 floats each; desc: 32 bytes each), synchronous.  A put on a live slot
 * replaces it.  desc == NULL keeps the stored descriptors (the refresh after bundle adjustment: 32 bytes per point); every
 * slot must then be live.  Staged through a pinned block of the handle: no allocation in the steady state, but one synchronous round
 * trip per call, so put many points per call.  ORBX_ERR_ARG for n < 0, a NULL array, a slot out of range or listed twice; the table is then unchanged. */
int orbp_put(orbp_map* map, const int32_t* slots, int n, const float* pos, const float* normal, const float* min_dist,
             const float* max_dist, const uint8_t* desc);
/* The same with the data in device arrays, asynchronous on `stream` (they are read when the stream reaches the call).
 * `slots` stays a host array: it is checked, and the live flags are kept, on the host. */
int orbp_put_device(orbp_map* map, const int32_t* slots, int n, const float* d_pos, const float* d_normal, const float* d_min_dist,
                    const float* d_max_dist, const uint8_t* d_desc, void* stream);
/* Frees n slots (host array); a slot that is not live is a no-op.  ORBX_ERR_ARG for a slot out of range. */
int orbp_erase(orbp_map* map, const int32_t* slots, int n);
/* Reads one slot back (synchronous; for tests).  *live = 0 and nothing else written for a free slot (the device's flag decides: see
 * orbp_refresh_batch_device).  pos[3], normal[3], desc[32]. */
int orbp_get(orbp_map* map, int slot, int* live, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc);

/* The frustum test and the search windows for nviews problems.  All arrays are device buffers except `factors`
 * (HOST pointer to mvScaleFactors, 1 <= nlevels <= ORBS_MAX_LEVELS, one table per call).
 *   d_views[nviews]; problem p walks the slots d_list[p*lcap + i], i < d_nlist[p] (clamped to [0, lcap]), in list order.
 *   d_list == NULL: every problem walks the identity list 0 .. capacity-1 (d_nlist is not read, lcap must be >= capacity), that
 *       is all live slots in ascending slot order, list position = slot.
 *   d_skip (may be NULL): entry i of problem p is passed over when d_skip[p*lcap + i] != 0 (mnLastFrameSeen == mnId || isBad()).
 *       An entry whose slot is out of range or not live is passed over too.
 *   d_rec (may be NULL): the record of every list entry at p*lcap + i.
 *   d_qxyr[3*qcap], d_qlev[2*qcap], d_qdesc[32*qcap] per problem: the visible entries, compacted in list order, in the layout
 *       orbs_window_search_batch_device reads (d_qdesc 16-byte aligned); d_qpos[qcap] the list position of each.
 *   A view whose `mode` is not ORBP_MODE_FRAME sees nothing: d_nq[p] = 0, d_overflow[p] = ORBX_ERR_ARG, its records are not written.
 *   d_nq[p]: the number of visible entries, always the true count.  When it exceeds qcap only the first qcap queries are written
 *       and d_overflow[p] = 1 (else 0): clamp d_nq before it is used as a query count.
 * Asynchronous on `stream`; allocates nothing. */
int orbp_project_batch_device(orbp_map* map, const orbp_view* d_views, int nviews, const float* factors, int nlevels,
                              const int32_t* d_list, const int32_t* d_nlist, int lcap, const uint8_t* d_skip, orbp_record* d_rec,
                              float* d_qxyr, int32_t* d_qlev, uint8_t* d_qdesc, int32_t* d_qpos, int32_t* d_nq, int32_t* d_overflow, int qcap,
                              void* stream);

/* Projection, then on the same stream the window search with ORBS_RULE_MAPPOINTS, TH_HIGH and `ratio` (mfNNratio) against the
 * frames that orbf_undistort_grid_batch_device left on the device: problem p searches frame p (d_kps_un / d_desc / d_claimed
 * + p*cap, d_cell_off + p*(ORBF_GRID_CELLS+1), d_cell_feat + p*cap, d_nt[p] features; d_claimed, may be NULL, marks features that
 * already hold a map point).  Outputs: d_t2slot[p*cap + idx] = the map slot matched to feature idx (-1 none), d_nmatches[p] the
 * return value of SearchByProjection, d_rec (may be NULL) as above, d_nq / d_overflow as above (a problem with d_overflow[p] set
 * was searched with its first qcap queries only).  qcap <= ORBF_MAX_FEATURES bounds the visible points of one problem.
 * The intermediate query arrays belong to the map handle; they grow on the first call of a size (synchronously) and are kept.
 * ORBX_ERR_CAPACITY when the search does not fit the LDS (orbs_lds_bytes(cap, qcap)). */
int orbp_track_batch_device(orbp_map* map, const orbp_view* d_views, int nviews, const float* factors, int nlevels,
                            const int32_t* d_list, const int32_t* d_nlist, int lcap, const uint8_t* d_skip,
                            const orbf_bounds* b, float ratio, const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int32_t* d_cell_off,
                            const int32_t* d_cell_feat, const int32_t* d_nt, int cap, const uint8_t* d_claimed, int qcap,
                            orbp_record* d_rec, int32_t* d_t2slot, int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow, void* stream);

/* One view, synchronous: the latency form.  view, factors, list / skip (nlist entries; list == NULL: all live slots, nlist must
 * then be the capacity and rec / skip are indexed by slot), rec[nlist] (may be NULL), t2slot[nt], *nmatches and *nvisible (may be
 * NULL) are HOST memory.  The frame (kps_un[nt], desc[32*nt], cell_off[ORBF_GRID_CELLS+1], cell_feat[nt], claimed[nt] or NULL) is
 * host memory, or device memory when frame_on_device != 0.  ORBX_ERR_CAPACITY when more than qcap points are visible
 * (*nvisible then holds the count; nothing else is written).  stream NULL: the map's own stream. */
int orbp_track(orbp_map* map, const orbp_view* view, const float* factors, int nlevels, const int32_t* list, int nlist,
               const uint8_t* skip, const orbf_bounds* b, float ratio, const orbx_keypoint* kps_un, const uint8_t* desc,
               const int32_t* cell_off, const int32_t* cell_feat, const uint8_t* claimed, int nt, int frame_on_device, int qcap,
               orbp_record* rec, int32_t* t2slot, int* nmatches, int* nvisible, void* stream);

/* ---- The projection searches whose queries are the features of a SOURCE frame: the last frame (ORBP_MODE_LAST_FRAME) or a key
 * frame (ORBP_MODE_KEYFRAME); the mode is each view's `mode`.  The arithmetic is stated at the top of this file.
 *
 * List entry i of problem p is feature i of its source frame: d_list[p*lcap + i] is the map slot of that feature's map point (-1:
 * it has none), i < d_nlist[p] (clamped to [0, lcap]); d_list and d_nlist are required.  d_skip (may be NULL) carries mvbOutlier[i]
 * (last frame) resp. isBad() || sAlreadyFound.count(pMP) (key frame).  An entry whose slot is out of range or not live is passed
 * over too.  d_src_kps + p*lcap: the source frame's key points in feature order (octave and angle are read; mvKeys and mvKeysUn
 * agree in both).  d_src_desc + p*32*lcap: its descriptors (16-byte aligned); read by last-frame views only, may be NULL when
 * every view is a key-frame view.
 * Outputs per problem, compacted in list order, in the layout orbs_window_search_batch_device reads: d_qxyr[3*qcap], d_qlev[2*qcap],
 * d_qdesc[32*qcap] (16-byte aligned), d_qangle[qcap]; d_qpos[qcap] the list position (= source feature index) of each query.
 * d_nq[p] is always the true count; when it exceeds qcap only the first qcap queries are written and d_overflow[p] = 1 (else 0).
 * A view whose mode is ORBP_MODE_FRAME or unknown (or a last-frame view without d_src_desc) sees nothing: d_nq[p] = 0,
 * d_overflow[p] = ORBX_ERR_ARG.  Asynchronous on `stream`; allocates nothing. */
int orbp_project_source_batch_device(orbp_map* map, const orbp_view* d_views, int nviews, const float* factors, int nlevels,
                                     const int32_t* d_list, const int32_t* d_nlist, int lcap, const uint8_t* d_skip,
                                     const orbx_keypoint* d_src_kps, const uint8_t* d_src_desc, float* d_qxyr, int32_t* d_qlev,
                                     uint8_t* d_qdesc, float* d_qangle, int32_t* d_qpos, int32_t* d_nq, int32_t* d_overflow, int qcap,
                                     void* stream);

/* Projection, then on the same stream orbs_window_search_batch_device with ORBS_RULE_BEST, prm->th (TH_HIGH for the last frame,
 * ORBdist for a key frame), prm->check_orientation and the queries' angles against the current frames on the device (laid out as
 * for orbp_track_batch_device; d_claimed, may be NULL, marks current features that hold a map point), then the result by source
 * feature: d_t2pos[p*cap + idx] = the source feature matched to current feature idx (-1 none; CurrentFrame.mvpMapPoints[idx] =
 * Source.mvpMapPoints[that]), d_t2slot (may be NULL) its map slot, d_nmatches[p] the reference's return value (after the rotation
 * filter).  prm->rule must be ORBS_RULE_BEST; prm->ratio is not used.  Scratch and ORBX_ERR_CAPACITY as orbp_track_batch_device. */
int orbp_track_source_batch_device(orbp_map* map, const orbp_view* d_views, int nviews, const float* factors, int nlevels,
                                   const int32_t* d_list, const int32_t* d_nlist, int lcap, const uint8_t* d_skip,
                                   const orbx_keypoint* d_src_kps, const uint8_t* d_src_desc, const orbf_bounds* b, const orbs_params* prm,
                                   const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat,
                                   const int32_t* d_nt, int cap, const uint8_t* d_claimed, int qcap, int32_t* d_t2pos, int32_t* d_t2slot,
                                   int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow, void* stream);

/* One view, synchronous: the latency form, one pinned block up and one down.  view, factors, list / skip (nlist entries), t2pos[nt],
 * t2slot[nt] (may be NULL), *nmatches and *nvisible (may be NULL) are HOST memory.  The source frame (src_kps[nlist], src_desc[32*nlist];
 * src_desc may be NULL for a key-frame view) is host memory, or device memory when src_on_device != 0; the current frame likewise
 * with frame_on_device (as orbp_track).  A caller who keeps both frames on the device uploads the view, the list and the skip flags
 * only.  ORBX_ERR_ARG for a view of ORBP_MODE_FRAME or an unknown mode; ORBX_ERR_CAPACITY when more than qcap entries project
 * inside the bounds (*nvisible then holds the count; nothing else is written).  stream NULL: the map's own stream.
 * With both frames in HOST memory the call uploads what the host-query route uploads and more (two whole frames instead of the
 * queries): it is there for callers such as ORB_SLAM::LocalMapPoints, not as the fast path, and has not been measured against that
 * route (NOTES.md §14); the form this interface is built for keeps both frames on the device. */
int orbp_track_source(orbp_map* map, const orbp_view* view, const float* factors, int nlevels, const int32_t* list, int nlist,
                      const uint8_t* skip, const orbx_keypoint* src_kps, const uint8_t* src_desc, int src_on_device, const orbf_bounds* b,
                      const orbs_params* prm, const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off,
                      const int32_t* cell_feat, const uint8_t* claimed, int nt, int frame_on_device, int qcap, int32_t* t2pos,
                      int32_t* t2slot, int* nmatches, int* nvisible, void* stream);

/* ---- The refresh of map points from their observations: MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:273-312) and
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:185-250) for n slots in one launch, written into the table in place.
 * The key frames are read where orbs_* and orbt_* read them: nkf frames of `cap` features each, key frame k's undistorted key points
 * at d_kf_kps + k*cap and its descriptors at d_kf_desc + k*32*cap (16-byte aligned).
 *
 * Point i (slot slots[i], position P = d_pos + 3*i, or the stored one when d_pos is NULL) has the observations
 * d_obs[2*j], d_obs[2*j + 1] = {kf, idx} for d_obs_off[i] <= j < d_obs_off[i + 1], in the order the reference iterates its
 * std::map<KeyFrame*, size_t>, which is pointer order: the float sum below depends on it, and the caller supplies it.  d_ref[i] is
 * the position INSIDE that segment of the observation by mpRefKF.
 *
 * Arithmetic, every step a single IEEE operation in the reference's order, no contraction, the cv::Mat primitives as DESIGN.md §2:
 *   ORBP_REFRESH_NORMAL_DEPTH.  For every observation in listed order, bad key frames INCLUDED (the reference does not skip them here):
 *     d = P - Ow_kf in float; s = sqrt(sum of (double)d[i]*(double)d[i]), a double sum from 0.0 in index order;
 *     unit[i] = (float)((double)d[i] / s); normal[i] = normal[i] + unit[i] in float, from 0.0f.
 *   mNormalVector[i] = (float)((double)normal[i] / (double)N), N the number of observations.
 *   PC = P - Ow_ref in float; dist = (float)sqrt(double sum of squares); level = the octave of key point idx of the reference key frame;
 *   scaleFactor = factors[1] (KeyFrame::GetScaleFactor() defaults to level 1: nlevels >= 2 is required);
 *   mfMinDistance = ((1.0f / scaleFactor) * dist) / factors[level]; mfMaxDistance = (scaleFactor * dist) * factors[nlevels - 1 - level],
 *   floats, left to right.
 *   ORBP_REFRESH_DESCRIPTOR.  The observations whose key frame is not bad (d_kf_bad), in listed order; none: the stored descriptor is
 *   kept (a slot that was free gets 32 zero bytes: the reference's mDescriptor is empty there).  Otherwise the row with the least
 *   vDists[(int)(0.5*(N' - 1))] of the N' x N' Hamming distances, the self distance included, the first such row on ties (what
 *   orbm_distinctive defines); the slot's 32 bytes become that key frame's row.
 *
 * Cases that cannot be evaluated are passed over, never dereferenced, and named in orbp_refreshed.status; the first that applies:
 *   ORBP_REFRESH_SKIPPED     d_skip[i] != 0 (mbBad: both functions return at once)
 *   ORBP_REFRESH_EMPTY       no observations (the reference divides by n == 0 and reads through a null mpRefKF entry)
 *   ORBP_REFRESH_BAD_INDEX   a kf outside [0, nkf), an idx outside [0, cap), or (with ORBP_REFRESH_NORMAL_DEPTH) d_ref[i] outside the segment
 *   ORBP_REFRESH_BAD_OCTAVE  the reference observation's octave is outside [0, nlevels)     (ORBP_REFRESH_NORMAL_DEPTH only)
 *   ORBP_REFRESH_NONFINITE   the normal or a distance is not finite: a point on a camera centre (ORBP_REFRESH_NORMAL_DEPTH only)
 * In every one of them the slot is unchanged, position and descriptor included, and a slot that was free stays free.
 * ORBP_REFRESH_NONFINITE is a DELIBERATE DEVIATION in the spirit of the NaN rule above: the reference stores the NaN, after which
 * isInFrustum's comparisons all fail for that point; here the record still carries the computed values and the table keeps the old.
 *
 * The record: normal / min_dist / max_dist as computed (zero without ORBP_REFRESH_NORMAL_DEPTH or before they were computed),
 * best_obs the position inside the segment (bad key frames counted) of the chosen observation and best_median its median (-1 and
 * INT32_MAX where no descriptor was chosen). */
#define ORBP_REFRESH_NORMAL_DEPTH 1
#define ORBP_REFRESH_DESCRIPTOR   2

#define ORBP_REFRESH_OK          0
#define ORBP_REFRESH_SKIPPED     1
#define ORBP_REFRESH_EMPTY       2
#define ORBP_REFRESH_BAD_INDEX   3
#define ORBP_REFRESH_BAD_OCTAVE  4
#define ORBP_REFRESH_NONFINITE   5

typedef struct orbp_refreshed {
    float normal[3];
    float min_dist, max_dist;
    int32_t best_obs;
    int32_t best_median;
    int32_t status;                          /* ORBP_REFRESH_* */
} orbp_refreshed;

/* All d_* are device arrays, read when the stream reaches the call; `slots` (n entries) and `factors` (nlevels) are HOST arrays.
 *   d_pos (3n floats, may be NULL = keep the stored position); with d_pos a slot that is not live becomes live (the new map point),
 *       which needs both `what` bits; without d_pos every slot must be live.
 *   d_obs_off[n + 1] (ascending), d_obs (int32 pairs, 8-byte aligned), d_ref[n] (read with ORBP_REFRESH_NORMAL_DEPTH only, may be NULL otherwise),
 *   d_skip[n] (may be NULL), d_kf_ow[3*nkf] (the key frames' camera centres, read with ORBP_REFRESH_NORMAL_DEPTH), d_kf_bad[nkf] (may
 *   be NULL: none is bad), d_kf_kps (read with ORBP_REFRESH_NORMAL_DEPTH), d_kf_desc (read with ORBP_REFRESH_DESCRIPTOR; 16-byte aligned),
 *   d_out[n] (may be NULL).
 * ORBX_ERR_ARG, with the table unchanged, for n < 0, a slot out of range or listed twice, a free slot without d_pos or without both
 * bits, `what` zero or with an unknown bit, nlevels outside [2, ORBS_MAX_LEVELS], nkf < 1, cap < 1, nkf * cap >= 2^31, a NULL or
 * misaligned array that `what` reads.  Asynchronous on `stream` (NULL: the map's own), inside the handle's event chain; allocates
 * nothing once the slot table has its size.
 * The host's count of live slots (orbp_size, and what later calls accept as live) takes a new slot as live from this call on,
 * whatever its status turns out to be: the device's flag, which the searches and orbp_get read, stays 0 for a status other than
 * ORBP_REFRESH_OK.  Erase such a slot or refresh it again; orbp_refresh below knows the statuses and keeps the count exact. */
int orbp_refresh_batch_device(orbp_map* map, const int32_t* slots, int n, const float* d_pos, const int32_t* d_obs_off, const int32_t* d_obs,
                              const int32_t* d_ref, const uint8_t* d_skip, const float* d_kf_ow, const uint8_t* d_kf_bad,
                              const orbx_keypoint* d_kf_kps, const uint8_t* d_kf_desc, int nkf, int cap, const float* factors, int nlevels,
                              int what, orbp_refreshed* d_out, void* stream);

/* The same with HOST arrays in and out, synchronous: the latency / test form, one pinned block up and one down.  pos, obs_off, obs,
 * ref, skip, kf_ow, kf_bad and out[n] (may be NULL) are host memory; the key frames' features (kf_kps, kf_desc) are host memory, or
 * device memory when kf_on_device != 0 (a caller who keeps its key frames resident uploads the lists and the camera centres only).
 * Checked here in addition: obs_off[0] >= 0 and obs_off ascending.  A new slot whose status is not ORBP_REFRESH_OK stays free on
 * the host's side too. */
int orbp_refresh(orbp_map* map, const int32_t* slots, int n, const float* pos, const int32_t* obs_off, const int32_t* obs, const int32_t* ref,
                 const uint8_t* skip, const float* kf_ow, const uint8_t* kf_bad, const orbx_keypoint* kf_kps, const uint8_t* kf_desc,
                 int kf_on_device, int nkf, int cap, const float* factors, int nlevels, int what, orbp_refreshed* out, void* stream);

/* ---- Fuse: the search of ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th) (src/ORBmatcher.cc:1016-1134) for many key frames in
 * one launch; the arithmetic is stated at the top of this file (ORBP_MODE_FUSE).  View p is a key frame's pose and camera (th = Fuse's th,
 * mode = ORBP_MODE_FUSE, view_cos_limit not read) and walks the slots d_list[p*lcap + i], i < d_nlist[p] (clamped to [0, lcap]); d_skip (may be
 * NULL) passes entry p*lcap + i over, as does a slot that is out of range or free.  It searches key frame d_frame[p] (d_frame == NULL: key
 * frame p) of the nframes key frames laid out as for orbp_track_batch_device: d_kps_un / d_desc / d_cell_feat + f*cap, d_cell_off +
 * f*(ORBF_GRID_CELLS+1), d_nt[f] features (clamped to [0, cap]); the grid precondition of orbs.h applies.  So one launch covers
 * SearchInNeighbors' forward loop (the views are the target key frames, every list the current key frame's points) and one more its reverse
 * call (one view, the candidates).  b: the key frames' image bounds and grid; orb_dist: ORBmatcher::TH_LOW in the reference.
 *
 * Outputs for every i < d_nlist[p], at p*lcap + i: d_best_idx the feature the point fuses into (-1 unless the status is ORBP_FUSE_FUSED),
 * d_best_dist the least distance of the window (INT32_MAX where nothing was scanned or kept), d_rec (may be NULL) the projection and the
 * status.  Entries at i >= d_nlist[p] are not written.  A view whose mode is not ORBP_MODE_FUSE or whose key frame is outside [0, nframes)
 * writes -1 / INT32_MAX / ORBP_FUSE_SKIPPED for its entries.  What Fuse does with a fused point (Replace, or AddObservation + AddMapPoint)
 * depends on the order of the points and on isBad() / IsInKeyFrame() as earlier points left them: that loop is the caller's, and the
 * result here does not depend on it.
 *
 * ORBX_ERR_ARG before anything touches the GPU for nviews outside [0, ORBP_MAX_VIEWS], lcap < 1, nviews * lcap >= 2^31, cap outside
 * [1, ORBF_MAX_FEATURES], nframes < 1, nframes * cap >= 2^31, nlevels outside [1, ORBS_MAX_LEVELS], orb_dist outside [0, 256], a NULL
 * required array, d_desc not 16-byte aligned, another array not 4-byte aligned.  Asynchronous on `stream` (NULL: the map's own), inside
 * the handle's event chain; allocates nothing. */
#define ORBP_FUSE_FUSED    0
#define ORBP_FUSE_SKIPPED  1
#define ORBP_FUSE_DEPTH    2
#define ORBP_FUSE_IMAGE    3
#define ORBP_FUSE_DISTANCE 4
#define ORBP_FUSE_ANGLE    5
#define ORBP_FUSE_EMPTY    6
#define ORBP_FUSE_FAR      7

typedef struct orbp_fused {
    float u, v;                              /* the projection; zero before it is computed (ORBP_FUSE_SKIPPED, ORBP_FUSE_DEPTH) */
    int32_t level;                           /* the predicted level; zero before it is computed (and for ORBP_FUSE_IMAGE, _DISTANCE, _ANGLE) */
    int32_t status;                          /* ORBP_FUSE_* */
} orbp_fused;

int orbp_fuse_batch_device(orbp_map* map, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                           const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const orbf_bounds* b, int orb_dist,
                           const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat,
                           const int32_t* d_nt, int nframes, int cap, const int32_t* d_frame, int32_t* d_best_idx, int32_t* d_best_dist,
                           orbp_fused* d_rec, void* stream);

/* The same with HOST arrays in and out, synchronous: the latency / test form, one pinned block up and one down.  views, list, nlist, skip, nt
 * (nframes entries), frame (nviews entries, may be NULL) and the outputs (nviews * lcap entries each; rec may be NULL) are host memory and
 * need no alignment; the key frames' arrays (kps_un, desc, cell_off, cell_feat: the whole batch layout is copied) are host memory, or
 * device memory when frames_on_device != 0 (a caller who keeps its key frames resident uploads the views and the lists only).  Checked
 * here in addition: ORBX_ERR_ARG for a view whose mode is not ORBP_MODE_FUSE or whose key frame is outside [0, nframes).  The block is
 * allocated on first use and kept. */
int orbp_fuse(orbp_map* map, const orbp_view* views, int nviews, const float* factors, int nlevels, const int32_t* list, const int32_t* nlist,
              int lcap, const uint8_t* skip, const orbf_bounds* b, int orb_dist, const orbx_keypoint* kps_un, const uint8_t* desc,
              const int32_t* cell_off, const int32_t* cell_feat, const int32_t* nt, int nframes, int cap, int frames_on_device,
              const int32_t* frame, int32_t* best_idx, int32_t* best_dist, orbp_fused* rec, void* stream);

/* ---- Loop closing.  orbp_view_from_sim3 fills Rcw, tcw and Ow of *view from rows 0..2 of the 4 x 4 float Scw (row major, [sR | st]) by the
 * arithmetic at the top of this file and leaves every other field alone.  ORBX_ERR_ARG for a NULL pointer or an scw that is zero or not
 * finite (the view is then untouched).  Host only: needs no GPU. */
int orbp_view_from_sim3(const float Scw[12], orbp_view* view);

/* The status of a list entry that passed every test of ORBP_MODE_LOOP, whether or not qcap left room for it as a query; the rejections are
 * ORBP_FUSE_SKIPPED, _DEPTH, _IMAGE, _DISTANCE and _ANGLE, and the record's u, v and level are filled as for those. */
#define ORBP_LOOP_QUERY 8

/* The projection of ORBP_MODE_LOOP for nviews views, flat over (view, 256-entry tile) in two launches: every entry is tested on its own, then
 * the entries that passed are compacted in list order behind the counts of the tiles in front of them.  All arrays are device buffers except
 * `factors`.  View p walks the slots d_list[p*lcap + i], i < d_nlist[p] (clamped to [0, lcap]); d_skip (may be NULL) passes an entry over
 * (isBad() || spAlreadyFound.count(pMP)), as does a slot that is out of range or free.
 *   d_rec (may be NULL): the record of every entry i < d_nlist[p] at p*lcap + i (entries behind the list are not written).
 *   d_qxyr[3*qcap], d_qlev[2*qcap], d_qdesc[32*qcap] (16-byte aligned), d_qpos[qcap] per view: the queries in list order, in the layout
 *       orbs_window_search_batch_device reads, and the list position of each.
 *   d_nq[p]: always the true count of entries that passed; when it exceeds qcap only the first qcap queries are written and d_overflow[p] = 1
 *       (else 0).  A view whose mode is not ORBP_MODE_LOOP sees nothing: d_nq[p] = 0, d_overflow[p] = ORBX_ERR_ARG, its records ORBP_FUSE_SKIPPED.
 * ORBX_ERR_ARG before anything touches the GPU for nviews outside [0, ORBP_MAX_VIEWS], lcap < 1, qcap < 1, nviews * lcap >= 2^31, nlevels
 * outside [1, ORBS_MAX_LEVELS], a NULL required array, d_qdesc not 16-byte aligned, another array not 4-byte aligned.  Asynchronous on
 * `stream` (NULL: the map's own) inside the handle's event chain.  The per-tile counts (and the records, without d_rec) live in the handle's
 * scratch, which grows on the first call of a size (synchronously, after a wait for the chain) and is kept. */
int orbp_loop_project_batch_device(orbp_map* map, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                                   const int32_t* d_nlist, int lcap, const uint8_t* d_skip, orbp_fused* d_rec, float* d_qxyr, int32_t* d_qlev,
                                   uint8_t* d_qdesc, int32_t* d_qpos, int32_t* d_nq, int32_t* d_overflow, int qcap, void* stream);

/* Projection, then on the same stream the window search (ORBS_RULE_BEST, th = orb_dist, no rotation check) and the result by feature.  View p
 * searches key frame d_frame[p] (d_frame == NULL: key frame p) of the nframes key frames in the batch layout of orbp_fuse_batch_device;
 * d_claimed (may be NULL) is per VIEW: d_claimed[p*cap + idx] != 0 when vpMatched[idx] is set on entry.  Outputs: d_t2pos[p*cap + idx] the list
 * position of the entry matched to feature idx in this call (-1 none, also for a feature claimed on entry or at or behind the key frame's
 * count; vpMatched[idx] = vpPoints[that]), d_t2slot (may be NULL) its map slot, d_nmatches[p] the reference's return value, d_nq / d_overflow
 * / d_rec (may be NULL) as above (a view with d_overflow[p] == 1 was searched with its first qcap queries only).  A view whose mode is not
 * ORBP_MODE_LOOP or whose key frame is outside [0, nframes) sees nothing: d_nq[p] = 0, d_overflow[p] = ORBX_ERR_ARG, no match.
 * With d_frame (or more views than key frames) the rows are gathered per view into the handle's scratch first: a caller with one view passes
 * the row's own addresses and nframes = 1 instead.
 * ORBX_ERR_ARG as above and for cap outside [1, ORBF_MAX_FEATURES], qcap > ORBF_MAX_FEATURES, nframes < 1, nframes * cap >= 2^31, orb_dist outside [0, 256], d_desc not 16-byte aligned; ORBX_ERR_CAPACITY when the search does not fit the LDS
 * (orbs_lds_bytes(cap, qcap)).  Scratch as above. */
int orbp_loop_search_batch_device(orbp_map* map, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                                  const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const orbf_bounds* b, int orb_dist,
                                  const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat,
                                  const int32_t* d_nt, int nframes, int cap, const int32_t* d_frame, const uint8_t* d_claimed, int qcap,
                                  orbp_fused* d_rec, int32_t* d_t2pos, int32_t* d_t2slot, int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow,
                                  void* stream);

/* One view, synchronous: the latency form, one pinned block up and one down.  view, factors, list / skip (nlist entries), rec[nlist] (may be
 * NULL), t2pos[nt], t2slot[nt] (may be NULL), *nmatches and *nvisible (may be NULL) are HOST memory.  The key frame (kps_un[nt], desc[32*nt],
 * cell_off[ORBF_GRID_CELLS+1], cell_feat[nt]) is host memory, or device memory when frame_on_device != 0 (a row of a resident store: desc
 * 16-byte aligned); claimed[nt] (may be NULL) is host memory either way: it is this call's vpMatched.  ORBX_ERR_ARG for a view whose mode is
 * not ORBP_MODE_LOOP; ORBX_ERR_CAPACITY when more than qcap entries pass (*nvisible then holds the count; nothing else is written).
 * stream NULL: the map's own stream. */
int orbp_loop_search(orbp_map* map, const orbp_view* view, const float* factors, int nlevels, const int32_t* list, int nlist, const uint8_t* skip,
                     const orbf_bounds* b, int orb_dist, const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off,
                     const int32_t* cell_feat, const uint8_t* claimed, int nt, int frame_on_device, int qcap, orbp_fused* rec, int32_t* t2pos,
                     int32_t* t2slot, int* nmatches, int* nvisible, void* stream);

/* ---- SearchBySim3 (src/ORBmatcher.cc:1267-1505): the arithmetic is stated at the top of this file (ORBP_MODE_SIM3).
 *
 * One direction a -> b of one pair: key frame a's pose, the similarity that takes camera a's frame into camera b's, key frame b's camera and image
 * bounds, SearchBySim3's th.  A multiple of 16 bytes; an orbp_view has no room for the second 3 x 4. */
typedef struct orbp_sim3_dir {
    float Raw[9];                            /* the SOURCE key frame's GetRotation(), row major */
    float taw[3];                            /* its GetTranslation() */
    float S[9];                              /* sR21 (direction 1 -> 2) or sR12 (2 -> 1), row major */
    float t[3];                              /* t21 or t12 */
    float fx, fy, cx, cy;
    int32_t min_x, max_x, min_y, max_y;      /* KeyFrame::mnMinX .. mnMaxY of the key frame searched in */
    float th;                                /* SearchBySim3's th: 7.5 in LoopClosing */
    int32_t mode;                            /* ORBP_MODE_SIM3 */
    int32_t reserved[2];                     /* 0 */
} orbp_sim3_dir;

/* Fills dirs[0] (direction 1 -> 2: R1w, t1w, sR21, t21) and dirs[1] (direction 2 -> 1: R2w, t2w, sR12, t12) from SearchBySim3's arguments by the
 * arithmetic at the top of this file; camera, bounds (those of b: min_x, max_x, min_y, max_y) and th go into both, mode = ORBP_MODE_SIM3.
 * ORBX_ERR_ARG for a NULL pointer or an s12 that is zero or not finite (dirs is then untouched).  Host only: needs no GPU. */
int orbp_sim3_from_pair(float s12, const float R12[9], const float t12[3], const float R1w[9], const float t1w[3], const float R2w[9],
                        const float t2w[3], float fx, float fy, float cx, float cy, const orbf_bounds* b, float th, orbp_sim3_dir dirs[2]);

/* npairs pairs of key frames, both directions of all of them in ONE launch of 2 * npairs rows, then the agreement on the same stream.  All arrays
 * are device buffers except `factors`.  Pair p owns rows 2p (direction 1 -> 2) and 2p + 1 (2 -> 1) of the per-row arrays d_dirs, d_nlist and
 * d_frame, and of the per-entry arrays (row r's entries at r*lcap + i).  Row r walks d_list[r*lcap + i], i < d_nlist[r] (clamped to [0, lcap]): list
 * entry i is FEATURE i of the row's source key frame, its map slot or -1 for "no map point"; d_skip (may be NULL) passes an entry over (isBad(), or
 * matched on entry), as does a slot that is out of range or free.  Row r searches key frame d_frame[r] (d_frame == NULL: key frame r) of the
 * nframes key frames in the batch layout of orbp_fuse_batch_device: row 2p searches key frame 2 of the pair, row 2p + 1 key frame 1.
 * b: the key frames' image bounds and grid; orb_dist: ORBmatcher::TH_HIGH in the reference.
 *
 * Outputs for every i < d_nlist[r], at r*lcap + i: d_best_idx (vnMatch1 in row 2p, vnMatch2 in row 2p + 1; -1 unless the status is ORBP_FUSE_FUSED),
 * d_best_dist, d_rec (may be NULL) as orbp_fuse_batch_device.  A row whose mode is not ORBP_MODE_SIM3 or whose key frame is outside [0, nframes)
 * writes -1 / INT32_MAX / ORBP_FUSE_SKIPPED for its entries, and its pair finds nothing.  d_match12[p*lcap + i1] for i1 < d_nlist[2p]: the feature
 * of key frame 2 whose map point vpMatches12[i1] becomes (-1 none); d_nfound[p]: the reference's return value, counted on the device.
 *
 * ORBX_ERR_ARG before anything touches the GPU for npairs outside [0, ORBP_MAX_VIEWS / 2], and otherwise as orbp_fuse_batch_device (with
 * nviews = 2 * npairs), d_match12 and d_nfound being required.  Asynchronous on `stream` (NULL: the map's own), inside the handle's event chain;
 * allocates nothing. */
int orbp_sim3_search_batch_device(orbp_map* map, const orbp_sim3_dir* d_dirs, int npairs, const float* factors, int nlevels, const int32_t* d_list,
                                  const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const int32_t* d_frame, const orbx_keypoint* d_kps_un,
                                  const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat, const int32_t* d_nt, int nframes, int cap,
                                  const orbf_bounds* b, int orb_dist, int32_t* d_best_idx, int32_t* d_best_dist, orbp_fused* d_rec, int32_t* d_match12,
                                  int32_t* d_nfound, void* stream);

/* The same with HOST arrays in and out, synchronous: the latency / test form, one pinned block up and one down.  dirs, list, nlist, skip, frame
 * (2 * npairs rows; frame may be NULL), nt and the outputs are host memory and need no alignment: best_idx, best_dist, rec (2 * npairs * lcap entries
 * each; each may be NULL), match12 (npairs * lcap) and nfound (npairs).  The key frames' arrays are host memory (the whole batch layout is copied),
 * or device memory when frames_on_device != 0 (a caller who keeps its key frames resident uploads the directions and the lists only).  Checked
 * here in addition: ORBX_ERR_ARG for a row whose mode is not ORBP_MODE_SIM3 or whose key frame is outside [0, nframes).  Entries behind a list
 * are not written.  The block is the handle's own, grown on first use and kept. */
int orbp_sim3_search(orbp_map* map, const orbp_sim3_dir* dirs, int npairs, const float* factors, int nlevels, const int32_t* list, const int32_t* nlist,
                     int lcap, const uint8_t* skip, const int32_t* frame, const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off,
                     const int32_t* cell_feat, const int32_t* nt, int nframes, int cap, int frames_on_device, const orbf_bounds* b, int orb_dist,
                     int32_t* best_idx, int32_t* best_dist, orbp_fused* rec, int32_t* match12, int32_t* nfound, void* stream);

/* ---- The local map: key-frame votes and the local point list, over a map-point COLUMN of the resident key-frame rows.
 *
 * Row k of the nkf resident key frames (the rows orbs_* and orbt_* read, `cap` features each) has the column d_kf_slot[k*cap + i]: the table
 * slot of pKF->mvpMapPoints[i], or -1; d_kf_nt[k] (clamped to [0, cap]) is the row's feature count.  Under the reference's map invariant
 * (pKF->mvpMapPoints[idx] == pMP exactly when pMP->mObservations[pKF] == idx, kept under its map mutex) the column is the transpose of the
 * observation maps, so "which key frames observe this point" is a scan over integer columns and no observation list goes up.
 * PRECONDITION, stated and not checked on the device: a slot occurs at most once per row.  An entry that is -1, out of range or not live in the
 * table is passed over, never dereferenced.
 *
 * orbp_local_votes*: the counting of Tracking::UpdateReferenceKeyFrames (src/Tracking.cc:768-783) and of KeyFrame::UpdateConnections
 * (src/KeyFrame.cc:334-363).  Query p is the list of slots d_query[p*qcap + j], j < d_nquery[p] (clamped to [0, qcap]); an entry may be -1, out
 * of range or repeated.  d_votes[p*nkf + k] = the sum, over the features i < d_kf_nt[k] of row k whose slot is live, of the MULTIPLICITY of that
 * slot in query p: the reference increments once per frame feature, so a frame that holds one point at two features votes twice.  Every word
 * of d_votes has one writer and is a plain store; the multiplicities are integer atomic adds, so nothing depends on arrival order.
 *
 * orbp_local_points*: the list of Tracking::UpdateReferencePoints (src/Tracking.cc:742-760) with the stamps of the first loop of
 * Tracking::SearchReferencePointsInFrustum (:678-694), in the layout orbp_track_batch_device reads.  Problem p walks the rows
 * d_rows[p*rcap + j], j < d_nrows[p] (clamped to [0, rcap]), in list order and each row's features in index order; a row outside [0, nkf) is passed
 * over, never dereferenced.  d_list[p*lcap ..] holds the slots met that are >= 0, in range and live, each at its FIRST occurrence only, in exactly
 * that order (so a row listed twice contributes nothing the second time).  d_nlist[p] is always the true count; beyond lcap only the first lcap
 * entries are written and d_overflow[p] = 1 (else 0): clamp d_nlist before it is used as a count (orbp_track_batch_device does).
 * d_skip[p*lcap + i] = 1 when the slot's multiplicity in query p is > 0 (the point the frame holds already: mnLastFrameSeen == mnId), else 0;
 * d_query == NULL: no query, every flag 0.  The call is self-contained: it takes the query list itself and leaves nothing behind.
 * The first occurrence is decided by an integer atomicMin of the walk position j*cap + i per slot, and the order is restored by counting (tile
 * counts, their sum in front of a tile, scatter), as orbp_loop_project_batch_device does: launch boundaries are the only ordering.
 *
 * orbp_rows_purge_device: sets every column entry (all nkf*cap of them) that names one of the n slots (HOST array, as orbp_erase takes them) to
 * -1, in one scan.  Run it before orbp_erase whenever slots die while a column is resident: a freed and re-assigned slot would otherwise alias
 * stale column entries.
 *
 * The handle owns the scratch: two words per (problem, slot) and one per (problem, listed row, 256-feature tile), grown on the first call of a
 * size (synchronously, after a wait for the chain) and kept.  The kernels put back every word they changed, so resetting the scratch needs
 * no host synchronisation and costs what the call itself touched, not the capacity.  nproblems <= ORBP_LOCAL_MAX_PROBLEMS, rcap <= ORBP_LOCAL_MAX_ROWS.
 *
 * ORBX_ERR_ARG before anything touches the GPU, with nothing changed, for a NULL handle, nproblems outside [0, ORBP_LOCAL_MAX_PROBLEMS], a negative
 * nkf or n, cap < 1, nkf * cap >= 2^31, qcap < 1 (lcap < 1, rcap outside [1, ORBP_LOCAL_MAX_ROWS], rcap * cap >= 2^31, nproblems * lcap >= 2^31), a
 * NULL required array, an array that is not 4-byte aligned (d_skip needs none), a purged slot out of range.  The batch-device forms are
 * asynchronous on `stream` (NULL: the map's own), inside the handle's event chain, and allocate nothing in the steady state. */
#define ORBP_LOCAL_MAX_PROBLEMS 64
#define ORBP_LOCAL_MAX_ROWS     65535

int orbp_local_votes_batch_device(orbp_map* map, const int32_t* d_query, const int32_t* d_nquery, int qcap, int nproblems, const int32_t* d_kf_slot,
                                  const int32_t* d_kf_nt, int nkf, int cap, int32_t* d_votes, void* stream);

/* The same with HOST arrays in and out, synchronous: one pinned block up and one down.  query, nquery and votes (nproblems * nkf) are host
 * memory; the columns (kf_slot, kf_nt) are host memory, or device memory when kf_on_device != 0 (the resident form: only the query goes up). */
int orbp_local_votes(orbp_map* map, const int32_t* query, const int32_t* nquery, int qcap, int nproblems, const int32_t* kf_slot, const int32_t* kf_nt,
                     int kf_on_device, int nkf, int cap, int32_t* votes, void* stream);

int orbp_local_points_batch_device(orbp_map* map, const int32_t* d_query, const int32_t* d_nquery, int qcap, int nproblems, const int32_t* d_rows,
                                   const int32_t* d_nrows, int rcap, const int32_t* d_kf_slot, const int32_t* d_kf_nt, int nkf, int cap, int32_t* d_list,
                                   int32_t* d_nlist, uint8_t* d_skip, int32_t* d_overflow, int lcap, void* stream);

/* The same with HOST arrays in and out, synchronous.  query (may be NULL), nquery, rows, nrows, list and skip (nproblems * lcap each; of problem p
 * the first min(nlist[p], lcap) entries are written), nlist and overflow (nproblems; overflow may be NULL) are host memory; the columns as above. */
int orbp_local_points(orbp_map* map, const int32_t* query, const int32_t* nquery, int qcap, int nproblems, const int32_t* rows, const int32_t* nrows,
                      int rcap, const int32_t* kf_slot, const int32_t* kf_nt, int kf_on_device, int nkf, int cap, int32_t* list, int32_t* nlist,
                      uint8_t* skip, int32_t* overflow, int lcap, void* stream);

int orbp_rows_purge_device(orbp_map* map, const int32_t* slots, int n, int32_t* d_kf_slot, int nkf, int cap, void* stream);

/* ---- Key-frame culling over the columns: the decisions of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:524-578), with what
 * KeyFrame::SetBadFlag (src/KeyFrame.cc:497-515: the guard and the EraseObservation loop) and MapPoint::EraseObservation / SetBadFlag
 * (src/MapPoint.cc:71-122) do to the observations in between, so that every candidate is judged on the map its predecessors left.
 *
 * Beside the slot column every row has an OCTAVE column, d_kf_oct[k*cap + i] = pKF->GetKeyPointUn(i).octave as a uint8.  A column entry TAKES
 * PART when i < clamp(d_kf_nt[k], 0, cap), its slot is in range and live in the table, and its octave is below nlevels; any other entry is passed
 * over in the build, in the count and in the erasure alike, never dereferenced.  DEVIATION: an octave outside [0, nlevels) cannot come from the
 * extractor; the reference would compare it like any other, here its entry does not exist.
 * PRECONDITIONS, stated and not checked: a slot occurs at most once per row; every non-bad key frame of the map is a resident row with its
 * column; bad key frames have no column.  Then H[s][l], the number of rows that hold slot s at a feature of octave l, is the transpose of
 * mObservations by level, and sum_l H[s][l] == pMP->Observations().
 *
 * Candidate c is judged in list order on row r = d_cand[c], with a flag dead[s] per slot (all clear at the start):
 *   nMPs  = the entries of row r that take part and whose slot is not dead;
 *   nRed  = those of them with T = sum_l H[s][l] > 3 and (sum_{l <= oct+1} H[s][l]) - 1 >= 3 (the row's own observation lies inside the sum; the
 *           reference stops counting at three, which changes nothing);
 *   cull  = (double)nRed > 0.9 * (double)nMPs, one IEEE multiply and one compare as :575 (nMPs == 0 gives 0).
 * When cull: every entry of row r that takes part, dead or not, loses its observation (H[s][oct] -= 1), a slot whose T is now <= 2 becomes dead,
 * and the row is erased for the rest of the call.  d_nmps[c], d_nred[c], d_cull[c] are as of the candidate's turn; a candidate whose row is
 * outside [0, nkf) or was erased earlier in the call writes 0, 0, 0 and reads nothing.  Exactly ncand words of each output are written.
 * The call leaves no trace: the table's live flags and the columns are not changed (the caller's SetBadFlag calls, orbp_erase and
 * orbp_rows_purge_device do that).  mbNotErase is the caller's business: a flagged key frame that does not go bad invalidates what follows it.
 *
 * The handle owns the scratch, grown on first use and kept: eight words per slot (sixteen 16-bit level counts; a count is at most the number
 * of rows, <= ORBP_LOCAL_MAX_ROWS, so a field cannot carry) and one dead word per slot.  The kernels put back every word they changed.
 *
 * ORBX_ERR_ARG before anything touches the GPU, with nothing changed, for a NULL handle, ncand outside [0, ORBP_CULL_MAX_CANDIDATES], nkf outside
 * [0, ORBP_LOCAL_MAX_ROWS], cap < 1, nkf * cap >= 2^31, nlevels outside [1, ORBS_MAX_LEVELS], a NULL required array, an int32 array that is not
 * 4-byte aligned (d_kf_oct needs no alignment).  ncand == 0 or nkf == 0 is ORBX_OK with nothing launched.  Asynchronous on `stream` (NULL: the
 * map's own), inside the handle's event chain; allocates nothing in the steady state. */
#define ORBP_CULL_MAX_CANDIDATES 4096

int orbp_cull_batch_device(orbp_map* map, const int32_t* d_cand, int ncand, const int32_t* d_kf_slot, const uint8_t* d_kf_oct,
                           const int32_t* d_kf_nt, int nkf, int cap, int nlevels, int32_t* d_nmps, int32_t* d_nred, int32_t* d_cull, void* stream);

/* The same with HOST arrays in and out, synchronous: one pinned block up and one down.  cand, nmps, nred and cull (ncand each) are host memory;
 * the columns (kf_slot, kf_oct, kf_nt) are host memory, or device memory when kf_on_device != 0 (only the candidate list goes up). */
int orbp_cull(orbp_map* map, const int32_t* cand, int ncand, const int32_t* kf_slot, const uint8_t* kf_oct, const int32_t* kf_nt,
              int kf_on_device, int nkf, int cap, int nlevels, int32_t* nmps, int32_t* nred, int32_t* cull, void* stream);

#ifdef __cplusplus
}
#endif
#endif
