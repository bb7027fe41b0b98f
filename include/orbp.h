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
 * ONE DELIBERATE DEVIATION.  Where the reference leaves u or v NaN (PcZ == 0 together with PcX == 0 or PcY == 0: a point at
 * the camera centre) all its comparisons fail, the point passes with a NaN window and GetFeaturesInArea converts NaN to
 * int, which is undefined.  Here a point whose u or v is NaN is not visible.
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

#define ORBP_MODE_FRAME 0             /* Frame::isInFrustum; the key-frame-side projections are a later mode */

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
    int32_t mode;                            /* ORBP_MODE_FRAME */
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
 * Device memory: 65 bytes per slot; the scratch of orbp_track* is allocated on first use and kept. */
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
/* Reads one slot back (synchronous; for tests).  *live = 0 and nothing else written for a free slot.  pos[3], normal[3], desc[32]. */
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

#ifdef __cplusplus
}
#endif
#endif
