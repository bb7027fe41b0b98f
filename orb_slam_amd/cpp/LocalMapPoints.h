// ORB_SLAM::LocalMapPoints — the local map's points mirrored on the MI355X (include/orbp.h), and the loop of
// Tracking::SearchReferencePointsInFrustum (reference src/Tracking.cc:699-726) as one call: Frame::isInFrustum on every listed map
// point, the write-back of the five mTrack* fields, IncreaseVisible(), and ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th)
// on the GPU.  Host C++ written against the reference's Frame / MapPoint member names; links the C ABI only.
//
// A map point is mirrored by Put (which reads GetWorldPos, GetNormal, Get{Min,Max}DistanceInvariance, GetDescriptor) and dropped by
// Forget.  Both only touch host memory; the device table is brought up to date in ONE orbp_put / orbp_erase at the start of the next
// search, so a bundle adjustment that moves thousands of points costs one upload.  The table grows by doubling.
// Refresh (LocalMapPointsRefresh.cc) replaces the pair MapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors + Put: the listed points'
// observation lists and their key frames' camera centres go up, the normal, the two distances and the descriptor are computed on the GPU
// from key frames whose features stay resident (orbp_refresh), and land in the table's slots directly.
// Fuse / FuseInNeighbors (LocalMapPointsFuse.cc) replace ORBmatcher::Fuse(pKF, vpMapPoints, th) as LocalMapping::SearchInNeighbors calls it: the
// search of every target key frame is one orbp_fuse over the same resident key frames, whose rows then carry their grid too; Replace /
// AddObservation / AddMapPoint stay the reference's in-order loop on the host.
// SearchByProjection(pKF, Scw, ...) / SearchAndFuse (LocalMapPointsLoop.cc) replace the two searches LoopClosing makes once a Sim3 is accepted:
// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) as one orbp_loop_search against pKF's resident row, and the loop of
// LoopClosing::SearchAndFuse as one orbp_fuse over every corrected key frame, followed by the reference's in-order loop on the host.  Both read
// the points' positions from the mirror: a caller who moved points (CorrectLoop does, before it fuses) must Put them first, or construct
// with refresh_every_call.
// SearchBySim3 (LocalMapPointsSim3.cc) replaces ORBmatcher::SearchBySim3 as LoopClosing::ComputeSim3 calls it for every candidate whose RANSAC
// converged: both key frames' points are searched in each other's resident row by ONE orbp_sim3_search, all candidates of a call together, and
// only two poses, the similarity and two slot lists per candidate go up.
// SearchByBoW (LocalMapPointsBoW.cc) replaces both ORBmatcher::SearchByBoW overloads as Tracking::Relocalisation and LoopClosing::ComputeSim3 call
// them per candidate: the rows of the key-frame store gain their FeatureVector, and every candidate of a call is one pair of ONE
// orbs_bow_rows_search.
// CreateNewMapPoints (LocalMapPointsNewPoints.cc) replaces ORBmatcher::SearchForTriangulation and the match loop behind it for every neighbour of
// LocalMapping::CreateNewMapPoints: one stream-ordered chain search -> triangulate per neighbour over the same rows, one call, one synchronisation.
// PutKeyFrame / UpdateReferenceKeyFrames / SearchLocalMap / ConnectionWeights (LocalMapPointsLocalMap.cc) replace the three host walks in front of
// Tracking's local-map search (UpdateReferenceKeyFrames, UpdateReferencePoints, the list building of SearchReferencePointsInFrustum) and the counting
// half of KeyFrame::UpdateConnections: every row of the key-frame store gains a map-point column, the votes are a scan over those columns, and the
// local point list is built on the device and handed to the search without visiting the host.
// Not thread safe: call it from the tracking thread, or guard it with the lock that guards the map.
// There is no CPU fallback: without a usable GPU the constructor throws std::runtime_error, as does a failing search.
#pragma once
#include <cstdint>
#include <map>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

#include "orbp.h"
#include "MapPoint.h"
#include "Frame.h"

namespace ORB_SLAM {

class MapPoint;
class Frame;
class KeyFrame;
struct NewMapPoint;             // NewMapPoints.h

class LocalMapPoints {
public:
    // nnratio: mfNNratio of the ORBmatcher Tracking uses for this search (0.8).  refresh_every_call: every listed point is Put again
    // on each search, for callers who do not hook the map; the default trusts the hooks.
    explicit LocalMapPoints(float nnratio = 0.8f, bool refresh_every_call = false, int capacity = 4096, int device = 0);
    ~LocalMapPoints();
    LocalMapPoints(const LocalMapPoints&) = delete;
    LocalMapPoints& operator=(const LocalMapPoints&) = delete;

    // mirrors pMP into its slot (the first call assigns one)
    void Put(MapPoint* pMP);
    // frees pMP's slot; unknown points are ignored
    void Forget(MapPoint* pMP);

    // src/Tracking.cc:699-726.  Points with mnLastFrameSeen == F.mnId or isBad() are passed over; every other listed point gets
    // mbTrackInView and, when visible, mTrackProjX/Y, mnTrackScaleLevel, mTrackViewCos and IncreaseVisible(); *nToMatch counts them.
    // F.mvpMapPoints[idx] receives the matched points; returns SearchByProjection's return value.  F.mTcw must hold the pose
    // (UpdatePoseMatrices need not have been called).  Listed points not yet mirrored are Put on the way.
    int SearchReferencePointsInFrustum(Frame& F, const std::vector<MapPoint*>& vpLocalMapPoints, float th, int* nToMatch = 0);

    // The two projection searches that run before it (LocalMapPointsSource.cc; both link only when that file is built in):
    // ORBmatcher::SearchByProjection(Frame&, const Frame&, float) of Tracking::TrackWithMotionModel (src/Tracking.cc:565) and
    // ORBmatcher::SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, float, int) of Tracking::Relocalisation (:960, :974).
    // CurrentFrame.mvpMapPoints[idx] is written exactly as the reference writes it; the return value is the reference's.
    // checkOrientation is the ORBmatcher's mbCheckOrientation.  Points not yet mirrored are Put on the way.
    int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, float th, bool checkOrientation = true);
    int SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound, float th, int ORBdist,
                           bool checkOrientation = true);

    // MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:273-312) and, with `descriptors`, MapPoint::ComputeDistinctiveDescriptors (:185-250) for
    // the listed points (LocalMapPointsRefresh.cc; links only when that file is built in).  Reads isBad(), GetWorldPos(), GetObservations() in
    // the map's order, GetReferenceKeyFrame(), and of the key frames GetCameraCenter(), isBad(), GetScaleFactors() and, once per key frame,
    // GetKeyPointsUn() and GetDescriptors().  The table's slots and this object's mirror are brought up to date; record i is what the two
    // functions would have left in vpMPs[i] (orbp.h: orbp_refreshed; status ORBP_REFRESH_SKIPPED for a null or bad point), for the caller to
    // store: MapPoint's members are not reached into.  A point not yet mirrored gets its slot here when `descriptors` is set and is Put
    // first otherwise; a new point whose status is not ORBP_REFRESH_OK stays unmirrored.
    std::vector<orbp_refreshed> Refresh(const std::vector<MapPoint*>& vpMPs, bool descriptors = true);
    // gives up pKF's row of the resident key-frame store: call it when a key frame is deleted
    void ForgetKeyFrame(KeyFrame* pKF);

    // int ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th) (src/ORBmatcher.cc:1016-1134) with the reference's signature and effects
    // (LocalMapPointsFuse.cc; links only when that file and LocalMapPointsRefresh.cc are built in).  Reads of the key frame GetRotation(),
    // GetTranslation(), GetCameraCenter(), fx, fy, cx, cy, GetScaleFactors(), GetScaleLevels(), GetMapPoint() and, once per key frame,
    // GetKeyPointsUn(), GetDescriptors() and its grid (ORBmatcherAccess.h); of the points isBad() and IsInKeyFrame() as of each iteration;
    // calls Replace() or AddObservation() + AddMapPoint() as the reference does.  Points not yet mirrored are Put on the way.
    int Fuse(KeyFrame* pKF, std::vector<MapPoint*>& vpMapPoints, float th = 2.5);
    // Lines :398-430 of LocalMapping::SearchInNeighbors (src/LocalMapping.cc): pCurrent's points into every target key frame (one orbp_fuse for all
    // of them, then the reference's loop per target in order), the candidate list built from the targets as the reference builds it (it
    // sets MapPoint::mnFuseCandidateForKF), and the candidates into pCurrent (one more orbp_fuse, then the loop).  nFused (may be NULL)
    // receives the return value of each of the vpTargetKFs.size() + 1 Fuse calls this replaces.
    void FuseInNeighbors(KeyFrame* pCurrent, const std::vector<KeyFrame*>& vpTargetKFs, float th = 2.5, std::vector<int>* nFused = 0);

    // int ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>& vpMatched, int th)
    // (src/ORBmatcher.cc:286-407, called at src/LoopClosing.cc:370) with the reference's signature and effects (LocalMapPointsLoop.cc; links only
    // when that file, LocalMapPointsFuse.cc and LocalMapPointsRefresh.cc are built in).  Points that are bad or already in vpMatched are passed
    // over, features with vpMatched[idx] != NULL are never matched, vpMatched[idx] receives the matched points; returns the reference's return
    // value.  pKF's features and grid come from the resident key-frame store.  At most ORBF_MAX_FEATURES listed points may pass the tests.
    int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th);
    // The loop of LoopClosing::SearchAndFuse (src/LoopClosing.cc:557-570): ORBmatcher::Fuse(pKF, Scw, vpLoopMapPoints, th) for every corrected key
    // frame.  vCorrectedScw: CorrectedPosesMap in its iteration order, with Converter::toCvMat applied.  One orbp_fuse searches every key frame
    // (nothing in Fuse claims a feature, so an entry's search does not depend on what earlier entries or key frames did); then lines :1152-1261 run
    // per key frame, in order: spAlreadyFound = pKF->GetMapPoints() as the key frame's turn begins, isBad() as of each iteration, and
    // pMPinKF->Replace(pMP), or AddObservation + AddMapPoint, as the reference does.  nFused (may be NULL) receives each call's return value.
    void SearchAndFuse(const std::vector<std::pair<KeyFrame*, cv::Mat> >& vCorrectedScw, const std::vector<MapPoint*>& vpLoopMapPoints, float th = 4,
                       std::vector<int>* nFused = 0);

    // int ORBmatcher::SearchBySim3(KeyFrame*, KeyFrame*, vector<MapPoint*>&, const float&, const cv::Mat&, const cv::Mat&, float)
    // (src/ORBmatcher.cc:1267-1505, called in LoopClosing::ComputeSim3 as SearchBySim3(mpCurrentKF, pKF, vpMapPointMatches, s, R, t, 7.5)) with the
    // reference's signature, return value and effect on vpMatches12 (LocalMapPointsSim3.cc; links only when that file, LocalMapPointsFuse.cc and
    // LocalMapPointsRefresh.cc are built in).  Reads of the key frames GetRotation(), GetTranslation(), GetMapPointMatches(), GetScaleFactors(),
    // GetScaleLevels(), pKF1's fx, fy, cx, cy and, once per key frame, the features and the grid (the resident key-frame store); of the points
    // isBad() and, for those in vpMatches12 on entry, GetIndexInKeyFrame(pKF2).  Points not yet mirrored are Put on the way.
    int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const cv::Mat& R12, const cv::Mat& t12, float th);
    // The same for every converged candidate of one ComputeSim3 against the one pKF1, in ONE call: 2 * vCandidates.size() directions in one launch.
    // Each candidate's vpMatches12 is written as its own call would write it; nFound (may be NULL) receives the return values.
    struct Sim3Candidate {
        KeyFrame* pKF2;
        float s12;
        cv::Mat R12, t12;
        std::vector<MapPoint*>* vpMatches12;
    };
    void SearchBySim3(KeyFrame* pKF1, const std::vector<Sim3Candidate>& vCandidates, float th, std::vector<int>* nFound = 0);

    // int ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:155-281) as Tracking::Relocalisation calls it for every
    // candidate (src/Tracking.cc:880-901, ORBmatcher(0.75, true)), with the reference's effect on vpMapPointMatches and its return value
    // (LocalMapPointsBoW.cc; links only when that file, LocalMapPointsFuse.cc and LocalMapPointsRefresh.cc are built in).  pKF's features come from
    // the resident key-frame store, whose rows also carry the key frame's FeatureVector from the first such call on (GetFeatureVector(), once per
    // key frame, until ForgetKeyFrame); F goes up per call as one extra row (mvKeys, mDescriptors, mFeatVec).  Reads GetMapPointMatches() and isBad().
    int SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches, float nnratio = 0.75f, bool checkOrientation = true);
    // The same for every candidate of one Relocalisation in ONE launch: F goes up once.  vvpMatches[i] is what candidate i's own call leaves; a
    // NULL or bad candidate is passed over with an empty vector and 0 matches, so the caller's loop keeps its shape.
    void SearchByBoW(const std::vector<KeyFrame*>& vpCandidates, Frame& F, std::vector<std::vector<MapPoint*> >& vvpMatches, std::vector<int>* nmatches = 0,
                     float nnratio = 0.75f, bool checkOrientation = true);
    // int ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (src/ORBmatcher.cc:715-850) as LoopClosing::ComputeSim3 calls it for every
    // consistent candidate (src/LoopClosing.cc:246-274, ORBmatcher(0.75, true)).  Both key frames are resident rows: per call only the pair list
    // and the two flag arrays built from GetMapPointMatches() and isBad() go up.
    int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, float nnratio = 0.75f, bool checkOrientation = true);
    // One pKF1 against every candidate in ONE launch; NULL and bad candidates as above.
    void SearchByBoW(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpCandidates, std::vector<std::vector<MapPoint*> >& vvpMatches12,
                     std::vector<int>* nmatches = 0, float nnratio = 0.75f, bool checkOrientation = true);

    // The neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:205-370) between ComputeF12 and `new MapPoint`, for every neighbour in
    // ONE call (LocalMapPointsNewPoints.cc; links only when that file, LocalMapPointsBoW.cc and what it needs are built in): per neighbour
    // ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, ...) of an ORBmatcher(0.6, checkOrientation) and the match loop (:269-353), chained on the
    // device so that a neighbour is not offered the features of pKF1 for which an earlier neighbour's loop reached `new MapPoint` (what AddMapPoint,
    // :360, means to the next search).  vvNew[i]: the accepted (idx1, idx2, x3D) of vpNeighKFs[i] in the order of vMatchedIndices; empty for a
    // neighbour that is NULL, bad, pKF1 itself, listed before, or whose vF12[i] is empty: the caller's loop with its baseline test keeps its shape.
    // Both key frames are resident rows with their FeatureVector; per call the two flag arrays (GetMapPointMatches(): NULL or not), the poses
    // (GetRotation(), GetTranslation(), GetCameraCenter(), fx, fy, cx, cy), the level tables and F12 go up.  NewMapPoint: NewMapPoints.h.
    void CreateNewMapPoints(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpNeighKFs, const std::vector<cv::Mat>& vF12,
                            std::vector<std::vector<NewMapPoint> >& vvNew, bool checkOrientation = false);

    // ---- The local map of Tracking (LocalMapPointsLocalMap.cc; links only when that file and LocalMapPointsRefresh.cc are built in): the three host
    // object-graph walks in front of the local-map search, over a map-point COLUMN per resident key-frame row (include/orbp.h: orbp_local_*).
    // CONTRACT.  Results equal the reference's when the map invariant holds (pKF->mvpMapPoints[idx] == pMP exactly when
    // pMP->mObservations[pKF] == idx, which the reference keeps under its map mutex), bad points have been Forgotten, and every key frame of the
    // map has been Put (PutKeyFrame).  A key frame never Put receives no votes and lists no points.
    //
    // Mirrors pKF->GetMapPointMatches() as the column of pKF's row: points not yet mirrored are Put on the way, NULL or bad points become -1.  Only
    // host state changes here; the column is built and uploaded at the start of the next local-map call.  Column residency is independent of
    // feature, grid and FeatureVector residency; ForgetKeyFrame drops the column too.  Fuse, FuseInNeighbors, SearchAndFuse and
    // CreateNewMapPoints mark the key frames they change themselves; re-Put a key frame whose mvpMapPoints changed elsewhere (INTEGRATION.md lists
    // the places).
    void PutKeyFrame(KeyFrame* pKF);
    // void Tracking::UpdateReferenceKeyFrames() (src/Tracking.cc:764-839) in full, for the frame F: bad points of F.mvpMapPoints are nulled and the
    // slot list is built on the host (a loop over the frame's features only), the votes come from the GPU (one int per row down), and the walk in
    // std::map<KeyFrame*,int> order (pointer order), the bad-key-frame test, the first-maximum rule and the neighbour extension with its `> 80` test at
    // the top of each iteration stay on the host.  KeyFrame::mnTrackReferenceForFrame is written as the reference writes it; vpLocalKeyFrames and
    // pReferenceKF are Tracking's mvpLocalKeyFrames and mpReferenceKF.
    void UpdateReferenceKeyFrames(Frame& F, std::vector<KeyFrame*>& vpLocalKeyFrames, KeyFrame*& pReferenceKF);
    // void Tracking::UpdateReferencePoints() (:738-761) followed by void Tracking::SearchReferencePointsInFrustum() (:675-726).  The first loop over the
    // frame's own points (:678-694) runs on the host; then orbp_local_points_batch_device feeds orbp_track_batch_device on one stream, the list
    // never visits the host on the way, and the list and the records come down once.  The mTrack* write-back, IncreaseVisible() and F.mvpMapPoints
    // are handled as in SearchReferencePointsInFrustum above; returns SearchByProjection's return value (0 when nothing is to match), *nToMatch as
    // there, *vpLocalMapPoints (may be NULL) Tracking's mvpLocalMapPoints.
    // DELIBERATE DEVIATION: MapPoint::mnTrackReferenceForFrame is NOT written.  Nothing but :752 / :757 reads it in the reference, and writing it
    // would reintroduce the per-point walk this call removes.  With F.mnId == 0 the reference lists nothing (the field's initial value is 0, so
    // :752 passes every point over); so does this.
    int SearchLocalMap(Frame& F, const std::vector<KeyFrame*>& vpLocalKeyFrames, float th, std::vector<MapPoint*>* vpLocalMapPoints = 0, int* nToMatch = 0);
    // The counting half of void KeyFrame::UpdateConnections() (src/KeyFrame.cc:334-363): KFcounter as the reference leaves it at :363, the query being
    // the key frame's own column.  The key frame with mnId == pKF->mnId is left out, a key frame with count 0 is absent.  The caller's
    // UpdateConnections continues from :365.
    void ConnectionWeights(KeyFrame* pKF, std::map<KeyFrame*, int>& KFcounter);
    // The same for several key frames (LocalMapping after SearchInNeighbors, LoopClosing::CorrectLoop for a covisibility group): one votes launch
    // per ORBP_LOCAL_MAX_PROBLEMS key frames.
    void ConnectionWeights(const std::vector<KeyFrame*>& vpKFs, std::vector<std::map<KeyFrame*, int> >& vKFcounter);

    // void LocalMapping::KeyFrameCulling() (src/LocalMapping.cc:524-578) for mpCurrentKeyFrame = pCurrentKF (LocalMapPointsCull.cc; links only when
    // that file, LocalMapPointsLocalMap.cc and LocalMapPointsRefresh.cc are built in).  Reads pCurrentKF->GetVectorCovisibleKeyFrames(), leaves out
    // mnId == 0, key frames never Put and NULL or bad ones, runs ONE orbp_cull over the resident slot and octave columns (include/orbp.h: every
    // candidate is judged on the map its predecessors' SetBadFlag calls leave), and calls pKF->SetBadFlag() in list order for the candidates
    // flagged.  After each SetBadFlag() it tests isBad(): a key frame that did not go bad (mbNotErase, which loop closing sets and the host cannot
    // know beforehand) is not erased, so what the device assumed behind it is wrong; the mirror is then brought up to date as after a complete call
    // and the call runs again on the candidates behind it.  At the end ForgetKeyFrame for every key frame that went bad and Forget for every
    // point of those rows that is bad now (the next flush purges them from the resident columns).  *vpCulled (may be NULL): the key frames that
    // went bad, in order.  The same CONTRACT as above; the octaves are read from GetKeyPointsUn() once per key frame and the number of levels from
    // GetScaleLevels().
    void KeyFrameCulling(KeyFrame* pCurrentKF, std::vector<KeyFrame*>* vpCulled = 0);
    // how many orbp_cull calls the last KeyFrameCulling made (more than one: a flagged key frame was protected)
    int keyFrameCullingCalls() const { return cull_calls_; }

    std::size_t size() const { return slot_.size(); }
    int capacity() const { return capacity_; }

private:
    // the columns (LocalMapPointsLocalMap.cc): builds and uploads what PutKeyFrame / ForgetKeyFrame left pending, around flush()
    void syncColumns();
    // the slots of pKF->GetMapPointMatches(): -1 for NULL or bad, Put on the way
    void columnOf(KeyFrame* pKF, std::vector<int32_t>& col);
    void votesFor(const std::vector<int32_t>& query, const std::vector<int32_t>& nquery, int qcap, std::vector<int32_t>& votes);
    // mvpMapPoints of these key frames changed (or is about to, in the caller's hands): the column of each that was Put is read from the key frame
    // again at the next local-map call.  Inline, so that the files that call it need not link LocalMapPointsLocalMap.cc.
    void columnsChanged(const std::vector<KeyFrame*>& kfs) {
        for (std::size_t i = 0; i < kfs.size(); i++) {
            std::unordered_map<KeyFrame*, int>::const_iterator it = kf_row_.find(kfs[i]);
            if (it == kf_row_.end() || (std::size_t)it->second >= kf_col_put_.size() || !kf_col_put_[it->second] || kf_col_dirty_[it->second]) continue;
            kf_col_dirty_[it->second] = 1;
            col_pending_.push_back(it->second);
        }
    }
    std::vector<uint8_t> kf_col_put_, kf_col_dirty_;   // per row: the key frame was Put; its column (or its absence) is to be uploaded
    std::vector<int32_t> col_pending_;           // the rows with kf_col_dirty_
    std::vector<int32_t> kf_col_n_;              // per row: the entries of its column on the device
    void* d_kf_slot_ = nullptr;                  // [col_rows_][col_cap_]
    void* d_kf_col_nt_ = nullptr;                // [col_rows_]
    void* d_kf_oct_ = nullptr;                   // [col_rows_][col_cap_] bytes: the octave of every feature, beside d_kf_slot_ (orbp_cull)
    std::vector<uint8_t> kf_oct_up_;             // per row: its octaves are on the device (read from GetKeyPointsUn() once per key frame and store)
    int cull_calls_ = 0;
    int col_rows_ = 0, col_cap_ = 0;
    void* d_local_ = nullptr;                    // the block of one SearchLocalMap call
    std::size_t local_bytes_ = 0;
    std::vector<uint8_t> local_h_;               // its host image

    // throws std::runtime_error: `what` failed with status rc
    static void fail(const char* what, int rc);
    void flush();
    void purgeColumns();
    void grow();
    void mirror(int slot, MapPoint* pMP);
    void viewOf(Frame& F, orbp_view& V, orbf_bounds& b);
    // the slot of pMP for a search's list: Put first when it is new, or when every call refreshes
    int slotOf(MapPoint* pMP);
    // vpSource[i]: the map point of source feature i (NULL: none); skip_ is filled by the caller
    int searchSource(Frame& CurrentFrame, int mode, const std::vector<MapPoint*>& vpSource, const cv::KeyPoint* srcKeys,
                     const unsigned char* srcDesc, float th, int ORBdist, bool checkOrientation);

    orbp_map* map_ = nullptr;
    float ratio_;
    bool refresh_;
    int capacity_, device_;
    std::unordered_map<MapPoint*, int> slot_;
    std::vector<MapPoint*> owner_;               // per slot; NULL = free
    std::vector<int32_t> free_;                  // free slots, lowest on top
    std::vector<uint8_t> dirty_, dead_;          // per slot: to upload / to erase at the next flush
    std::vector<int32_t> dirty_list_, dead_list_;
    std::vector<float> pos_, nrm_, dmin_, dmax_; // host copy of the table (re-uploaded when it grows)
    std::vector<uint8_t> desc_;
    // the key frames Refresh and Fuse have seen: one row of feat_cap_ key points and descriptors each, resident on the device, and (once Fuse
    // has needed it) the row's grid CSR
    int keyFrameRow(KeyFrame* pKF);
    void growKeyFrames(int rows, int feats);
    void residentForFuse(const std::vector<KeyFrame*>& kfs);
    // the view of pKF's camera inside the bounds b (LocalMapPointsFuse.cc): its own pose, or (Scw != NULL) the decomposition of a similarity
    orbp_view keyFrameView(KeyFrame* pKF, const cv::Mat* Scw, const orbf_bounds& b, float th, int mode);
    // best_idx of orbp_fuse for views[p] = (targets[p], *lists[p]) -> best[p][i]
    // vScw (may be NULL): the views are the decompositions of these similarities (SearchAndFuse)
    void searchFuse(const std::vector<KeyFrame*>& targets, const std::vector<const std::vector<MapPoint*>*>& lists, float th,
                    std::vector<std::vector<int32_t> >& best, const std::vector<cv::Mat>* vScw = 0);
    std::unordered_map<KeyFrame*, int> kf_row_;
    std::vector<KeyFrame*> kf_owner_;            // per row; NULL = free
    std::vector<int32_t> kf_free_;
    std::vector<uint8_t> kf_resident_;           // per row: its features are on the device
    std::vector<uint8_t> kf_grid_resident_;      // per row: its grid is on the device
    std::vector<int32_t> kf_nt_;                 // per row: its number of features
    void* d_kf_kps_ = nullptr;
    void* d_kf_desc_ = nullptr;
    void* d_kf_cell_off_ = nullptr;
    void* d_kf_cell_feat_ = nullptr;
    int kf_rows_ = 0, feat_cap_ = 0;
    // the rows' FeatureVectors (LocalMapPointsBoW.cc), as CSR, for kf_rows_ + 1 rows of feat_cap_: the last row is the frame of the call.  The
    // features' arrays above have that extra row too.
    void residentForBoW(const std::vector<KeyFrame*>& kfs, int frameFeatures);
    void searchBoW(const std::vector<int32_t>& pairs, int frameFeatures, int frameNodes, int th, float nnratio, bool checkOrientation,
                   const std::vector<uint8_t>& qvalid, const std::vector<uint8_t>* claimed, std::vector<int32_t>* q2t, std::vector<int32_t>* t2q,
                   std::vector<int32_t>& found);
    std::vector<uint8_t> kf_fv_resident_;        // per row: its FeatureVector is on the device
    std::vector<int32_t> kf_nfv_;                // per row: its number of nodes
    void* d_kf_fv_node_ = nullptr;
    void* d_kf_fv_off_ = nullptr;
    void* d_kf_fv_feat_ = nullptr;
    int fv_rows_ = 0, fv_cap_ = 0;               // the dimensions the three arrays were allocated for
    // per call
    std::vector<int32_t> list_, t2slot_, t2pos_, cell_off_, cell_feat_;
    std::vector<uint8_t> skip_, claimed_;
    std::vector<orbp_record> rec_;
};

}  // namespace ORB_SLAM
