// The argument groups of the map-point table's entry points (orbp_project.hip), the clauses their argument checks are composed of, and the
// layouts the synchronous host forms give the one block an orbp_map keeps (orbx::Staged): OneView, the shared form of the one-view calls
// (orbp_track, orbp_track_source: TrackBlock; orbp_loop_search: LoopBlock), RefreshBlock and FlatBlock (orbp_fuse: FuseBlock; orbp_sim3_search:
// Sim3Block), LocalVotesBlock and LocalPointsBlock (orbp_local_votes, orbp_local_points; tests/_probe/local_map_host.cpp) and CullBlock (orbp_cull; tests/_probe/cull_host.cpp).  Each layout's stage() goes through
// Layout::put: a host array is copied into its slot and named on the device, an absent one is passed through.  Host C++ only:
// tests/_probe/host_owners.cpp, tests/_probe/refresh_host.cpp, tests/_probe/fuse_host.cpp, tests/_probe/loop_host.cpp and tests/_probe/sim3_host.cpp hold the checks
// and the layouts against their sizes without a GPU.
#pragma once
#include <cmath>
#include <cstring>

#include "orbp.h"
#include "orbx_host.h"

#pragma GCC visibility push(hidden)
namespace orbp {

using orbx::Layout;

// the table as the kernels read it: geom, tdesc and live per slot
struct Table { int capacity; const float* geom; const uint8_t* tdesc; const uint8_t* live; };
// the lists the views walk (list == NULL: the identity list, frame mode only)
struct Lists { const int32_t* list; const int32_t* nlist; int lcap; const uint8_t* skip; };
// the source frames of the last-frame / key-frame modes, entry i of a list being feature i
struct Source { const orbx_keypoint* kps; const uint8_t* desc; };
// the frames the queries are searched in, as orbf_undistort_grid_batch_device leaves them
struct Frame { const orbx_keypoint* kps_un; const uint8_t* desc; const int32_t* cell_off; const int32_t* cell_feat; const int32_t* nt; int cap; const uint8_t* claimed; };
// the queries between projection and search, in orbs_window_search_batch_device's layout, and the search's two tables
struct Queries { float* qxyr; int32_t* qlev; uint8_t* qdesc; int32_t* qpos; int32_t* nq_clamped; int32_t* q2t; int32_t* t2q; float* qangle; };

// Queries carved from a handle-owned block; qangle for the source modes only
struct QuerySlots {
    Layout::Slot<float> qxyr, qangle;
    Layout::Slot<int32_t> qlev, qpos, nq_clamped, q2t, t2q;
    Layout::Slot<uint8_t> qdesc;
    void reserve(Layout& L, int nviews, int cap, int qcap, bool with_angle) {
        const size_t nqc = (size_t)nviews * qcap;
        qxyr = L.add<float>(nqc * 3); qlev = L.add<int32_t>(nqc * 2); qdesc = L.add<uint8_t>(nqc * 32); qpos = L.add<int32_t>(nqc);
        nq_clamped = L.add<int32_t>(nviews); q2t = L.add<int32_t>(nqc); t2q = L.add<int32_t>((size_t)nviews * cap);
        qangle = L.add<float>(nqc, with_angle);
    }
    Queries at(void* d) const {
        return {Layout::at(d, qxyr), Layout::at(d, qlev), Layout::at(d, qdesc), Layout::at(d, qpos), Layout::at(d, nq_clamped), Layout::at(d, q2t),
                Layout::at(d, t2q), Layout::at(d, qangle)};
    }
};

// One frame of `cap` features in the upload span of a one-view call; absent when the caller's frame is on the device already.  The
// claimed flags have a flag of their own: they go up when they are a host array, which is not the same as "the frame goes up"
// (orbp_track's follow the frame's residence, orbp_loop_search's are a host array beside a resident key frame too).
struct FrameSlots {
    Layout::Slot<orbx_keypoint> kps;
    Layout::Slot<uint8_t> desc, claimed;
    Layout::Slot<int32_t> cell_off, cell_feat;
    void reserve(Layout& L, int cap, bool upload, bool claimed_host) {
        kps = L.add<orbx_keypoint>(cap, upload); desc = L.add<uint8_t>((size_t)cap * 32, upload); cell_off = L.add<int32_t>(ORBF_GRID_CELLS + 1, upload);
        cell_feat = L.add<int32_t>(cap, upload); claimed = L.add<uint8_t>(cap, claimed_host);
    }
    // the caller's frame `f` of nt features as the kernels read it: copied into the pinned block h and named inside the device block d,
    // or passed through
    Frame stage(uint8_t* h, uint8_t* d, const Frame& f, int nt, const int32_t* d_nt) const {
        return {Layout::put(h, d, kps, f.kps_un, nt), Layout::put(h, d, desc, f.desc, (size_t)nt * 32), Layout::put(h, d, cell_off, f.cell_off, ORBF_GRID_CELLS + 1),
                Layout::put(h, d, cell_feat, f.cell_feat, nt), d_nt, f.cap, Layout::put(h, d, claimed, f.claimed, nt)};
    }
};

// what the caller of a one-view form hands in and wants back, beyond its records; frame.cap = max(nt, 1), frame.nt unused
struct OneViewCall { const orbp_view* view; const int32_t* list; int nlist; const uint8_t* skip; Frame frame; int nt; int32_t* t2pos; int32_t* t2slot; int* nmatches; int* nvisible; };

// The block of a one-view synchronous form, one pinned copy up and one down; Rec: the form's record type.
//   up    [view | nt, nlist | list | skip | frame, claimed | the form's own]     (absent: what the caller does not pass or keeps on the device)
//   down  [nq, overflow, nmatches | t2pos | t2slot | rec]                        (absent: what the caller does not want)
// and behind them, on the device only, what the form keeps between its launches.  A form reserves in this order: up(), its own upload
// slots, down(), its device-only tail.
template <class Rec>
struct OneView {
    struct Flags { bool list, skip, frame, claimed_host, t2pos, t2slot, rec; };    // claimed_host: the flags are a host array (FrameSlots)
    Layout L;
    Layout::Slot<orbp_view> view;
    Layout::Slot<int32_t> counts, list, result, t2pos, t2slot;
    Layout::Slot<uint8_t> skip;
    Layout::Slot<Rec> rec;
    FrameSlots frame;
    int cap = 1, lcap = 1;
    Flags flags{};
    void up(int cap_, int lcap_, const Flags& f) {
        cap = cap_; lcap = lcap_; flags = f;
        view = L.add<orbp_view>(1); counts = L.add<int32_t>(2); list = L.add<int32_t>(lcap, f.list); skip = L.add<uint8_t>(lcap, f.skip);
        frame.reserve(L, cap, f.frame, f.claimed_host);
    }
    void down() {
        const Flags& f = flags;
        L.end_upload();
        result = L.add<int32_t>(3); t2pos = L.add<int32_t>(cap, f.t2pos); t2slot = L.add<int32_t>(cap, f.t2slot); rec = L.add<Rec>(lcap, f.rec);
        L.end_download();
    }
    // fills the shared upload slots of the pinned block h and names lists and frame inside the device block d
    void stage(uint8_t* h, uint8_t* d, const OneViewCall& c, Lists& dl, Frame& fr) const {
        std::memcpy(Layout::at(h, view), c.view, sizeof(orbp_view));
        Layout::at(h, counts)[0] = c.nt;
        Layout::at(h, counts)[1] = c.nlist;
        const int32_t* d_counts = Layout::at(d, counts);
        dl = {Layout::put(h, d, list, c.list, c.nlist), d_counts + 1, lcap, Layout::put(h, d, skip, c.skip, c.nlist)};
        fr = frame.stage(h, d, c.frame, c.nt, d_counts);
    }
    // the download span of the pinned block h (result: nq, overflow, nmatches) into the caller's arrays; *nvisible also when the queries overflowed
    int unpack(uint8_t* h, const OneViewCall& c, Rec* out_rec) const {
        const int32_t* res = Layout::at(h, result);
        if (c.nvisible) *c.nvisible = res[0];
        if (res[1]) return ORBX_ERR_CAPACITY;
        *c.nmatches = res[2];
        if (c.nt > 0 && c.t2pos) std::memcpy(c.t2pos, Layout::at(h, t2pos), (size_t)c.nt * 4);
        if (c.nt > 0 && c.t2slot) std::memcpy(c.t2slot, Layout::at(h, t2slot), (size_t)c.nt * 4);
        if (out_rec && c.nlist > 0) std::memcpy(out_rec, Layout::at(h, rec), (size_t)c.nlist * sizeof(Rec));
        return ORBX_OK;
    }
};

// orbp_track / orbp_track_source: OneView, the source frame's key points and descriptors in the upload span, the queries behind the download
// span.  claimed: the caller passes the flags, which follow the frame's residence (on the device with it: a pointer passed through).
struct TrackBlock : OneView<orbp_record> {
    struct Flags { bool source, list, skip, src_kps, src_desc, frame, claimed, t2slot, rec; };    // source: t2pos and the queries' angles
    Layout::Slot<uint8_t> src_desc;
    Layout::Slot<orbx_keypoint> src_kps;
    QuerySlots q;
    TrackBlock(int cap, int lcap, int qcap, const Flags& f) {
        up(cap, lcap, {f.list, f.skip, f.frame, f.frame && f.claimed, f.source, f.t2slot, f.rec});
        src_kps = L.add<orbx_keypoint>(lcap, f.src_kps); src_desc = L.add<uint8_t>((size_t)lcap * 32, f.src_desc);
        down();
        q.reserve(L, 1, cap, qcap, f.source);
    }
};

// mvScaleFactors, by value into the kernels
struct Factors {
    float f[ORBS_MAX_LEVELS];
    int n;
};

// what orbp_refresh* reads: the points' lists and the key-frame store (device pointers by the time the kernel sees them)
struct RefreshLists { const float* pos; const int32_t* obs_off; const int32_t* obs; const int32_t* ref; const uint8_t* skip; };
struct KeyFrames { const float* ow; const uint8_t* bad; const orbx_keypoint* kps; const uint8_t* desc; int nkf, cap; };

// what the refresh kernel reads and writes (orbp_refresh.hip); `slots` is the uploaded slot table
struct Refresh {
    int n;
    const int32_t* slots;
    RefreshLists L;
    KeyFrames K;
    int what;
    float* geom;
    uint8_t* tdesc;
    uint8_t* live;
    orbp_refreshed* out;
};
hipError_t launch_refresh(const Refresh& a, const Factors& F, hipStream_t st);

// The arguments of orbp_refresh* that do not need the handle.  on_device: the lists are device memory (orbp_refresh_batch_device), so
// only their presence can be checked; else obs_off is walked.  kf_device: d_kf_desc is a device address and must be 16-byte aligned (a
// host array is copied into an aligned slot).
inline int check_refresh(int n, const RefreshLists& L, const KeyFrames& K, const float* factors, int nlevels, int what, bool on_device, bool kf_device) {
    if (n < 0 || !factors || nlevels < 2 || nlevels > ORBS_MAX_LEVELS) return ORBX_ERR_ARG;
    if (what == 0 || (what & ~(ORBP_REFRESH_NORMAL_DEPTH | ORBP_REFRESH_DESCRIPTOR))) return ORBX_ERR_ARG;
    if (K.nkf < 1 || K.cap < 1 || (long long)K.nkf * K.cap >= (1ll << 31)) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!L.obs_off || !L.obs || (on_device && ((uintptr_t)L.obs & 7))) return ORBX_ERR_ARG;       // the pairs are read as one 8-byte load
    if ((what & ORBP_REFRESH_NORMAL_DEPTH) && (!L.ref || !K.ow || !K.kps)) return ORBX_ERR_ARG;
    if ((what & ORBP_REFRESH_DESCRIPTOR) && (!K.desc || (kf_device && ((uintptr_t)K.desc & 15)))) return ORBX_ERR_ARG;
    if (!on_device) {
        if (L.obs_off[0] < 0) return ORBX_ERR_ARG;
        for (int i = 0; i < n; i++)
            if (L.obs_off[i + 1] < L.obs_off[i]) return ORBX_ERR_ARG;
    }
    return ORBX_OK;
}

// The block of orbp_refresh, one pinned copy up and one down:
//   up    [pos | obs_off | obs | ref | skip | kf_ow | kf_bad | kf_kps | kf_desc]     (absent: what the caller does not pass, and the
//                                                                                     key frames' features when they are on the device)
//   down  [out]
// `out` is always present: the host needs the statuses for its live flags.
struct RefreshBlock {
    Layout L;
    Layout::Slot<float> pos, kf_ow;
    Layout::Slot<int32_t> obs_off, obs, ref;
    Layout::Slot<uint8_t> skip, kf_bad, kf_desc;
    Layout::Slot<orbx_keypoint> kf_kps;
    Layout::Slot<orbp_refreshed> out;
    int n, nobs, nkf;
    size_t nfeat;                                      // nkf * cap
    RefreshBlock(int n_, int nobs_, const RefreshLists& l, const KeyFrames& k, bool kf_upload) : n(n_), nobs(nobs_), nkf(k.nkf), nfeat((size_t)k.nkf * k.cap) {
        pos = L.add<float>((size_t)n * 3, l.pos != nullptr); obs_off = L.add<int32_t>((size_t)n + 1); obs = L.add<int32_t>((size_t)nobs * 2);
        ref = L.add<int32_t>(n, l.ref != nullptr); skip = L.add<uint8_t>(n, l.skip != nullptr);
        kf_ow = L.add<float>((size_t)nkf * 3, k.ow != nullptr); kf_bad = L.add<uint8_t>(nkf, k.bad != nullptr);
        kf_kps = L.add<orbx_keypoint>(nfeat, kf_upload && k.kps); kf_desc = L.add<uint8_t>(nfeat * 32, kf_upload && k.desc);
        L.end_upload();
        out = L.add<orbp_refreshed>(n);
        L.end_download();
    }
    // copies the caller's host arrays into the pinned block h and names them inside the device block d; the key frames' features are
    // passed through when they are not part of the block
    void stage(uint8_t* h, uint8_t* d, const RefreshLists& l, const KeyFrames& k, RefreshLists& dl, KeyFrames& dk) const {
        dl = {Layout::put(h, d, pos, l.pos, (size_t)n * 3), Layout::put(h, d, obs_off, l.obs_off, (size_t)n + 1), Layout::put(h, d, obs, l.obs, (size_t)nobs * 2),
              Layout::put(h, d, ref, l.ref, n), Layout::put(h, d, skip, l.skip, n)};
        dk = {Layout::put(h, d, kf_ow, k.ow, (size_t)nkf * 3), Layout::put(h, d, kf_bad, k.bad, nkf), Layout::put(h, d, kf_kps, k.kps, nfeat),
              Layout::put(h, d, kf_desc, k.desc, nfeat * 32), k.nkf, k.cap};
    }
};

// what orbp_fuse* reads beyond the lists: the key frames in the batch layout (row f at f*cap, its grid at f*(ORBF_GRID_CELLS+1)), and the row
// each view searches (frame == NULL: view p searches row p)
struct FuseFrames { const orbx_keypoint* kps_un; const uint8_t* desc; const int32_t* cell_off; const int32_t* cell_feat; const int32_t* nt; int nframes, cap; const int32_t* frame; };
struct FuseOut { int32_t* best_idx; int32_t* best_dist; orbp_fused* rec; };

// what the fuse kernel reads and writes (orbp_fuse.hip); p0: the first view of the launch
struct Fuse {
    const orbp_view* views;
    Table T;
    Lists L;
    FuseFrames K;
    orbf_bounds b;
    int orb_dist;
    FuseOut out;
    int p0;
};
hipError_t launch_fuse(const Fuse& a, int nviews, const Factors& F, hipStream_t st);

// gridDim.y holds at most 65535 views, so ORBP_MAX_VIEWS takes a second launch: launch(p0, np) for every chunk of views, up to the first
// HIP error
template <class Launch>
hipError_t for_view_chunks(int nviews, Launch launch) {
    for (int p0 = 0; p0 < nviews; p0 += 65535) {
        const hipError_t e = launch(p0, nviews - p0 < 65535 ? nviews - p0 : 65535);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- the clauses the argument checks are composed of; each returns true when the arguments pass

// the number of views and the stride of their lists
inline bool views_ok(int nviews, int lcap) { return nviews >= 0 && nviews <= ORBP_MAX_VIEWS && lcap >= 1; }
// the scale table
inline bool factors_ok(const float* factors, int nlevels) { return factors && nlevels >= 1 && nlevels <= ORBS_MAX_LEVELS; }
// both for the flat kernels, whose entries and records are indexed p*lcap + i in an int
inline bool flat_views_ok(int nviews, int lcap, const float* factors, int nlevels) {
    return views_ok(nviews, lcap) && factors_ok(factors, nlevels) && (long long)nviews * lcap < (1ll << 31);
}
// the key frames of a search, their grid's bounds and the distance that accepts a match: the sizes ...
inline bool keyframes_ok(const orbf_bounds* b, int orb_dist, const FuseFrames& K) {
    return b && orb_dist >= 0 && orb_dist <= 256 && K.cap >= 1 && K.cap <= ORBF_MAX_FEATURES && K.nframes >= 1 && (long long)K.nframes * K.cap < (1ll << 31);
}
// ... and the arrays
inline bool keyframes_present(const FuseFrames& K) { return K.kps_un && K.desc && K.cell_off && K.cell_feat && K.nt; }
// a frame that is read in place on the device: its descriptors in 16-byte pieces
inline bool frame_aligned(const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off, const int32_t* cell_feat) {
    return !((uintptr_t)desc & 15) && !(((uintptr_t)kps_un | (uintptr_t)cell_off | (uintptr_t)cell_feat) & 3);
}
// every pointer is 4-byte aligned (a null one is)
template <class... P>
bool words_aligned(const P*... p) { return (((uintptr_t)p | ...) & 3) == 0; }

// The arguments of the flat searches (orbp_fuse*: View = orbp_view, mode = ORBP_MODE_FUSE; orbp_sim3_search*: View = orbp_sim3_dir, mode =
// ORBP_MODE_SIM3, a view being one direction) that do not need the handle.  on_device: views, lists and outputs are device memory (the
// batch-device forms), so only their presence and alignment can be checked; else the views' modes and rows are walked.  frames_device: the key
// frames are device addresses, read in place (host arrays are copied into aligned slots).  out_optional: the caller need not want best_idx / best_dist
// (orbp_sim3_search, whose block holds them for the agreement either way).
template <class View>
int check_flat(const View* views, int nviews, const float* factors, int nlevels, const Lists& L, const orbf_bounds* b, int orb_dist, const FuseFrames& K,
               const FuseOut& out, bool on_device, bool frames_device, int mode, bool out_optional = false) {
    if (!flat_views_ok(nviews, L.lcap, factors, nlevels) || !keyframes_ok(b, orb_dist, K)) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!views || !L.list || !L.nlist || !keyframes_present(K) || (!out_optional && (!out.best_idx || !out.best_dist))) return ORBX_ERR_ARG;
    if (frames_device && !frame_aligned(K.kps_un, K.desc, K.cell_off, K.cell_feat)) return ORBX_ERR_ARG;
    if (on_device) return words_aligned(views, L.list, L.nlist, K.nt, K.frame, out.best_idx, out.best_dist, out.rec) ? ORBX_OK : ORBX_ERR_ARG;
    for (int p = 0; p < nviews; p++) {
        const int f = K.frame ? K.frame[p] : p;
        if (views[p].mode != mode || f < 0 || f >= K.nframes) return ORBX_ERR_ARG;
    }
    return ORBX_OK;
}
inline int check_fuse(const orbp_view* views, int nviews, const float* factors, int nlevels, const Lists& L, const orbf_bounds* b, int orb_dist,
                      const FuseFrames& K, const FuseOut& out, bool on_device, bool frames_device) {
    return check_flat(views, nviews, factors, nlevels, L, b, orb_dist, K, out, on_device, frames_device, ORBP_MODE_FUSE);
}

// The block of a flat search over `nviews` views of type View, one pinned copy up and one down:
//   up    [views | nlist | frame | nt | list | skip | kps_un | desc | cell_off | cell_feat]     (absent: frame and skip when the caller passes none,
//                                                                                                the key frames' arrays when they are on the device)
//   down  [best_idx | best_dist | rec | match12 | nfound]                                       (rec absent when the caller wants none; match12 and
//                                                                                                nfound, npairs > 0 only: the agreement of orbp_sim3_search)
template <class View>
struct FlatBlock {
    Layout L;
    Layout::Slot<View> views;
    Layout::Slot<int32_t> nlist, frame, nt, list, cell_off, cell_feat, best_idx, best_dist, match12, nfound;
    Layout::Slot<uint8_t> skip, desc;
    Layout::Slot<orbx_keypoint> kps;
    Layout::Slot<orbp_fused> rec;
    int nviews, nframes;
    size_t nent, nfeat;                                // nviews * lcap, nframes * cap
    FlatBlock(int nviews_, const Lists& l, const FuseFrames& k, bool frames_upload, bool with_rec, int npairs = 0)
        : nviews(nviews_), nframes(k.nframes), nent((size_t)nviews_ * l.lcap), nfeat((size_t)k.nframes * k.cap) {
        views = L.add<View>(nviews); nlist = L.add<int32_t>(nviews); frame = L.add<int32_t>(nviews, k.frame != nullptr); nt = L.add<int32_t>(nframes);
        list = L.add<int32_t>(nent); skip = L.add<uint8_t>(nent, l.skip != nullptr);
        kps = L.add<orbx_keypoint>(nfeat, frames_upload); desc = L.add<uint8_t>(nfeat * 32, frames_upload);
        cell_off = L.add<int32_t>((size_t)nframes * (ORBF_GRID_CELLS + 1), frames_upload); cell_feat = L.add<int32_t>(nfeat, frames_upload);
        L.end_upload();
        best_idx = L.add<int32_t>(nent); best_dist = L.add<int32_t>(nent); rec = L.add<orbp_fused>(nent, with_rec);
        match12 = L.add<int32_t>((size_t)npairs * l.lcap, npairs > 0); nfound = L.add<int32_t>(npairs, npairs > 0);
        L.end_download();
    }
    // copies the caller's host arrays into the pinned block h and names everything inside the device block d; key frames that are not part
    // of the block are passed through
    void stage(uint8_t* h, uint8_t* d, const View* v, const Lists& l, const FuseFrames& k, const View*& dv, Lists& dl, FuseFrames& dk, FuseOut& dout) const {
        dv = Layout::put(h, d, views, v, nviews);
        dl = {Layout::put(h, d, list, l.list, nent), Layout::put(h, d, nlist, l.nlist, nviews), l.lcap, Layout::put(h, d, skip, l.skip, nent)};
        dk = {Layout::put(h, d, kps, k.kps_un, nfeat), Layout::put(h, d, desc, k.desc, nfeat * 32),
              Layout::put(h, d, cell_off, k.cell_off, (size_t)nframes * (ORBF_GRID_CELLS + 1)), Layout::put(h, d, cell_feat, k.cell_feat, nfeat),
              Layout::put(h, d, nt, k.nt, nframes), k.nframes, k.cap, Layout::put(h, d, frame, k.frame, nviews)};
        dout = {Layout::at(d, best_idx), Layout::at(d, best_dist), Layout::at(d, rec)};
    }
    // what the kernel wrote, out of the pinned block h into the caller's arrays (a null one is passed over): entries at i >= nlist[p] stay as they were
    void unpack(uint8_t* h, const Lists& l, const FuseOut& out) const {
        for (int p = 0; p < nviews; p++) {
            const int n = l.nlist[p] < 0 ? 0 : (l.nlist[p] > l.lcap ? l.lcap : l.nlist[p]);
            const size_t e = (size_t)p * l.lcap;
            if (n == 0) continue;
            if (out.best_idx) std::memcpy(out.best_idx + e, Layout::at(h, best_idx) + e, (size_t)n * 4);
            if (out.best_dist) std::memcpy(out.best_dist + e, Layout::at(h, best_dist) + e, (size_t)n * 4);
            if (out.rec) std::memcpy(out.rec + e, Layout::at(h, rec) + e, (size_t)n * sizeof(orbp_fused));
        }
    }
};
using FuseBlock = FlatBlock<orbp_view>;

// ---- SearchBySim3: ORBP_MODE_SIM3 (orbp_sim3.hip)

// orbp_sim3_from_pair: the arithmetic include/orbp.h states, every step a single IEEE operation (the build has -ffp-contract=off)
inline int sim3_from_pair(float s12, const float* R12, const float* t12, const float* R1w, const float* t1w, const float* R2w, const float* t2w, float fx,
                          float fy, float cx, float cy, const orbf_bounds* b, float th, orbp_sim3_dir* dirs) {
    if (!R12 || !t12 || !R1w || !t1w || !R2w || !t2w || !b || !dirs) return ORBX_ERR_ARG;
    if (s12 == 0.0f || !std::isfinite(s12)) return ORBX_ERR_ARG;
    orbp_sim3_dir d12{}, d21{};                        // named by the similarity they carry: d21 is direction 1 -> 2
    const double inv = 1.0 / (double)s12;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            d12.S[r * 3 + c] = (float)((double)R12[r * 3 + c] * (double)s12);
            d21.S[r * 3 + c] = (float)((double)R12[c * 3 + r] * inv);
        }
    for (int r = 0; r < 3; r++) {
        float s = 0.0f;
        for (int k = 0; k < 3; k++) s = s + (-d21.S[r * 3 + k]) * t12[k];
        d21.t[r] = s;
        d12.t[r] = t12[r];
    }
    std::memcpy(d21.Raw, R1w, 36); std::memcpy(d21.taw, t1w, 12);
    std::memcpy(d12.Raw, R2w, 36); std::memcpy(d12.taw, t2w, 12);
    for (orbp_sim3_dir* d : {&d21, &d12}) {
        d->fx = fx; d->fy = fy; d->cx = cx; d->cy = cy;
        d->min_x = b->min_x; d->max_x = b->max_x; d->min_y = b->min_y; d->max_y = b->max_y;
        d->th = th; d->mode = ORBP_MODE_SIM3;
    }
    dirs[0] = d21;
    dirs[1] = d12;
    return ORBX_OK;
}

// what the two kernels of orbp_sim3.hip read and write; the rows are the 2 * npairs directions, K.frame the key frame each searches, p0 the first
// row (k_sim3) or pair (k_sim3_agree) of a launch
struct Sim3 {
    const orbp_sim3_dir* dirs;
    Table T;
    Lists L;
    FuseFrames K;
    orbf_bounds b;
    int orb_dist;
    FuseOut out;
    int32_t* match12;
    int32_t* nfound;
    int p0;
};
hipError_t launch_sim3(const Sim3& a, int npairs, const Factors& F, hipStream_t st);

// The arguments of orbp_sim3_search* that do not need the handle: those of the flat search over the 2 * npairs directions (the directions' own outputs
// are required on the device only), and the agreement's outputs
inline int check_sim3(const orbp_sim3_dir* dirs, int npairs, const float* factors, int nlevels, const Lists& L, const orbf_bounds* b, int orb_dist,
                      const FuseFrames& K, const FuseOut& out, const int32_t* match12, const int32_t* nfound, bool on_device, bool frames_device) {
    if (npairs < 0 || npairs > ORBP_MAX_VIEWS / 2) return ORBX_ERR_ARG;
    const int rc = check_flat(dirs, 2 * npairs, factors, nlevels, L, b, orb_dist, K, out, on_device, frames_device, ORBP_MODE_SIM3, !on_device);
    if (rc != ORBX_OK || npairs == 0) return rc;
    if (!match12 || !nfound || (on_device && !words_aligned(match12, nfound))) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// orbp_sim3_search: the flat block over the directions, with the agreement's outputs in the download span
struct Sim3Block : FlatBlock<orbp_sim3_dir> {
    int npairs;
    Sim3Block(int npairs_, const Lists& l, const FuseFrames& k, bool frames_upload, bool with_rec)
        : FlatBlock<orbp_sim3_dir>(2 * npairs_, l, k, frames_upload, with_rec, npairs_), npairs(npairs_) {}
};

// ---- loop closing: ORBP_MODE_LOOP (orbp_loop.hip) and the view of a similarity

// orbp_view_from_sim3: the arithmetic include/orbp.h states, every step a single IEEE operation (the build has -ffp-contract=off)
inline int view_from_sim3(const float* Scw, orbp_view* view) {
    if (!Scw || !view) return ORBX_ERR_ARG;
    double s2 = 0.0;
    for (int k = 0; k < 3; k++) s2 = s2 + (double)Scw[k] * (double)Scw[k];
    const float scw = (float)std::sqrt(s2);
    if (!(scw > 0.0f) || !std::isfinite(scw)) return ORBX_ERR_ARG;
    float R[9], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) R[r * 3 + c] = (float)((double)Scw[r * 4 + c] / (double)scw);
        t[r] = (float)((double)Scw[r * 4 + 3] / (double)scw);
    }
    for (int c = 0; c < 3; c++) {
        float s = 0.0f;
        for (int k = 0; k < 3; k++) s = s + (-R[k * 3 + c]) * t[k];
        view->Ow[c] = s;
    }
    std::memcpy(view->Rcw, R, sizeof(R));
    std::memcpy(view->tcw, t, sizeof(t));
    return ORBX_OK;
}

constexpr int LOOP_TILE = 256;                         // entries of one workgroup of the loop projection
inline int loop_tiles(int lcap) { return (lcap + LOOP_TILE - 1) / LOOP_TILE; }

// What the two kernels of the loop projection read and write; p0: the first view of the launch.  nframes == 0: the projection alone, no key
// frame to be in range.  rec is never null here: the caller's array or the handle's scratch.  tile_count: the passing entries of every
// (view, tile), loop_tiles(lcap) words per view.  Of Q the kernels write qxyr, qlev, qdesc, qpos and nq_clamped (may be null).
struct Loop {
    const orbp_view* views;
    Table T;
    Lists L;
    const int32_t* frame;
    int nframes;
    orbp_fused* rec;
    int32_t* tile_count;
    Queries Q;
    int32_t* nq;
    int32_t* overflow;
    int qcap;
    int p0;
};
hipError_t launch_loop_project(const Loop& a, int nviews, const Factors& F, hipStream_t st);

// The rows K.frame names (null: row p), copied per view into the layout orbs_window_search_batch_device reads (problem p = view p); a row out
// of range becomes an empty frame.
struct LoopGather {
    FuseFrames K;
    orbx_keypoint* kps;
    uint8_t* desc;
    int32_t* cell_off;
    int32_t* cell_feat;
    int32_t* nt;
    int p0;
};
hipError_t launch_loop_gather(const LoopGather& g, int nviews, hipStream_t st);

struct LoopOut { orbp_fused* rec; int32_t* t2pos; int32_t* t2slot; int32_t* nmatches; int32_t* nq; int32_t* overflow; };

// The arguments of orbp_loop_project_batch_device that do not need the handle (all arrays are device memory: presence and alignment); of q
// the four arrays the projection writes.
inline int check_loop_project(const orbp_view* d_views, int nviews, const float* factors, int nlevels, const Lists& L, const orbp_fused* d_rec,
                              const Queries& q, const int32_t* d_nq, const int32_t* d_overflow, int qcap) {
    if (!flat_views_ok(nviews, L.lcap, factors, nlevels) || qcap < 1) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_views || !L.list || !L.nlist || !q.qxyr || !q.qlev || !q.qdesc || !q.qpos || !d_nq || !d_overflow) return ORBX_ERR_ARG;
    if ((uintptr_t)q.qdesc & 15) return ORBX_ERR_ARG;
    return words_aligned(d_views, L.list, L.nlist, d_rec, q.qxyr, q.qlev, q.qpos, d_nq, d_overflow) ? ORBX_OK : ORBX_ERR_ARG;
}

// The arguments of orbp_loop_search_batch_device that do not need the handle (device memory: presence and alignment; a view's mode and row are
// reported per view by the kernels).  The LDS limit of the search comes after them.
inline int check_loop_search(const orbp_view* d_views, int nviews, const float* factors, int nlevels, const Lists& L, const orbf_bounds* b, int orb_dist,
                             const FuseFrames& K, int qcap, const LoopOut& out) {
    if (!flat_views_ok(nviews, L.lcap, factors, nlevels) || qcap < 1 || qcap > ORBF_MAX_FEATURES || !keyframes_ok(b, orb_dist, K)) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_views || !L.list || !L.nlist || !keyframes_present(K) || !out.t2pos || !out.nmatches || !out.nq || !out.overflow) return ORBX_ERR_ARG;
    if (!frame_aligned(K.kps_un, K.desc, K.cell_off, K.cell_feat)) return ORBX_ERR_ARG;
    return words_aligned(d_views, L.list, L.nlist, K.nt, K.frame, out.rec, out.t2pos, out.t2slot, out.nmatches, out.nq, out.overflow) ? ORBX_OK : ORBX_ERR_ARG;
}

// The arguments of orbp_loop_search (one view, host memory; the key frame on the device when frame_device)
inline int check_loop_one(const orbp_view* view, const float* factors, int nlevels, const int32_t* list, int nlist, const orbf_bounds* b, int orb_dist,
                          const Frame& fr, int nt, bool frame_device, int qcap, const int32_t* t2pos, const int* nmatches) {
    if (!view || !factors_ok(factors, nlevels) || nlist < 0 || nt < 0 || nt > ORBF_MAX_FEATURES || qcap < 1 || qcap > ORBF_MAX_FEATURES)
        return ORBX_ERR_ARG;
    if (!b || orb_dist < 0 || orb_dist > 256 || view->mode != ORBP_MODE_LOOP) return ORBX_ERR_ARG;
    if (nlist > 0 && !list) return ORBX_ERR_ARG;
    if (!nmatches || !fr.cell_off || (nt > 0 && (!fr.kps_un || !fr.desc || !fr.cell_feat || !t2pos))) return ORBX_ERR_ARG;
    if (frame_device && !frame_aligned(fr.kps_un, fr.desc, fr.cell_off, fr.cell_feat)) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// What the loop projection and search keep on the device between their launches, carved from the handle's scratch (batch forms) or from the
// tail of the one-view block: the queries, the per-tile counts, the records when the caller wants none, and the gathered rows.
struct LoopSlots {
    QuerySlots q;
    Layout::Slot<int32_t> tile_count, g_cell_off, g_cell_feat, g_nt;
    Layout::Slot<orbp_fused> rec;
    Layout::Slot<orbx_keypoint> g_kps;
    Layout::Slot<uint8_t> g_desc;
    // search: the search's tables beside the queries (cap: the key frames'); else the caller owns the query arrays
    void reserve(Layout& L, int nviews, int lcap, int cap, int qcap, bool search, bool with_rec, bool gather) {
        if (search) q.reserve(L, nviews, cap, qcap, false);
        tile_count = L.add<int32_t>((size_t)nviews * loop_tiles(lcap));
        rec = L.add<orbp_fused>((size_t)nviews * lcap, with_rec);
        const size_t nfeat = (size_t)nviews * cap;
        g_kps = L.add<orbx_keypoint>(nfeat, gather); g_desc = L.add<uint8_t>(nfeat * 32, gather);
        g_cell_off = L.add<int32_t>((size_t)nviews * (ORBF_GRID_CELLS + 1), gather); g_cell_feat = L.add<int32_t>(nfeat, gather); g_nt = L.add<int32_t>(nviews, gather);
    }
};

// orbp_loop_search: OneView with the list and t2pos always there, and behind the download span the queries, the per-tile counts and the
// records nobody asked for.  claimed: the caller passes the flags, always a host array, also beside a key frame that is resident.
struct LoopBlock : OneView<orbp_fused> {
    struct Flags { bool skip, claimed, frame, t2slot, rec; };
    LoopSlots dev;
    LoopBlock(int cap, int lcap, int qcap, const Flags& f) {
        up(cap, lcap, {true, f.skip, f.frame, f.claimed, true, f.t2slot, f.rec});
        down();
        dev.reserve(L, 1, lcap, cap, qcap, true, !f.rec, false);
    }
};

// ---- the local map: key-frame votes and the local point list over the rows' map-point column (orbp_local.hip)

constexpr int LOCAL_TILE = 256;                        // features of one workgroup of the point list's kernels
inline int local_tiles(int cap) { return (cap + LOCAL_TILE - 1) / LOCAL_TILE; }

// the column of the resident key-frame rows: slot[k*cap + i] the table slot of feature i of row k (or -1), nt[k] the row's feature count
struct Columns { const int32_t* slot; const int32_t* nt; int nkf, cap; };
// the queries: problem p holds the slots q[p*qcap + j], j < nq[p] (q == NULL: no query)
struct Query { const int32_t* q; const int32_t* nq; int qcap; };
// the rows each problem walks, in list order
struct RowLists { const int32_t* rows; const int32_t* nrows; int rcap; };
// the point list as orbp_track_batch_device reads it
struct LocalOut { int32_t* list; int32_t* nlist; uint8_t* skip; int32_t* overflow; int lcap; };
// The handle's scratch.  mult: the query multiplicity of every (problem, slot), all 0 between calls; first: the least walk position of every
// (problem, slot), all 0xFFFFFFFF between calls; tile_count: the kept entries of every (problem, listed row, tile).  The kernels put back what
// they changed.
struct LocalScratch { uint32_t* mult; uint32_t* first; int32_t* tile_count; };
// the words of tile_count
inline size_t local_tile_words(int nproblems, int rcap, int cap) { return (size_t)nproblems * rcap * local_tiles(cap); }

struct LocalVotes { Table T; Query Q; Columns K; LocalScratch S; int32_t* votes; };
struct LocalPoints { Table T; Query Q; RowLists R; Columns K; LocalScratch S; LocalOut O; };
// slots: the uploaded slot table; mark: problem 0 of LocalScratch::mult; nent: nkf * cap
struct RowsPurge { int n; const int32_t* slots; int capacity; uint32_t* mark; int32_t* kf_slot; size_t nent; };
hipError_t launch_local_votes(const LocalVotes& a, int nproblems, hipStream_t st);
hipError_t launch_local_points(const LocalPoints& a, int nproblems, hipStream_t st);
hipError_t launch_rows_purge(const RowsPurge& a, hipStream_t st);

// the sizes of the columns, and of the problems over them
inline bool columns_ok(int nkf, int cap) { return nkf >= 0 && cap >= 1 && (long long)nkf * cap < (1ll << 31); }
inline bool local_problems_ok(int nproblems, int qcap) { return nproblems >= 0 && nproblems <= ORBP_LOCAL_MAX_PROBLEMS && qcap >= 1; }

// The arguments of orbp_local_votes* that do not need the handle.  on_device: query and votes are device memory (alignment is checked); kf_device:
// the columns are.  Nothing to do (no problem or no row) passes before the arrays are looked at.
inline int check_local_votes(const Query& Q, int nproblems, const Columns& K, const int32_t* votes, bool on_device, bool kf_device) {
    if (!local_problems_ok(nproblems, Q.qcap) || !columns_ok(K.nkf, K.cap)) return ORBX_ERR_ARG;
    if (nproblems == 0 || K.nkf == 0) return ORBX_OK;
    if (!Q.q || !Q.nq || !K.slot || !K.nt || !votes) return ORBX_ERR_ARG;
    if (on_device && !words_aligned(Q.q, Q.nq, votes)) return ORBX_ERR_ARG;
    if (kf_device && !words_aligned(K.slot, K.nt)) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The arguments of orbp_local_points* that do not need the handle; on_device / kf_device as above.  The query is optional (with it, its counts are
// required), overflow is optional in the host form; the columns are required only when there are rows to name.
inline int check_local_points(const Query& Q, int nproblems, const RowLists& R, const Columns& K, const LocalOut& O, bool on_device, bool kf_device) {
    if (!local_problems_ok(nproblems, Q.qcap) || !columns_ok(K.nkf, K.cap)) return ORBX_ERR_ARG;
    if (R.rcap < 1 || R.rcap > ORBP_LOCAL_MAX_ROWS || O.lcap < 1) return ORBX_ERR_ARG;
    if ((long long)R.rcap * K.cap >= (1ll << 31) || (long long)nproblems * O.lcap >= (1ll << 31)) return ORBX_ERR_ARG;
    if (nproblems == 0) return ORBX_OK;
    if ((Q.q && !Q.nq) || !R.rows || !R.nrows || !O.list || !O.nlist || !O.skip || (on_device && !O.overflow)) return ORBX_ERR_ARG;
    if (K.nkf > 0 && (!K.slot || !K.nt)) return ORBX_ERR_ARG;
    if (on_device && !words_aligned(Q.q, Q.nq, R.rows, R.nrows, O.list, O.nlist, O.overflow)) return ORBX_ERR_ARG;
    if (kf_device && !words_aligned(K.slot, K.nt)) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The arguments of orbp_rows_purge_device that do not need the handle (the slots' range does)
inline int check_rows_purge(const int32_t* slots, int n, const int32_t* d_kf_slot, int nkf, int cap) {
    if (n < 0 || !columns_ok(nkf, cap)) return ORBX_ERR_ARG;
    if (n == 0 || nkf == 0) return ORBX_OK;
    return slots && d_kf_slot && words_aligned(d_kf_slot) ? ORBX_OK : ORBX_ERR_ARG;
}

// The upload slots the two host forms share: the queries and the columns
struct LocalIn {
    Layout::Slot<int32_t> query, nquery, kf_slot, kf_nt;
    int nproblems = 0, nkf = 0;
    size_t nq = 0, nfeat = 0;                          // nproblems * qcap, nkf * cap
    void reserve(Layout& L, int nproblems_, const Query& Q, const Columns& K, bool kf_upload) {
        nproblems = nproblems_; nkf = K.nkf; nq = (size_t)nproblems * Q.qcap; nfeat = (size_t)K.nkf * K.cap;
        query = L.add<int32_t>(nq, Q.q != nullptr); nquery = L.add<int32_t>(nproblems, Q.q != nullptr);
        kf_slot = L.add<int32_t>(nfeat, kf_upload && K.slot); kf_nt = L.add<int32_t>(nkf, kf_upload && K.nt);
    }
    void stage(uint8_t* h, uint8_t* d, const Query& Q, const Columns& K, Query& dq, Columns& dk) const {
        dq = {Layout::put(h, d, query, Q.q, nq), Layout::put(h, d, nquery, Q.nq, nproblems), Q.qcap};
        dk = {Layout::put(h, d, kf_slot, K.slot, nfeat), Layout::put(h, d, kf_nt, K.nt, nkf), K.nkf, K.cap};
    }
};

// The block of orbp_local_votes, one pinned copy up and one down:
//   up    [query | nquery | kf_slot | kf_nt]     (absent: the columns when they are on the device)
//   down  [votes]
struct LocalVotesBlock {
    Layout L;
    LocalIn in;
    Layout::Slot<int32_t> votes;
    size_t nvotes;                                     // nproblems * nkf
    LocalVotesBlock(int nproblems, const Query& Q, const Columns& K, bool kf_upload) : nvotes((size_t)nproblems * K.nkf) {
        in.reserve(L, nproblems, Q, K, kf_upload);
        L.end_upload();
        votes = L.add<int32_t>(nvotes);
        L.end_download();
    }
};

// The block of orbp_local_points:
//   up    [query | nquery | kf_slot | kf_nt | rows | nrows]     (absent: the query when the caller has none, the columns when they are on the device)
//   down  [nlist | overflow | list | skip]
struct LocalPointsBlock {
    Layout L;
    LocalIn in;
    Layout::Slot<int32_t> rows, nrows, nlist, overflow, list;
    Layout::Slot<uint8_t> skip;
    int nproblems, rcap, lcap;
    LocalPointsBlock(int nproblems_, const Query& Q, const RowLists& R, const Columns& K, int lcap_, bool kf_upload) : nproblems(nproblems_), rcap(R.rcap), lcap(lcap_) {
        in.reserve(L, nproblems, Q, K, kf_upload);
        rows = L.add<int32_t>((size_t)nproblems * rcap); nrows = L.add<int32_t>(nproblems);
        L.end_upload();
        nlist = L.add<int32_t>(nproblems); overflow = L.add<int32_t>(nproblems); list = L.add<int32_t>((size_t)nproblems * lcap);
        skip = L.add<uint8_t>((size_t)nproblems * lcap);
        L.end_download();
    }
    void stage(uint8_t* h, uint8_t* d, const Query& Q, const RowLists& R, const Columns& K, Query& dq, RowLists& dr, Columns& dk, LocalOut& dout) const {
        in.stage(h, d, Q, K, dq, dk);
        dr = {Layout::put(h, d, rows, R.rows, (size_t)nproblems * rcap), Layout::put(h, d, nrows, R.nrows, nproblems), rcap};
        dout = {Layout::at(d, list), Layout::at(d, nlist), Layout::at(d, skip), Layout::at(d, overflow), lcap};
    }
    // what the kernels wrote, out of the pinned block h: the counts, and of every problem the entries it has (at most lcap)
    void unpack(uint8_t* h, const LocalOut& out) const {
        const int32_t* n = Layout::at(h, nlist);
        std::memcpy(out.nlist, n, (size_t)nproblems * 4);
        if (out.overflow) std::memcpy(out.overflow, Layout::at(h, overflow), (size_t)nproblems * 4);
        for (int p = 0; p < nproblems; p++) {
            const size_t e = (size_t)p * lcap, k = n[p] < 0 ? 0 : (n[p] > lcap ? lcap : n[p]);
            if (k == 0) continue;
            std::memcpy(out.list + e, Layout::at(h, list) + e, k * 4);
            std::memcpy(out.skip + e, Layout::at(h, skip) + e, k);
        }
    }
};

// ---- key-frame culling over the slot and octave columns (orbp_cull.hip)

constexpr int CULL_WORDS = 8;                          // words of level counts per slot: sixteen 16-bit fields, level l in word l >> 1 at bit 16 * (l & 1)
// the candidate rows in list order
struct CullList { const int32_t* cand; int ncand; };
// the columns with the octave of every feature beside its slot
struct CullColumns { Columns K; const uint8_t* oct; int nlevels; };
struct CullOut { int32_t* nmps; int32_t* nred; int32_t* cull; };
// The handle's scratch.  hist: CULL_WORDS words per slot; dead: one word per slot; both all 0 between calls, the kernels put back what they changed.
struct CullScratch { uint32_t* hist; uint32_t* dead; };
struct Cull { Table T; CullList C; CullColumns K; CullScratch S; CullOut O; };
hipError_t launch_cull(const Cull& a, hipStream_t st);

// The arguments of orbp_cull* that do not need the handle.  on_device: the candidates and the outputs are device memory (alignment is checked);
// kf_device: the columns are.  Nothing to do (no candidate or no row) passes before the arrays are looked at.
inline int check_cull(const CullList& C, const CullColumns& K, const CullOut& O, bool on_device, bool kf_device) {
    if (C.ncand < 0 || C.ncand > ORBP_CULL_MAX_CANDIDATES || !columns_ok(K.K.nkf, K.K.cap) || K.K.nkf > ORBP_LOCAL_MAX_ROWS) return ORBX_ERR_ARG;
    if (K.nlevels < 1 || K.nlevels > ORBS_MAX_LEVELS) return ORBX_ERR_ARG;
    if (C.ncand == 0 || K.K.nkf == 0) return ORBX_OK;
    if (!C.cand || !K.K.slot || !K.oct || !K.K.nt || !O.nmps || !O.nred || !O.cull) return ORBX_ERR_ARG;
    if (on_device && !words_aligned(C.cand, O.nmps, O.nred, O.cull)) return ORBX_ERR_ARG;
    if (kf_device && !words_aligned(K.K.slot, K.K.nt)) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The block of orbp_cull, one pinned copy up and one down:
//   up    [cand | kf_slot | kf_oct | kf_nt]     (absent: the columns when they are on the device)
//   down  [nmps | nred | cull]
struct CullBlock {
    Layout L;
    Layout::Slot<int32_t> cand, kf_slot, kf_nt, nmps, nred, cull;
    Layout::Slot<uint8_t> kf_oct;
    int ncand, nkf;
    size_t nfeat;                                      // nkf * cap
    CullBlock(const CullList& C, const CullColumns& K, bool kf_upload) : ncand(C.ncand), nkf(K.K.nkf), nfeat((size_t)K.K.nkf * K.K.cap) {
        cand = L.add<int32_t>(ncand);
        kf_slot = L.add<int32_t>(nfeat, kf_upload); kf_oct = L.add<uint8_t>(nfeat, kf_upload); kf_nt = L.add<int32_t>(nkf, kf_upload);
        L.end_upload();
        nmps = L.add<int32_t>(ncand); nred = L.add<int32_t>(ncand); cull = L.add<int32_t>(ncand);
        L.end_download();
    }
    void stage(uint8_t* h, uint8_t* d, const CullList& C, const CullColumns& K, CullList& dc, CullColumns& dk, CullOut& dout) const {
        dc = {Layout::put(h, d, cand, C.cand, ncand), ncand};
        dk = {{Layout::put(h, d, kf_slot, K.K.slot, nfeat), Layout::put(h, d, kf_nt, K.K.nt, nkf), K.K.nkf, K.K.cap}, Layout::put(h, d, kf_oct, K.oct, nfeat), K.nlevels};
        dout = {Layout::at(d, nmps), Layout::at(d, nred), Layout::at(d, cull)};
    }
    void unpack(uint8_t* h, const CullOut& out) const {
        std::memcpy(out.nmps, Layout::at(h, nmps), (size_t)ncand * 4);
        std::memcpy(out.nred, Layout::at(h, nred), (size_t)ncand * 4);
        std::memcpy(out.cull, Layout::at(h, cull), (size_t)ncand * 4);
    }
};

}  // namespace orbp
#pragma GCC visibility pop
