// The argument groups of the map-point walk (orbp_project.hip) and the layouts of the blocks an orbp_map keeps for them.  Host C++
// only: tests/_probe/host_owners.cpp holds the layouts against their sizes without a GPU.
#pragma once
#include <cstring>

#include "orbp.h"
#include "orbx_host.h"

#pragma GCC visibility push(hidden)
namespace orbp {

using orbx::Layout;

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

// One frame of `cap` features in the upload span of a one-view call; absent when the caller's frame is on the device already
struct FrameSlots {
    Layout::Slot<orbx_keypoint> kps;
    Layout::Slot<uint8_t> desc, claimed;
    Layout::Slot<int32_t> cell_off, cell_feat;
    void reserve(Layout& L, int cap, bool upload, bool with_claimed) {
        kps = L.add<orbx_keypoint>(cap, upload); desc = L.add<uint8_t>((size_t)cap * 32, upload); cell_off = L.add<int32_t>(ORBF_GRID_CELLS + 1, upload);
        cell_feat = L.add<int32_t>(cap, upload); claimed = L.add<uint8_t>(cap, upload && with_claimed);
    }
    // the caller's frame `f` of nt features as the kernels read it: copied into the pinned block h and named inside the device block d,
    // or passed through
    Frame stage(uint8_t* h, uint8_t* d, const Frame& f, int nt, const int32_t* d_nt) const {
        if (!kps.present) return {f.kps_un, f.desc, f.cell_off, f.cell_feat, d_nt, f.cap, f.claimed};
        std::memcpy(Layout::at(h, kps), f.kps_un, (size_t)nt * sizeof(orbx_keypoint));
        std::memcpy(Layout::at(h, desc), f.desc, (size_t)nt * 32);
        std::memcpy(Layout::at(h, cell_off), f.cell_off, (size_t)(ORBF_GRID_CELLS + 1) * 4);
        std::memcpy(Layout::at(h, cell_feat), f.cell_feat, (size_t)nt * 4);
        if (claimed.present) std::memcpy(Layout::at(h, claimed), f.claimed, (size_t)nt);
        return {Layout::at(d, kps), Layout::at(d, desc), Layout::at(d, cell_off), Layout::at(d, cell_feat), d_nt, f.cap, Layout::at(d, claimed)};
    }
};

// The block of orbp_track / orbp_track_source, one pinned copy up and one down:
//   up    [view | nt, nlist | list | skip | source key points, descriptors | frame]     (what the caller keeps on the device is absent)
//   down  [nq, overflow, nmatches | t2pos | t2slot | rec]
// and behind them, on the device only, the queries.
struct TrackBlock {
    struct Flags { bool source, list, skip, src_kps, src_desc, frame, claimed, t2slot, rec; };    // source: t2pos and the queries' angles
    Layout L;
    Layout::Slot<orbp_view> view;
    Layout::Slot<int32_t> counts, list, result, t2pos, t2slot;
    Layout::Slot<uint8_t> skip, src_desc;
    Layout::Slot<orbx_keypoint> src_kps;
    Layout::Slot<orbp_record> rec;
    FrameSlots frame;
    QuerySlots q;
    TrackBlock(int cap, int lcap, int qcap, const Flags& f) {
        view = L.add<orbp_view>(1); counts = L.add<int32_t>(2); list = L.add<int32_t>(lcap, f.list); skip = L.add<uint8_t>(lcap, f.skip);
        src_kps = L.add<orbx_keypoint>(lcap, f.src_kps); src_desc = L.add<uint8_t>((size_t)lcap * 32, f.src_desc);
        frame.reserve(L, cap, f.frame, f.claimed);
        L.end_upload();
        result = L.add<int32_t>(3); t2pos = L.add<int32_t>(cap, f.source); t2slot = L.add<int32_t>(cap, f.t2slot); rec = L.add<orbp_record>(lcap, f.rec);
        L.end_download();
        q.reserve(L, 1, cap, qcap, f.source);
    }
};

}  // namespace orbp
#pragma GCC visibility pop
