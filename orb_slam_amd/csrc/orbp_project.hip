// Local map-point table on gfx950: Frame::isInFrustum (reference src/Frame.cc:137-198) and the search windows of
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:57-72) for many poses per launch,
// over map points that stay in HBM.  include/orbp.h is the boundary and states the arithmetic.
//
// Data layout in HBM, per slot: geom = 8 floats (position, mean viewing direction, minDistance, maxDistance: two 16-byte
// loads), desc = 32 bytes (two 16-byte loads), live = 1 byte.
//
// Kernels:
//   k_put      one thread per stored point: scatters the host- or device-side arrays into the slots.
//   k_project<SOURCE>  one workgroup (four waves) per view strides over the view's list with a running base.  Every thread tests one
//              entry; the visible ones are ranked in list order (orbx::tile_rank: ballot + mbcnt inside a wave, the four wave totals
//              meet in LDS), and the survivor writes its window, list position and descriptor at base + rank: list order without
//              atomics.  Only the per-entry test and what a survivor writes depend on SOURCE:
//     <false>  ORBP_MODE_FRAME, the frustum test: three f64 multiply-adds, one f64 sqrt and two f64 divides per point; the stage is
//              bound by the latency of the gathered 64 bytes per entry.
//     <true>   the two projection searches whose list is a source frame's features (orbp.h, ORBP_MODE_LAST_FRAME and
//              ORBP_MODE_KEYFRAME, a run-time field of each view; reference src/ORBmatcher.cc:1507-1746): entry i is feature i of the
//              last frame or of a key frame, the test is the projection and the image bounds only, and a survivor writes the window
//              th * factors[level] over the levels [level-1, level+1], its angle and the source frame's (last frame) or the table's
//              (key frame) descriptor.  The key point's octave and angle do not depend on the slot, so their loads leave with the
//              list's and overlap the dependent list -> live -> geometry chain that bounds the stage.
//   k_t2source every search's last step: turns the search's feature -> query table into feature -> list position (the source feature index of
//              orbp_track_source*) and feature -> map slot through the list positions the projection left (d_qpos); features
//              without a match, or beyond the frame's count, get -1.  Either output may be absent, and so may the list (identity).
// With one workgroup per view the one-view call walks its list as a serial chain of 256-entry tiles (two barriers and a dependent
// list -> live -> geometry load each): its latency grows linearly with the list length.
//
// The host side of every orbp_* entry point is here too; the kernels of the other modes are k_refresh (orbp_refresh.hip), k_fuse
// (orbp_fuse.hip), k_loop_test / k_loop_pack / k_loop_gather (orbp_loop.hip), k_sim3 / k_sim3_agree (orbp_sim3.hip), the local map's (orbp_local.hip) and the key-frame culling's (orbp_cull.hip).  Every search ends in search_tail (window search, then
// k_t2source).  The one-view synchronous forms (orbp_track, orbp_track_source, orbp_loop_search) share one_view over the block orbp::OneView
// of orbp_host.h, where the argument groups, the checks' clauses and the other forms' blocks are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "orbp.h"
#include "orbp_device.h"
#include "orbp_host.h"

namespace orbp {

constexpr int TPB = 256;              // one workgroup: four waves
constexpr int WAVES = TPB / 64;

// what one walk reads and writes
struct Walk {
    const orbp_view* views;
    Table T;
    Lists L;
    Source S;                                          // k_project<true> only
    orbp_record* rec;                                  // k_project<false> only, may be NULL
    Queries Q;                                         // q2t / t2q are not the walk's; qangle k_project<true> only; nq_clamped may be NULL
    int32_t* nq;
    int32_t* overflow;
    int qcap;
};

__global__ __launch_bounds__(TPB) void k_put(int n, const int32_t* slots, const float* pos, const float* normal, const float* dmin,
                                             const float* dmax, const uint8_t* desc, float* geom, uint8_t* tdesc, uint8_t* live) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    float4* g = reinterpret_cast<float4*>(geom) + (size_t)s * 2;
    g[0] = make_float4(pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2], normal[i * 3]);
    g[1] = make_float4(normal[i * 3 + 1], normal[i * 3 + 2], dmin[i], dmax[i]);
    if (desc) {
        uint8_t* d = tdesc + (size_t)s * 32;
        for (int k = 0; k < 32; k++) d[k] = desc[(size_t)i * 32 + k];      // the caller's array need not be aligned
    }
    live[s] = 1;
}

__global__ __launch_bounds__(TPB) void k_erase(int n, const int32_t* slots, uint8_t* live) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) live[slots[i]] = 0;
}

// src/Frame.cc:151-160 (= src/ORBmatcher.cc:1529-1542, :1647-1660): the projection of a point in camera coordinates; true = inside
// the image bounds.  The documented deviation: a NaN projection is outside.
__device__ __forceinline__ bool to_image(const orbp_view& V, const float Pc[3], float& u, float& v) {
    const float invz = (float)(1.0 / (double)Pc[2]);
    u = V.fx * Pc[0] * invz + V.cx;
    v = V.fy * Pc[1] * invz + V.cy;
    if (u < (float)V.min_x || u > (float)V.max_x) return false;
    if (v < (float)V.min_y || v > (float)V.max_y) return false;
    return !(u != u || v != v);
}

// src/Frame.cc:137-198 for one point; true = visible.  Not orbp::entry_test (orbp_device.h) with other constants: the reference's two
// passages differ in every detail, and so do these.  Here 1 / z is a double division, the image bounds are closed, a NaN is rejected by a
// rule of its own (to_image), and the angle test is against the view's limit on view_cos, which the caller needs.
__device__ __forceinline__ bool in_frustum(const orbp_view& V, const Factors& F, const float4 g0, const float4 g1, float& u, float& v,
                                           float& view_cos, int& level) {
    const float P[3] = {g0.x, g0.y, g0.z}, Pn[3] = {g0.w, g1.x, g1.y};
    const float dmin = g1.z, dmax = g1.w;
    float Pc[3];
    to_camera(V, P, Pc);
    if (Pc[2] < 0.0f || !to_image(V, Pc, u, v)) return false;
    double PO[3], dot = 0.0;
    const float dist = centre_distance(V, P, PO);
    if (dist < dmin || dist > dmax) return false;
    for (int k = 0; k < 3; k++) dot = dot + PO[k] * (double)Pn[k];
    view_cos = (float)(dot / (double)dist);
    if (view_cos < V.view_cos_limit) return false;
    level = level_of(F, dist / dmin);
    return true;
}

// src/ORBmatcher.cc:1662-1669: the level predicted from the distance to the camera centre
__device__ __forceinline__ int predicted_level(const orbp_view& V, const Factors& F, const float P[3], float dmin) {
    double PO[3];
    return level_of(F, centre_distance(V, P, PO) / dmin);
}

template <bool SOURCE>
__global__ __launch_bounds__(TPB) void k_project(Walk a, Factors F) {
    __shared__ orbp_view V;
    __shared__ int wave_total[WAVES];
    const int p = blockIdx.x, tid = threadIdx.x;
    stage_view(V, a.views, p);
    __syncthreads();
    const Lists& L = a.L;
    int n = clamp_count(SOURCE || L.list ? L.nlist[p] : a.T.capacity, L.lcap);                          // no list: every slot of the table
    const bool from_last = SOURCE && V.mode == ORBP_MODE_LAST_FRAME;
    const bool known_mode = SOURCE ? (from_last && a.S.desc) || V.mode == ORBP_MODE_KEYFRAME : V.mode == ORBP_MODE_FRAME;
    if (!known_mode) n = 0;                                            // reported below: such a view sees nothing
    const size_t lb = (size_t)p * L.lcap, qb = (size_t)p * a.qcap;
    const float th = V.th;
    int base = 0;                                                      // queries before this tile (uniform)
    for (int i0 = 0; i0 < n; i0 += TPB) {
        const int i = i0 + tid;
        bool vis = false;
        float u = 0.0f, v = 0.0f, vc = 0.0f, angle = 0.0f;
        int level = 0, slot = -1;
        if constexpr (SOURCE) {
            if (i < n) {
                slot = L.list[lb + i];
                const int octave = a.S.kps[lb + i].octave;             // independent of the slot: in flight with the list
                angle = a.S.kps[lb + i].angle;
                if (!(L.skip && L.skip[lb + i]) && slot >= 0 && slot < a.T.capacity && a.T.live[slot]) {
                    const float4* g = reinterpret_cast<const float4*>(a.T.geom) + (size_t)slot * 2;
                    const float4 g0 = g[0];
                    const float P[3] = {g0.x, g0.y, g0.z};
                    float Pc[3];
                    level = from_last ? octave : predicted_level(V, F, P, g[1].z);
                    to_camera(V, P, Pc);                               // no depth test: orbp.h
                    vis = level >= 0 && level < F.n && to_image(V, Pc, u, v);
                }
            }
        } else {
            if (i < n && !(L.skip && L.skip[lb + i])) {
                slot = L.list ? L.list[lb + i] : i;
                if (slot >= 0 && slot < a.T.capacity && a.T.live[slot]) {
                    const float4* g = reinterpret_cast<const float4*>(a.T.geom) + (size_t)slot * 2;
                    vis = in_frustum(V, F, g[0], g[1], u, v, vc, level);
                }
            }
            if (a.rec && i < n) {
                orbp_record r;
                r.in_view = vis ? 1 : 0;
                r.pad[0] = r.pad[1] = r.pad[2] = 0;
                r.u = vis ? u : 0.0f; r.v = vis ? v : 0.0f; r.view_cos = vis ? vc : 0.0f;
                r.level = vis ? level : 0;
                a.rec[lb + i] = r;
            }
        }
        const int q = orbx::tile_rank(vis, wave_total, base);
        if (vis && q < a.qcap) {
            float r = th;
            if constexpr (!SOURCE) {
                r = (double)vc > 0.998 ? 2.5f : 4.0f;                  // RadiusByViewingCos: the float against a double
                if (th != 1.0f) r = r * th;
            }
            float* o = a.Q.qxyr + (qb + q) * 3;
            o[0] = u; o[1] = v; o[2] = r * F.f[level];
            a.Q.qlev[(qb + q) * 2] = level - 1;
            a.Q.qlev[(qb + q) * 2 + 1] = SOURCE ? level + 1 : level;
            if constexpr (SOURCE) a.Q.qangle[qb + q] = angle;
            a.Q.qpos[qb + q] = i;
            const uint4* d = from_last ? reinterpret_cast<const uint4*>(a.S.desc) + (lb + i) * 2 : reinterpret_cast<const uint4*>(a.T.tdesc) + (size_t)slot * 2;
            uint4* od = reinterpret_cast<uint4*>(a.Q.qdesc) + (qb + q) * 2;
            od[0] = d[0]; od[1] = d[1];
        }
    }
    if (tid == 0) {
        a.nq[p] = base;
        if (a.Q.nq_clamped) a.Q.nq_clamped[p] = base > a.qcap ? a.qcap : base;
        a.overflow[p] = !known_mode ? ORBX_ERR_ARG : (base > a.qcap ? 1 : 0);
    }
}

__global__ __launch_bounds__(TPB) void k_t2source(const int32_t* t2q, const int32_t* qpos, const int32_t* list, const int32_t* nt, int cap, int qcap,
                                                  int lcap, int32_t* t2pos, int32_t* t2slot) {
    const int p = blockIdx.y, idx = blockIdx.x * TPB + threadIdx.x;
    if (idx >= cap) return;
    int pos = -1, slot = -1;
    if (idx < nt[p]) {
        const int q = t2q[(size_t)p * cap + idx];
        if (q >= 0 && q < qcap) {
            pos = qpos[(size_t)p * qcap + q];
            slot = list ? list[(size_t)p * lcap + pos] : pos;
        }
    }
    if (t2pos) t2pos[(size_t)p * cap + idx] = pos;
    if (t2slot) t2slot[(size_t)p * cap + idx] = slot;
}

}  // namespace orbp

struct orbp_map {
    int device = 0, capacity = 0, n_live = 0;
    std::mutex mu;
    std::string err;
    std::vector<uint8_t> live;                        // host copy of the live flags
    std::vector<uint32_t> stamp;                      // duplicate check of one put
    uint32_t stamp_now = 0;
    orbx::DevBuf geom, desc, d_live, d_tab, scratch;
    orbx::DevBuf lmult, lfirst, ltiles;               // orbp::LocalScratch of orbp_local_* / orbp_rows_purge_device
    bool local_dirty = true;                          // lmult / lfirst are not (known to be) all 0 / all 0xFF: the next call fills them first
    orbx::DevBuf chist, cdead;                        // orbp::CullScratch of orbp_cull*
    bool cull_dirty = true;                           // chist / cdead are not (known to be) all 0: the next call fills them first
    orbx::PinnedBuf h_tab;
    orbx::Block block;                                // of the synchronous host forms (orbx::Staged), one at a time under `mu`
    orbx::Stream own;
    orbx::Chain chain;                                // device work on the map is ordered across the callers' streams
    orbx::Event tab_done;
    bool tab_pending = false;
};

namespace {

using orbx::DeviceScope;
using orbx::Layout;
using Call = orbx::Call<orbp_map>;
using Staged = orbx::Staged<orbp_map>;

// the slots of a put / erase: range, and for a put no slot twice
int check_slots(orbp_map* m, const int32_t* slots, int n, bool unique, bool need_live) {
    if (unique && ++m->stamp_now == 0) { std::fill(m->stamp.begin(), m->stamp.end(), 0u); m->stamp_now = 1; }
    for (int i = 0; i < n; i++) {
        const int s = slots[i];
        if (s < 0 || s >= m->capacity) return ORBX_ERR_ARG;
        if (need_live && !m->live[s]) return ORBX_ERR_ARG;
        if (unique) {
            if (m->stamp[s] == m->stamp_now) return ORBX_ERR_ARG;
            m->stamp[s] = m->stamp_now;
        }
    }
    return ORBX_OK;
}

// uploads the slot table of one put / erase through the pinned buffer
int upload_slots(orbp_map* m, const int32_t* slots, int n, hipStream_t st) {
    if (m->tab_pending) HIPCHK(m, hipEventSynchronize(m->tab_done));
    m->tab_pending = false;
    if (m->h_tab.size() < (size_t)n * 4) {
        HIPCHK(m, hipStreamSynchronize(st));
        HIPCHK(m, m->chain.wait());
        const size_t want = orbx::doubled(m->h_tab.size(), (size_t)n * 4);
        HIPCHK(m, m->h_tab.ensure(want, hipHostMallocDefault));
        HIPCHK(m, m->d_tab.ensure(want));
    }
    std::memcpy(m->h_tab.as(), slots, (size_t)n * 4);
    HIPCHK(m, hipMemcpyAsync(m->d_tab.as(), m->h_tab.as(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(m, hipEventRecord(m->tab_done, st));
    m->tab_pending = true;
    return ORBX_OK;
}

// inside the caller's call
int put_locked(orbp_map* m, const int32_t* slots, int n, const float* d_pos, const float* d_normal, const float* d_min, const float* d_max,
               const uint8_t* d_desc, hipStream_t st) {
    TRY(upload_slots(m, slots, n, st));
    orbp::k_put<<<(n + orbp::TPB - 1) / orbp::TPB, orbp::TPB, 0, st>>>(n, m->d_tab.as<int32_t>(), d_pos, d_normal, d_min, d_max, d_desc,
                                                                       m->geom.as<float>(), m->desc.as<uint8_t>(), m->d_live.as<uint8_t>());
    HIPCHK(m, hipGetLastError());
    for (int i = 0; i < n; i++)
        if (!m->live[slots[i]]) { m->live[slots[i]] = 1; m->n_live++; }
    return ORBX_OK;
}

// Inside the caller's call: the slot table goes up as for a put, one launch refreshes the slots in place.  The host's
// live flags are the caller's business: orbp_refresh knows the statuses, orbp_refresh_batch_device does not.
int refresh_locked(orbp_map* m, const int32_t* slots, int n, const orbp::RefreshLists& L, const orbp::KeyFrames& K, const orbp::Factors& F, int what,
                   orbp_refreshed* d_out, hipStream_t st) {
    TRY(upload_slots(m, slots, n, st));
    const orbp::Refresh a{n, m->d_tab.as<int32_t>(), L, K, what, m->geom.as<float>(), m->desc.as<uint8_t>(), m->d_live.as<uint8_t>(), d_out};
    HIPCHK(m, orbp::launch_refresh(a, F, st));
    return ORBX_OK;
}

// the slots of a refresh: range, no slot twice, and a free slot only as a new map point (a position and both parts)
int check_refresh_slots(orbp_map* m, const int32_t* slots, int n, bool with_pos, int what) {
    const bool may_create = with_pos && what == (ORBP_REFRESH_NORMAL_DEPTH | ORBP_REFRESH_DESCRIPTOR);
    return check_slots(m, slots, n, true, !may_create);
}

orbp::Table table_of(const orbp_map* m) { return {m->capacity, m->geom.as<float>(), m->desc.as<uint8_t>(), m->d_live.as<uint8_t>()}; }

int fill_factors(const float* factors, int nlevels, orbp::Factors& F) {
    if (!orbp::factors_ok(factors, nlevels)) return ORBX_ERR_ARG;
    std::memset(&F, 0, sizeof(F));
    for (int i = 0; i < nlevels; i++) F.f[i] = factors[i];
    F.n = nlevels;
    return ORBX_OK;
}

int check_walk(const orbp_map* m, const void* d_views, int nviews, const int32_t* d_list, const int32_t* d_nlist, int lcap, int qcap) {
    if (!m || !orbp::views_ok(nviews, lcap) || qcap < 1) return ORBX_ERR_ARG;
    if (nviews > 0 && !d_views) return ORBX_ERR_ARG;
    if (d_list ? !d_nlist : lcap < m->capacity) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// src == NULL: the frustum test of ORBP_MODE_FRAME (rec may be set); else the source-frame modes
void launch_project(orbp_map* m, const orbp_view* d_views, int nviews, const orbp::Factors& F, const orbp::Lists& lists, const orbp::Source* src,
                    orbp_record* d_rec, const orbp::Queries& q, int32_t* d_nq, int32_t* d_overflow, int qcap, hipStream_t st) {
    const orbp::Walk w{d_views, table_of(m), lists, src ? *src : orbp::Source{}, d_rec, q, d_nq, d_overflow, qcap};
    if (src) orbp::k_project<true><<<nviews, orbp::TPB, 0, st>>>(w, F);
    else orbp::k_project<false><<<nviews, orbp::TPB, 0, st>>>(w, F);
}

// what the source-frame walks need beyond check_walk: a list (entry i is feature i of the source frame) and its key points
int check_source(const orbp_map* m, const void* d_views, int nviews, const int32_t* d_list, const int32_t* d_nlist, int lcap, int qcap,
                 const void* d_src_kps, const void* d_src_desc) {
    if (!m || !orbp::views_ok(nviews, lcap) || qcap < 1) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_views || !d_list || !d_nlist || !d_src_kps || ((uintptr_t)d_src_desc & 15)) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The two steps every search ends in, inside the caller's call: the in-order window search of the queries `q` in the frames `fr` (problem p =
// view p), and the result by feature (k_t2source).  q.qangle is null where the rule does not look at angles.
int search_tail(orbp_map* m, const orbf_bounds* b, const orbs_params& prm, const orbp::Frame& fr, const orbp::Queries& q, int qcap, int nviews,
                const orbp::Lists& lists, int32_t* d_t2pos, int32_t* d_t2slot, int32_t* d_nmatches, hipStream_t st) {
    TRY(orbs_window_search_batch_device(b, &prm, fr.kps_un, fr.desc, fr.cell_off, fr.cell_feat, fr.nt, fr.cap, fr.claimed, q.qxyr, q.qlev, q.qdesc, q.qangle, nullptr,
                                        q.nq_clamped, qcap, nviews, q.q2t, q.t2q, nullptr, nullptr, d_nmatches, st));
    orbp::k_t2source<<<dim3((fr.cap + orbp::TPB - 1) / orbp::TPB, nviews), orbp::TPB, 0, st>>>(q.t2q, q.qpos, lists.list, fr.nt, fr.cap, qcap, lists.lcap,
                                                                                              d_t2pos, d_t2slot);
    HIPCHK(m, hipGetLastError());
    return ORBX_OK;
}

// Projection, window search and the result by feature, inside the caller's call.  src == NULL: the frame mode
// (d_t2pos NULL, d_rec may be set).
int track_locked(orbp_map* m, const orbp_view* d_views, int nviews, const orbp::Factors& F, const orbp::Lists& lists, const orbp::Source* src,
                 const orbf_bounds* b, const orbs_params& prm, const orbp::Frame& fr, int qcap, const orbp::Queries& q, orbp_record* d_rec,
                 int32_t* d_t2pos, int32_t* d_t2slot, int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow, hipStream_t st) {
    launch_project(m, d_views, nviews, F, lists, src, d_rec, q, d_nq, d_overflow, qcap, st);
    HIPCHK(m, hipGetLastError());
    return search_tail(m, b, prm, fr, q, qcap, nviews, lists, d_t2pos, d_t2slot, d_nmatches, st);
}

// The device side of orbp_loop_search*, inside the caller's call: the gather of the views' rows (gather slots present), the flat projection,
// the in-order window search and the result by feature.  K: the key frames as the caller laid them out; claimed: per view.
int loop_locked(orbp_map* m, const orbp_view* d_views, int nviews, const orbp::Factors& F, const orbp::Lists& lists, const orbf_bounds* b, int orb_dist,
                const orbp::FuseFrames& K, const uint8_t* d_claimed, int qcap, const orbp::LoopSlots& S, void* scratch, const orbp::LoopOut& out, hipStream_t st) {
    const orbp::Queries q = S.q.at(scratch);
    orbp::Frame fr{K.kps_un, K.desc, K.cell_off, K.cell_feat, K.nt, K.cap, d_claimed};
    if (S.g_kps.present) {
        const orbp::LoopGather g{K, Layout::at(scratch, S.g_kps), Layout::at(scratch, S.g_desc), Layout::at(scratch, S.g_cell_off), Layout::at(scratch, S.g_cell_feat),
                                 Layout::at(scratch, S.g_nt), 0};
        HIPCHK(m, orbp::launch_loop_gather(g, nviews, st));
        fr = {g.kps, g.desc, g.cell_off, g.cell_feat, g.nt, K.cap, d_claimed};
    }
    const orbp::Loop a{d_views, table_of(m), lists, K.frame, K.nframes, out.rec ? out.rec : Layout::at(scratch, S.rec), Layout::at(scratch, S.tile_count), q,
                       out.nq, out.overflow, qcap, 0};
    HIPCHK(m, orbp::launch_loop_project(a, nviews, F, st));
    return search_tail(m, b, {ORBS_RULE_BEST, orb_dist, 0.0f, 0}, fr, q, qcap, nviews, lists, out.t2pos, out.t2slot, out.nmatches, st);
}

// the handle's scratch holds `L`: grown synchronously on the first call of a size, after the device work that may still use it
int fit_scratch(orbp_map* m, const Layout& L) {
    if (L.total() > m->scratch.size()) {
        HIPCHK(m, m->chain.wait());
        HIPCHK(m, m->scratch.ensure(L.total()));
    }
    return ORBX_OK;
}

// The local map's scratch holds `nproblems` problems and `tile_words` tile counts: grown synchronously on the first call of a size, after the device
// work that may still use it.  New words are unknown, so the next local_begin fills them.
int fit_local(orbp_map* m, int nproblems, size_t tile_words) {
    const size_t words = (size_t)nproblems * m->capacity * 4, tiles = tile_words * 4;
    if (words > m->lmult.size() || words > m->lfirst.size() || tiles > m->ltiles.size()) {
        HIPCHK(m, m->chain.wait());
        m->local_dirty = true;
        HIPCHK(m, m->lmult.ensure(words));
        HIPCHK(m, m->lfirst.ensure(words));
        HIPCHK(m, m->ltiles.ensure(tiles));
    }
    return ORBX_OK;
}

// Inside the caller's call, in front of the kernels of orbp_local.hip: the scratch in its between-calls state.  In the steady state the last call
// left it so; after a grow, or a call whose launches failed half way, the whole of it is filled on the stream.  The scratch counts as dirty until
// local_end: every way out in between leaves the flag set.
int local_begin(orbp_map* m, hipStream_t st, orbp::LocalScratch& S) {
    if (m->local_dirty) {
        if (m->lmult.size()) HIPCHK(m, hipMemsetAsync(m->lmult.as(), 0, m->lmult.size(), st));
        if (m->lfirst.size()) HIPCHK(m, hipMemsetAsync(m->lfirst.as(), 0xFF, m->lfirst.size(), st));
    }
    m->local_dirty = true;
    S = {m->lmult.as<uint32_t>(), m->lfirst.as<uint32_t>(), m->ltiles.as<int32_t>()};
    return ORBX_OK;
}
void local_end(orbp_map* m) { m->local_dirty = false; }

int local_votes_locked(orbp_map* m, const orbp::Query& Q, int nproblems, const orbp::Columns& K, int32_t* d_votes, hipStream_t st) {
    orbp::LocalScratch S;
    TRY(local_begin(m, st, S));
    HIPCHK(m, orbp::launch_local_votes({table_of(m), Q, K, S, d_votes}, nproblems, st));
    local_end(m);
    return ORBX_OK;
}

int local_points_locked(orbp_map* m, const orbp::Query& Q, int nproblems, const orbp::RowLists& R, const orbp::Columns& K, const orbp::LocalOut& O, hipStream_t st) {
    orbp::LocalScratch S;
    TRY(local_begin(m, st, S));
    HIPCHK(m, orbp::launch_local_points({table_of(m), Q, R, K, S, O}, nproblems, st));
    local_end(m);
    return ORBX_OK;
}

// The culling's scratch holds the table's capacity: grown synchronously on the first call, after the device work that may still use it, and filled
// by the next cull_locked.
int fit_cull(orbp_map* m) {
    const size_t hist = (size_t)m->capacity * orbp::CULL_WORDS * 4, dead = (size_t)m->capacity * 4;
    if (hist > m->chist.size() || dead > m->cdead.size()) {
        HIPCHK(m, m->chain.wait());
        m->cull_dirty = true;
        HIPCHK(m, m->chist.ensure(hist));
        HIPCHK(m, m->cdead.ensure(dead));
    }
    return ORBX_OK;
}

// Inside the caller's call: the scratch in its between-calls state (local_begin's mechanism: filled on the stream after a grow or a call whose
// launches failed half way, and dirty on every way out but the last), then the kernels of orbp_cull.hip.
int cull_locked(orbp_map* m, const orbp::CullList& C, const orbp::CullColumns& K, const orbp::CullOut& O, hipStream_t st) {
    if (m->cull_dirty && m->chist.size()) {
        HIPCHK(m, hipMemsetAsync(m->chist.as(), 0, m->chist.size(), st));
        HIPCHK(m, hipMemsetAsync(m->cdead.as(), 0, m->cdead.size(), st));
    }
    m->cull_dirty = true;
    HIPCHK(m, orbp::launch_cull({table_of(m), C, K, {m->chist.as<uint32_t>(), m->cdead.as<uint32_t>()}, O}, st));
    m->cull_dirty = false;
    return ORBX_OK;
}

// orbp_track_batch_device / orbp_track_source_batch_device after their argument checks: the queries live in the handle's scratch
int track_batch(orbp_map* m, const orbp_view* d_views, int nviews, const orbp::Factors& F, const orbp::Lists& lists, const orbp::Source* src,
                const orbf_bounds* b, const orbs_params& prm, const orbp::Frame& fr, int qcap, orbp_record* d_rec, int32_t* d_t2pos, int32_t* d_t2slot,
                int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow, void* stream) {
    if (orbs_lds_bytes(fr.cap, qcap) > 160 * 1024) return ORBX_ERR_CAPACITY;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    Layout L;
    orbp::QuerySlots q;
    q.reserve(L, nviews, fr.cap, qcap, src != nullptr);
    TRY(fit_scratch(m, L));
    TRY(c.begin());
    TRY(track_locked(m, d_views, nviews, F, lists, src, b, prm, fr, qcap, q.at(m->scratch.as()), d_rec, d_t2pos, d_t2slot, d_nmatches, d_nq, d_overflow, c.st));
    return c.end();
}

// The one-view synchronous forms after their argument checks: one view through the handle's block `B` (an orbp::OneView), which the caller
// has laid out.  The shared slots are staged, own(s) stages what only this form has, the block goes up, launch(st, d, lists, frame)
// enqueues the kernels on the device block d, and the download span comes back into the caller's arrays.
template <class Block, class Rec, class Own, class Launch>
int one_view(orbp_map* m, void* stream, const Block& B, const orbp::OneViewCall& io, Rec* rec, Own own, Launch launch) {
    Call c(m, stream);
    Staged s(c, m->block, B.L);
    TRY(s.fit());
    orbp::Lists dl;
    orbp::Frame fr;
    B.stage(s.h, s.d, io, dl, fr);
    own(s);
    TRY(s.run([&] { return launch(c.st, s.d, dl, fr); }));
    return B.unpack(s.h, io, rec);
}

// orbp_track / orbp_track_source after their argument checks (orbp::TrackBlock).  src == NULL: the frame mode.  io.frame holds the caller's
// host or device arrays.  Its own: the source frame's key points and descriptors.
int track_one(orbp_map* m, const orbp::OneViewCall& io, const orbp::Factors& F, const orbp::Source* src, bool src_on_device, const orbf_bounds* b,
              const orbs_params& prm, bool frame_on_device, int qcap, orbp_record* rec, void* stream) {
    const int cap = io.frame.cap, lcap = std::max(io.nlist, 1), nlist = io.nlist;
    if (orbs_lds_bytes(cap, qcap) > 160 * 1024) return ORBX_ERR_CAPACITY;
    const bool up_src = src && !src_on_device && nlist > 0;
    const orbp::TrackBlock B(cap, lcap, qcap, {src != nullptr, src || io.list, io.skip != nullptr, up_src, up_src && io.view->mode == ORBP_MODE_LAST_FRAME,
                                              !frame_on_device, io.frame.claimed != nullptr, io.t2slot != nullptr, rec != nullptr});
    orbp::Source d_src{};                                              // staged by the first functor, read by the second: one_view calls them in that order
    return one_view(m, stream, B, io, rec,
        [&](const Staged& s) {
            // with nlist == 0 nothing is read through the source pointers; the kernel still wants them non-NULL for a last-frame view
            d_src = {reinterpret_cast<const orbx_keypoint*>(s.d), s.d};
            if (src && nlist > 0) d_src = {s.put(B.src_kps, src->kps, nlist), s.put(B.src_desc, src->desc, (size_t)nlist * 32)};
        },
        [&](hipStream_t st, uint8_t* d, const orbp::Lists& dl, const orbp::Frame& fr) {
            int32_t* d_res = Layout::at(d, B.result);                      // nq, overflow, nmatches
            return track_locked(m, Layout::at(d, B.view), 1, F, dl, src ? &d_src : nullptr, b, prm, fr, qcap, B.q.at(d), Layout::at(d, B.rec), Layout::at(d, B.t2pos),
                                Layout::at(d, B.t2slot), d_res + 2, d_res, d_res + 1, st);
        });
}

}  // namespace

extern "C" {

int orbp_create(int capacity, int device, orbp_map** out) {
    if (!out || capacity < 1 || capacity > ORBP_MAX_CAPACITY) return ORBX_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return ORBX_ERR_DEVICE;
    DeviceScope ds(device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    orbp_map* m = new orbp_map;
    m->device = device;
    m->capacity = capacity;
    m->live.assign(capacity, 0);
    m->stamp.assign(capacity, 0);
    if (m->geom.ensure((size_t)capacity * 32) != hipSuccess || m->desc.ensure((size_t)capacity * 32) != hipSuccess ||
        m->d_live.ensure((size_t)capacity) != hipSuccess || m->own.ensure() != hipSuccess || m->chain.ev.ensure() != hipSuccess ||
        m->tab_done.ensure() != hipSuccess || hipMemset(m->d_live.as(), 0, (size_t)capacity) != hipSuccess ||
        hipMemset(m->geom.as(), 0, (size_t)capacity * 32) != hipSuccess || hipMemset(m->desc.as(), 0, (size_t)capacity * 32) != hipSuccess) {
        delete m;
        return ORBX_ERR_DEVICE;
    }
    *out = m;
    return ORBX_OK;
}

void orbp_destroy(orbp_map* m) {
    if (!m) return;
    DeviceScope ds(m->device);
    (void)m->chain.wait();                                     // the last piece of device work on the map
    if (m->tab_pending) (void)hipEventSynchronize(m->tab_done);
    delete m;
}

int orbp_capacity(const orbp_map* m) { return m ? m->capacity : 0; }
int orbp_size(const orbp_map* m) { return m ? m->n_live : 0; }

int orbp_clear(orbp_map* m) {
    if (!m) return ORBX_ERR_ARG;
    Call c(m, nullptr);
    TRY(c.begin());
    HIPCHK(m, hipMemsetAsync(m->d_live.as(), 0, (size_t)m->capacity, c.st));
    TRY(c.end());
    HIPCHK(m, hipStreamSynchronize(c.st));
    std::fill(m->live.begin(), m->live.end(), 0);
    m->n_live = 0;
    return ORBX_OK;
}

int orbp_put_device(orbp_map* m, const int32_t* slots, int n, const float* d_pos, const float* d_normal, const float* d_min_dist,
                    const float* d_max_dist, const uint8_t* d_desc, void* stream) {
    if (!m || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!slots || !d_pos || !d_normal || !d_min_dist || !d_max_dist) return ORBX_ERR_ARG;
    Call c(m, stream);
    if (check_slots(m, slots, n, true, d_desc == nullptr) != ORBX_OK) return ORBX_ERR_ARG;
    TRY(c.begin());
    TRY(put_locked(m, slots, n, d_pos, d_normal, d_min_dist, d_max_dist, d_desc, c.st));
    return c.end();
}

int orbp_put(orbp_map* m, const int32_t* slots, int n, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
             const uint8_t* desc) {
    if (!m || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!slots || !pos || !normal || !min_dist || !max_dist) return ORBX_ERR_ARG;
    Call c(m, nullptr);                                                // always the handle's own stream
    if (check_slots(m, slots, n, true, desc == nullptr) != ORBX_OK) return ORBX_ERR_ARG;
    Layout L;
    const auto s_pos = L.add<float>((size_t)n * 3), s_nrm = L.add<float>((size_t)n * 3), s_min = L.add<float>(n), s_max = L.add<float>(n);
    const auto s_desc = L.add<uint8_t>((size_t)n * 32, desc != nullptr);
    L.end_upload();                                                    // nothing comes back
    Staged s(c, m->block, L);
    TRY(s.fit());
    const float *d_pos = s.put(s_pos, pos, (size_t)n * 3), *d_nrm = s.put(s_nrm, normal, (size_t)n * 3), *d_min = s.put(s_min, min_dist, n), *d_max = s.put(s_max, max_dist, n);
    const uint8_t* d_desc = s.put(s_desc, desc, (size_t)n * 32);
    return s.run([&] { return put_locked(m, slots, n, d_pos, d_nrm, d_min, d_max, d_desc, c.st); });
}

int orbp_erase(orbp_map* m, const int32_t* slots, int n) {
    if (!m || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!slots) return ORBX_ERR_ARG;
    Call c(m, nullptr);
    if (check_slots(m, slots, n, false, false) != ORBX_OK) return ORBX_ERR_ARG;
    TRY(c.begin());
    TRY(upload_slots(m, slots, n, c.st));
    orbp::k_erase<<<(n + orbp::TPB - 1) / orbp::TPB, orbp::TPB, 0, c.st>>>(n, m->d_tab.as<int32_t>(), m->d_live.as<uint8_t>());
    HIPCHK(m, hipGetLastError());
    TRY(c.end());
    HIPCHK(m, hipStreamSynchronize(c.st));
    for (int i = 0; i < n; i++)
        if (m->live[slots[i]]) { m->live[slots[i]] = 0; m->n_live--; }
    return ORBX_OK;
}

int orbp_get(orbp_map* m, int slot, int* live, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc) {
    if (!m || !live || slot < 0 || slot >= m->capacity) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lk(m->mu);
    *live = m->live[slot];
    if (!*live) return ORBX_OK;
    if (!pos || !normal || !min_dist || !max_dist || !desc) return ORBX_ERR_ARG;
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    HIPCHK(m, m->chain.wait());
    // a slot that orbp_refresh_batch_device was to create is live on the host and free on the device when its status was not OK
    uint8_t d_live = 0;
    HIPCHK(m, hipMemcpy(&d_live, m->d_live.as<uint8_t>() + slot, 1, hipMemcpyDeviceToHost));
    *live = d_live;
    if (!*live) return ORBX_OK;
    float g[8];
    HIPCHK(m, hipMemcpy(g, m->geom.as<float>() + (size_t)slot * 8, 32, hipMemcpyDeviceToHost));
    HIPCHK(m, hipMemcpy(desc, m->desc.as<uint8_t>() + (size_t)slot * 32, 32, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) { pos[k] = g[k]; normal[k] = g[3 + k]; }
    *min_dist = g[6];
    *max_dist = g[7];
    return ORBX_OK;
}

int orbp_refresh_batch_device(orbp_map* m, const int32_t* slots, int n, const float* d_pos, const int32_t* d_obs_off, const int32_t* d_obs,
                              const int32_t* d_ref, const uint8_t* d_skip, const float* d_kf_ow, const uint8_t* d_kf_bad, const orbx_keypoint* d_kf_kps,
                              const uint8_t* d_kf_desc, int nkf, int cap, const float* factors, int nlevels, int what, orbp_refreshed* d_out,
                              void* stream) {
    const orbp::RefreshLists L{d_pos, d_obs_off, d_obs, d_ref, d_skip};
    const orbp::KeyFrames K{d_kf_ow, d_kf_bad, d_kf_kps, d_kf_desc, nkf, cap};
    orbp::Factors F;
    if (!m || orbp::check_refresh(n, L, K, factors, nlevels, what, true, true) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!slots) return ORBX_ERR_ARG;
    Call c(m, stream);
    if (check_refresh_slots(m, slots, n, d_pos != nullptr, what) != ORBX_OK) return ORBX_ERR_ARG;
    TRY(c.begin());
    TRY(refresh_locked(m, slots, n, L, K, F, what, d_out, c.st));
    TRY(c.end());
    for (int i = 0; i < n; i++)                                        // the statuses stay on the device: orbp.h
        if (!m->live[slots[i]]) { m->live[slots[i]] = 1; m->n_live++; }
    return ORBX_OK;
}

int orbp_refresh(orbp_map* m, const int32_t* slots, int n, const float* pos, const int32_t* obs_off, const int32_t* obs, const int32_t* ref,
                 const uint8_t* skip, const float* kf_ow, const uint8_t* kf_bad, const orbx_keypoint* kf_kps, const uint8_t* kf_desc, int kf_on_device,
                 int nkf, int cap, const float* factors, int nlevels, int what, orbp_refreshed* out, void* stream) {
    const orbp::RefreshLists L{pos, obs_off, obs, ref, skip};
    const orbp::KeyFrames K{kf_ow, kf_bad, kf_kps, kf_desc, nkf, cap};
    orbp::Factors F;
    if (!m || orbp::check_refresh(n, L, K, factors, nlevels, what, false, kf_on_device != 0) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!slots) return ORBX_ERR_ARG;
    Call c(m, stream);
    if (check_refresh_slots(m, slots, n, pos != nullptr, what) != ORBX_OK) return ORBX_ERR_ARG;
    const orbp::RefreshBlock B(n, obs_off[n], L, K, kf_on_device == 0);
    Staged s(c, m->block, B.L);
    TRY(s.fit());
    orbp::RefreshLists dl;
    orbp::KeyFrames dk;
    B.stage(s.h, s.d, L, K, dl, dk);
    TRY(s.run([&] { return refresh_locked(m, slots, n, dl, dk, F, what, Layout::at(s.d, B.out), c.st); }));
    const orbp_refreshed* res = Layout::at(s.h, B.out);
    for (int i = 0; i < n; i++)
        if (res[i].status == ORBP_REFRESH_OK && !m->live[slots[i]]) { m->live[slots[i]] = 1; m->n_live++; }
    if (out) std::memcpy(out, res, (size_t)n * sizeof(orbp_refreshed));
    return ORBX_OK;
}

int orbp_fuse_batch_device(orbp_map* m, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                           const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const orbf_bounds* b, int orb_dist, const orbx_keypoint* d_kps_un,
                           const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat, const int32_t* d_nt, int nframes, int cap,
                           const int32_t* d_frame, int32_t* d_best_idx, int32_t* d_best_dist, orbp_fused* d_rec, void* stream) {
    const orbp::Lists L{d_list, d_nlist, lcap, d_skip};
    const orbp::FuseFrames K{d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, nframes, cap, d_frame};
    const orbp::FuseOut out{d_best_idx, d_best_dist, d_rec};
    orbp::Factors F;
    if (!m || orbp::check_fuse(d_views, nviews, factors, nlevels, L, b, orb_dist, K, out, true, true) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    Call c(m, stream);
    TRY(c.begin());
    const orbp::Fuse a{d_views, table_of(m), L, K, *b, orb_dist, out, 0};
    HIPCHK(m, orbp::launch_fuse(a, nviews, F, c.st));
    return c.end();
}

int orbp_fuse(orbp_map* m, const orbp_view* views, int nviews, const float* factors, int nlevels, const int32_t* list, const int32_t* nlist, int lcap,
              const uint8_t* skip, const orbf_bounds* b, int orb_dist, const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off,
              const int32_t* cell_feat, const int32_t* nt, int nframes, int cap, int frames_on_device, const int32_t* frame, int32_t* best_idx,
              int32_t* best_dist, orbp_fused* rec, void* stream) {
    const orbp::Lists L{list, nlist, lcap, skip};
    const orbp::FuseFrames K{kps_un, desc, cell_off, cell_feat, nt, nframes, cap, frame};
    const orbp::FuseOut out{best_idx, best_dist, rec};
    orbp::Factors F;
    if (!m || orbp::check_fuse(views, nviews, factors, nlevels, L, b, orb_dist, K, out, false, frames_on_device != 0) != ORBX_OK ||
        fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    Call c(m, stream);
    const orbp::FuseBlock B(nviews, L, K, frames_on_device == 0, rec != nullptr);
    Staged s(c, m->block, B.L);
    TRY(s.fit());
    const orbp_view* dv;
    orbp::Lists dl;
    orbp::FuseFrames dk;
    orbp::FuseOut dout;
    B.stage(s.h, s.d, views, L, K, dv, dl, dk, dout);
    TRY(s.run([&]() -> int {
        const orbp::Fuse a{dv, table_of(m), dl, dk, *b, orb_dist, dout, 0};
        HIPCHK(m, orbp::launch_fuse(a, nviews, F, c.st));
        return ORBX_OK;
    }));
    B.unpack(s.h, L, out);                                                // only what the kernel wrote reaches the caller
    return ORBX_OK;
}

int orbp_sim3_from_pair(float s12, const float* R12, const float* t12, const float* R1w, const float* t1w, const float* R2w, const float* t2w, float fx,
                        float fy, float cx, float cy, const orbf_bounds* b, float th, orbp_sim3_dir* dirs) {
    return orbp::sim3_from_pair(s12, R12, t12, R1w, t1w, R2w, t2w, fx, fy, cx, cy, b, th, dirs);
}

int orbp_sim3_search_batch_device(orbp_map* m, const orbp_sim3_dir* d_dirs, int npairs, const float* factors, int nlevels, const int32_t* d_list,
                                  const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const int32_t* d_frame, const orbx_keypoint* d_kps_un,
                                  const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat, const int32_t* d_nt, int nframes, int cap,
                                  const orbf_bounds* b, int orb_dist, int32_t* d_best_idx, int32_t* d_best_dist, orbp_fused* d_rec, int32_t* d_match12,
                                  int32_t* d_nfound, void* stream) {
    const orbp::Lists L{d_list, d_nlist, lcap, d_skip};
    const orbp::FuseFrames K{d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, nframes, cap, d_frame};
    const orbp::FuseOut out{d_best_idx, d_best_dist, d_rec};
    orbp::Factors F;
    if (!m || orbp::check_sim3(d_dirs, npairs, factors, nlevels, L, b, orb_dist, K, out, d_match12, d_nfound, true, true) != ORBX_OK ||
        fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    Call c(m, stream);
    TRY(c.begin());
    const orbp::Sim3 a{d_dirs, table_of(m), L, K, *b, orb_dist, out, d_match12, d_nfound, 0};
    HIPCHK(m, orbp::launch_sim3(a, npairs, F, c.st));
    return c.end();
}

int orbp_sim3_search(orbp_map* m, const orbp_sim3_dir* dirs, int npairs, const float* factors, int nlevels, const int32_t* list, const int32_t* nlist, int lcap,
                     const uint8_t* skip, const int32_t* frame, const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off,
                     const int32_t* cell_feat, const int32_t* nt, int nframes, int cap, int frames_on_device, const orbf_bounds* b, int orb_dist,
                     int32_t* best_idx, int32_t* best_dist, orbp_fused* rec, int32_t* match12, int32_t* nfound, void* stream) {
    const orbp::Lists L{list, nlist, lcap, skip};
    const orbp::FuseFrames K{kps_un, desc, cell_off, cell_feat, nt, nframes, cap, frame};
    const orbp::FuseOut out{best_idx, best_dist, rec};
    orbp::Factors F;
    if (!m || orbp::check_sim3(dirs, npairs, factors, nlevels, L, b, orb_dist, K, out, match12, nfound, false, frames_on_device != 0) != ORBX_OK ||
        fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    Call c(m, stream);
    const orbp::Sim3Block B(npairs, L, K, frames_on_device == 0, rec != nullptr);
    Staged s(c, m->block, B.L);
    TRY(s.fit());
    const orbp_sim3_dir* dv;
    orbp::Lists dl;
    orbp::FuseFrames dk;
    orbp::FuseOut dout;
    B.stage(s.h, s.d, dirs, L, K, dv, dl, dk, dout);
    TRY(s.run([&]() -> int {
        const orbp::Sim3 a{dv, table_of(m), dl, dk, *b, orb_dist, dout, Layout::at(s.d, B.match12), Layout::at(s.d, B.nfound), 0};
        HIPCHK(m, orbp::launch_sim3(a, npairs, F, c.st));
        return ORBX_OK;
    }));
    B.unpack(s.h, L, out);
    for (int p = 0; p < npairs; p++) {
        const int n1 = std::min(std::max(nlist[2 * p], 0), lcap);
        if (n1 > 0) std::memcpy(match12 + (size_t)p * lcap, Layout::at(s.h, B.match12) + (size_t)p * lcap, (size_t)n1 * 4);
    }
    std::memcpy(nfound, Layout::at(s.h, B.nfound), (size_t)npairs * 4);
    return ORBX_OK;
}

int orbp_project_batch_device(orbp_map* m, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                              const int32_t* d_nlist, int lcap, const uint8_t* d_skip, orbp_record* d_rec, float* d_qxyr, int32_t* d_qlev,
                              uint8_t* d_qdesc, int32_t* d_qpos, int32_t* d_nq, int32_t* d_overflow, int qcap, void* stream) {
    orbp::Factors F;
    if (check_walk(m, d_views, nviews, d_list, d_nlist, lcap, qcap) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_qxyr || !d_qlev || !d_qdesc || !d_qpos || !d_nq || !d_overflow) return ORBX_ERR_ARG;
    Call c(m, stream);
    TRY(c.begin());
    launch_project(m, d_views, nviews, F, {d_list, d_nlist, lcap, d_skip}, nullptr, d_rec, {d_qxyr, d_qlev, d_qdesc, d_qpos}, d_nq, d_overflow, qcap, c.st);
    HIPCHK(m, hipGetLastError());
    return c.end();
}

int orbp_track_batch_device(orbp_map* m, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                            const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const orbf_bounds* b, float ratio,
                            const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat,
                            const int32_t* d_nt, int cap, const uint8_t* d_claimed, int qcap, orbp_record* d_rec, int32_t* d_t2slot,
                            int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow, void* stream) {
    orbp::Factors F;
    if (check_walk(m, d_views, nviews, d_list, d_nlist, lcap, qcap) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK) return ORBX_ERR_ARG;
    if (!b || cap < 1 || cap > ORBF_MAX_FEATURES || qcap > ORBF_MAX_FEATURES) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_kps_un || !d_desc || !d_cell_off || !d_cell_feat || !d_nt || !d_t2slot || !d_nmatches || !d_nq || !d_overflow) return ORBX_ERR_ARG;
    return track_batch(m, d_views, nviews, F, {d_list, d_nlist, lcap, d_skip}, nullptr, b, {ORBS_RULE_MAPPOINTS, ORBS_TH_HIGH, ratio, 0},
                       {d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap, d_claimed}, qcap, d_rec, nullptr, d_t2slot, d_nmatches, d_nq, d_overflow, stream);
}

int orbp_track(orbp_map* m, const orbp_view* view, const float* factors, int nlevels, const int32_t* list, int nlist, const uint8_t* skip,
               const orbf_bounds* b, float ratio, const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off,
               const int32_t* cell_feat, const uint8_t* claimed, int nt, int frame_on_device, int qcap, orbp_record* rec, int32_t* t2slot,
               int* nmatches, int* nvisible, void* stream) {
    orbp::Factors F;
    if (!m || !view || !b || nlist < 0 || nt < 0 || nt > ORBF_MAX_FEATURES || qcap < 1 || qcap > ORBF_MAX_FEATURES) return ORBX_ERR_ARG;
    if (fill_factors(factors, nlevels, F) != ORBX_OK || view->mode != ORBP_MODE_FRAME) return ORBX_ERR_ARG;
    if (!list && nlist != m->capacity) return ORBX_ERR_ARG;
    if (!nmatches || (nt > 0 && (!kps_un || !desc || !cell_feat || !t2slot)) || !cell_off) return ORBX_ERR_ARG;
    return track_one(m, {view, list, nlist, skip, {kps_un, desc, cell_off, cell_feat, nullptr, std::max(nt, 1), claimed}, nt, nullptr, t2slot, nmatches, nvisible}, F,
                     nullptr, false, b, {ORBS_RULE_MAPPOINTS, ORBS_TH_HIGH, ratio, 0}, frame_on_device != 0, qcap, rec, stream);
}

int orbp_project_source_batch_device(orbp_map* m, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                                     const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const orbx_keypoint* d_src_kps,
                                     const uint8_t* d_src_desc, float* d_qxyr, int32_t* d_qlev, uint8_t* d_qdesc, float* d_qangle, int32_t* d_qpos,
                                     int32_t* d_nq, int32_t* d_overflow, int qcap, void* stream) {
    orbp::Factors F;
    if (check_source(m, d_views, nviews, d_list, d_nlist, lcap, qcap, d_src_kps, d_src_desc) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_qxyr || !d_qlev || !d_qdesc || ((uintptr_t)d_qdesc & 15) || !d_qangle || !d_qpos || !d_nq || !d_overflow) return ORBX_ERR_ARG;
    Call c(m, stream);
    TRY(c.begin());
    const orbp::Source src{d_src_kps, d_src_desc};
    launch_project(m, d_views, nviews, F, {d_list, d_nlist, lcap, d_skip}, &src, nullptr, {d_qxyr, d_qlev, d_qdesc, d_qpos, nullptr, nullptr, nullptr, d_qangle},
                   d_nq, d_overflow, qcap, c.st);
    HIPCHK(m, hipGetLastError());
    return c.end();
}

int orbp_track_source_batch_device(orbp_map* m, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                                   const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const orbx_keypoint* d_src_kps,
                                   const uint8_t* d_src_desc, const orbf_bounds* b, const orbs_params* prm, const orbx_keypoint* d_kps_un,
                                   const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat, const int32_t* d_nt, int cap,
                                   const uint8_t* d_claimed, int qcap, int32_t* d_t2pos, int32_t* d_t2slot, int32_t* d_nmatches, int32_t* d_nq,
                                   int32_t* d_overflow, void* stream) {
    orbp::Factors F;
    if (check_source(m, d_views, nviews, d_list, d_nlist, lcap, qcap, d_src_kps, d_src_desc) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (!b || !prm || prm->rule != ORBS_RULE_BEST || cap < 1 || cap > ORBF_MAX_FEATURES || qcap > ORBF_MAX_FEATURES) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_kps_un || !d_desc || !d_cell_off || !d_cell_feat || !d_nt || !d_t2pos || !d_nmatches || !d_nq || !d_overflow) return ORBX_ERR_ARG;
    const orbp::Source src{d_src_kps, d_src_desc};
    return track_batch(m, d_views, nviews, F, {d_list, d_nlist, lcap, d_skip}, &src, b, *prm, {d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap, d_claimed},
                       qcap, nullptr, d_t2pos, d_t2slot, d_nmatches, d_nq, d_overflow, stream);
}

int orbp_track_source(orbp_map* m, const orbp_view* view, const float* factors, int nlevels, const int32_t* list, int nlist, const uint8_t* skip,
                      const orbx_keypoint* src_kps, const uint8_t* src_desc, int src_on_device, const orbf_bounds* b, const orbs_params* prm,
                      const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off, const int32_t* cell_feat, const uint8_t* claimed,
                      int nt, int frame_on_device, int qcap, int32_t* t2pos, int32_t* t2slot, int* nmatches, int* nvisible, void* stream) {
    orbp::Factors F;
    if (!m || !view || !b || !prm || prm->rule != ORBS_RULE_BEST || nlist < 0 || nt < 0 || nt > ORBF_MAX_FEATURES || qcap < 1 ||
        qcap > ORBF_MAX_FEATURES)
        return ORBX_ERR_ARG;
    if (fill_factors(factors, nlevels, F) != ORBX_OK) return ORBX_ERR_ARG;
    const bool from_last = view->mode == ORBP_MODE_LAST_FRAME;
    if (!from_last && view->mode != ORBP_MODE_KEYFRAME) return ORBX_ERR_ARG;
    if (nlist > 0 && (!list || !src_kps || (from_last && !src_desc))) return ORBX_ERR_ARG;
    if (src_on_device && ((uintptr_t)src_desc & 15)) return ORBX_ERR_ARG;
    if (!nmatches || (nt > 0 && (!kps_un || !desc || !cell_feat || !t2pos)) || !cell_off) return ORBX_ERR_ARG;
    const orbp::Source src{src_kps, src_desc};
    return track_one(m, {view, list, nlist, skip, {kps_un, desc, cell_off, cell_feat, nullptr, std::max(nt, 1), claimed}, nt, t2pos, t2slot, nmatches, nvisible}, F,
                     &src, src_on_device != 0, b, *prm, frame_on_device != 0, qcap, nullptr, stream);
}

int orbp_view_from_sim3(const float* Scw, orbp_view* view) { return orbp::view_from_sim3(Scw, view); }

int orbp_loop_project_batch_device(orbp_map* m, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                                   const int32_t* d_nlist, int lcap, const uint8_t* d_skip, orbp_fused* d_rec, float* d_qxyr, int32_t* d_qlev,
                                   uint8_t* d_qdesc, int32_t* d_qpos, int32_t* d_nq, int32_t* d_overflow, int qcap, void* stream) {
    const orbp::Lists L{d_list, d_nlist, lcap, d_skip};
    orbp::Factors F;
    if (!m || orbp::check_loop_project(d_views, nviews, factors, nlevels, L, d_rec, {d_qxyr, d_qlev, d_qdesc, d_qpos}, d_nq, d_overflow, qcap) != ORBX_OK ||
        fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    Layout lay;
    orbp::LoopSlots S;
    S.reserve(lay, nviews, lcap, 1, qcap, false, d_rec == nullptr, false);
    TRY(fit_scratch(m, lay));
    TRY(c.begin());
    void* scratch = m->scratch.as();
    const orbp::Loop a{d_views, table_of(m), L, nullptr, 0,
                       d_rec ? d_rec : Layout::at(scratch, S.rec), Layout::at(scratch, S.tile_count), {d_qxyr, d_qlev, d_qdesc, d_qpos}, d_nq, d_overflow, qcap, 0};
    HIPCHK(m, orbp::launch_loop_project(a, nviews, F, c.st));
    return c.end();
}

int orbp_loop_search_batch_device(orbp_map* m, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                                  const int32_t* d_nlist, int lcap, const uint8_t* d_skip, const orbf_bounds* b, int orb_dist, const orbx_keypoint* d_kps_un,
                                  const uint8_t* d_desc, const int32_t* d_cell_off, const int32_t* d_cell_feat, const int32_t* d_nt, int nframes, int cap,
                                  const int32_t* d_frame, const uint8_t* d_claimed, int qcap, orbp_fused* d_rec, int32_t* d_t2pos, int32_t* d_t2slot,
                                  int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow, void* stream) {
    const orbp::Lists L{d_list, d_nlist, lcap, d_skip};
    const orbp::FuseFrames K{d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, nframes, cap, d_frame};
    const orbp::LoopOut out{d_rec, d_t2pos, d_t2slot, d_nmatches, d_nq, d_overflow};
    orbp::Factors F;
    if (!m || orbp::check_loop_search(d_views, nviews, factors, nlevels, L, b, orb_dist, K, qcap, out) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (orbs_lds_bytes(cap, qcap) > 160 * 1024) return ORBX_ERR_CAPACITY;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    Layout lay;
    orbp::LoopSlots S;
    S.reserve(lay, nviews, lcap, cap, qcap, true, d_rec == nullptr, d_frame != nullptr || nviews > nframes);
    TRY(fit_scratch(m, lay));
    TRY(c.begin());
    TRY(loop_locked(m, d_views, nviews, F, L, b, orb_dist, K, d_claimed, qcap, S, m->scratch.as(), out, c.st));
    return c.end();
}

int orbp_loop_search(orbp_map* m, const orbp_view* view, const float* factors, int nlevels, const int32_t* list, int nlist, const uint8_t* skip,
                     const orbf_bounds* b, int orb_dist, const orbx_keypoint* kps_un, const uint8_t* desc, const int32_t* cell_off, const int32_t* cell_feat,
                     const uint8_t* claimed, int nt, int frame_on_device, int qcap, orbp_fused* rec, int32_t* t2pos, int32_t* t2slot, int* nmatches,
                     int* nvisible, void* stream) {
    const int cap = std::max(nt, 1), lcap = std::max(nlist, 1);
    const orbp::Frame frame{kps_un, desc, cell_off, cell_feat, nullptr, cap, claimed};
    orbp::Factors F;
    if (!m || orbp::check_loop_one(view, factors, nlevels, list, nlist, b, orb_dist, frame, nt, frame_on_device != 0, qcap, t2pos, nmatches) != ORBX_OK ||
        fill_factors(factors, nlevels, F) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (orbs_lds_bytes(cap, qcap) > 160 * 1024) return ORBX_ERR_CAPACITY;
    // its own: nothing goes up beyond the shared slots; the queries, the per-tile counts and unwanted records lie behind the download span
    const orbp::LoopBlock B(cap, lcap, qcap, {skip != nullptr, claimed != nullptr, frame_on_device == 0, t2slot != nullptr, rec != nullptr});
    return one_view(m, stream, B, {view, list, nlist, skip, frame, nt, t2pos, t2slot, nmatches, nvisible}, rec, [](const Staged&) {},
        [&](hipStream_t st, uint8_t* d, const orbp::Lists& dl, const orbp::Frame& fr) {
            int32_t* d_res = Layout::at(d, B.result);                      // nq, overflow, nmatches
            const orbp::FuseFrames K{fr.kps_un, fr.desc, fr.cell_off, fr.cell_feat, fr.nt, 1, cap, nullptr};
            return loop_locked(m, Layout::at(d, B.view), 1, F, dl, b, orb_dist, K, fr.claimed, qcap, B.dev, d,
                               {Layout::at(d, B.rec), Layout::at(d, B.t2pos), Layout::at(d, B.t2slot), d_res + 2, d_res, d_res + 1}, st);
        });
}

int orbp_local_votes_batch_device(orbp_map* m, const int32_t* d_query, const int32_t* d_nquery, int qcap, int nproblems, const int32_t* d_kf_slot,
                                  const int32_t* d_kf_nt, int nkf, int cap, int32_t* d_votes, void* stream) {
    const orbp::Query Q{d_query, d_nquery, qcap};
    const orbp::Columns K{d_kf_slot, d_kf_nt, nkf, cap};
    if (!m || orbp::check_local_votes(Q, nproblems, K, d_votes, true, true) != ORBX_OK) return ORBX_ERR_ARG;
    if (nproblems == 0 || nkf == 0) return ORBX_OK;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    TRY(fit_local(m, nproblems, 0));
    TRY(c.begin());
    TRY(local_votes_locked(m, Q, nproblems, K, d_votes, c.st));
    return c.end();
}

int orbp_local_votes(orbp_map* m, const int32_t* query, const int32_t* nquery, int qcap, int nproblems, const int32_t* kf_slot, const int32_t* kf_nt,
                     int kf_on_device, int nkf, int cap, int32_t* votes, void* stream) {
    const orbp::Query Q{query, nquery, qcap};
    const orbp::Columns K{kf_slot, kf_nt, nkf, cap};
    if (!m || orbp::check_local_votes(Q, nproblems, K, votes, false, kf_on_device != 0) != ORBX_OK) return ORBX_ERR_ARG;
    if (nproblems == 0 || nkf == 0) return ORBX_OK;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    TRY(fit_local(m, nproblems, 0));
    const orbp::LocalVotesBlock B(nproblems, Q, K, kf_on_device == 0);
    Staged s(c, m->block, B.L);
    TRY(s.fit());
    orbp::Query dq;
    orbp::Columns dk;
    B.in.stage(s.h, s.d, Q, K, dq, dk);
    TRY(s.run([&] { return local_votes_locked(m, dq, nproblems, dk, Layout::at(s.d, B.votes), c.st); }));
    std::memcpy(votes, Layout::at(s.h, B.votes), B.nvotes * 4);
    return ORBX_OK;
}

int orbp_local_points_batch_device(orbp_map* m, const int32_t* d_query, const int32_t* d_nquery, int qcap, int nproblems, const int32_t* d_rows,
                                   const int32_t* d_nrows, int rcap, const int32_t* d_kf_slot, const int32_t* d_kf_nt, int nkf, int cap, int32_t* d_list,
                                   int32_t* d_nlist, uint8_t* d_skip, int32_t* d_overflow, int lcap, void* stream) {
    const orbp::Query Q{d_query, d_nquery, qcap};
    const orbp::RowLists R{d_rows, d_nrows, rcap};
    const orbp::Columns K{d_kf_slot, d_kf_nt, nkf, cap};
    const orbp::LocalOut O{d_list, d_nlist, d_skip, d_overflow, lcap};
    if (!m || orbp::check_local_points(Q, nproblems, R, K, O, true, true) != ORBX_OK) return ORBX_ERR_ARG;
    if (nproblems == 0) return ORBX_OK;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    TRY(fit_local(m, nproblems, orbp::local_tile_words(nproblems, rcap, cap)));
    TRY(c.begin());
    TRY(local_points_locked(m, Q, nproblems, R, K, O, c.st));
    return c.end();
}

int orbp_local_points(orbp_map* m, const int32_t* query, const int32_t* nquery, int qcap, int nproblems, const int32_t* rows, const int32_t* nrows, int rcap,
                      const int32_t* kf_slot, const int32_t* kf_nt, int kf_on_device, int nkf, int cap, int32_t* list, int32_t* nlist, uint8_t* skip,
                      int32_t* overflow, int lcap, void* stream) {
    const orbp::Query Q{query, nquery, qcap};
    const orbp::RowLists R{rows, nrows, rcap};
    const orbp::Columns K{kf_slot, kf_nt, nkf, cap};
    const orbp::LocalOut O{list, nlist, skip, overflow, lcap};
    if (!m || orbp::check_local_points(Q, nproblems, R, K, O, false, kf_on_device != 0) != ORBX_OK) return ORBX_ERR_ARG;
    if (nproblems == 0) return ORBX_OK;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    TRY(fit_local(m, nproblems, orbp::local_tile_words(nproblems, rcap, cap)));
    const orbp::LocalPointsBlock B(nproblems, Q, R, K, lcap, kf_on_device == 0);
    Staged s(c, m->block, B.L);
    TRY(s.fit());
    orbp::Query dq;
    orbp::RowLists dr;
    orbp::Columns dk;
    orbp::LocalOut dout;
    B.stage(s.h, s.d, Q, R, K, dq, dr, dk, dout);
    TRY(s.run([&] { return local_points_locked(m, dq, nproblems, dr, dk, dout, c.st); }));
    B.unpack(s.h, O);
    return ORBX_OK;
}

int orbp_rows_purge_device(orbp_map* m, const int32_t* slots, int n, int32_t* d_kf_slot, int nkf, int cap, void* stream) {
    if (!m || orbp::check_rows_purge(slots, n, d_kf_slot, nkf, cap) != ORBX_OK) return ORBX_ERR_ARG;
    if (n == 0 || nkf == 0) return ORBX_OK;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    if (check_slots(m, slots, n, false, false) != ORBX_OK) return ORBX_ERR_ARG;
    TRY(fit_local(m, 1, 0));
    TRY(c.begin());
    TRY(upload_slots(m, slots, n, c.st));
    orbp::LocalScratch S;
    TRY(local_begin(m, c.st, S));
    HIPCHK(m, orbp::launch_rows_purge({n, m->d_tab.as<int32_t>(), m->capacity, S.mult, d_kf_slot, (size_t)nkf * cap}, c.st));
    local_end(m);
    return c.end();
}

int orbp_cull_batch_device(orbp_map* m, const int32_t* d_cand, int ncand, const int32_t* d_kf_slot, const uint8_t* d_kf_oct, const int32_t* d_kf_nt, int nkf,
                           int cap, int nlevels, int32_t* d_nmps, int32_t* d_nred, int32_t* d_cull, void* stream) {
    const orbp::CullList C{d_cand, ncand};
    const orbp::CullColumns K{{d_kf_slot, d_kf_nt, nkf, cap}, d_kf_oct, nlevels};
    const orbp::CullOut O{d_nmps, d_nred, d_cull};
    if (!m || orbp::check_cull(C, K, O, true, true) != ORBX_OK) return ORBX_ERR_ARG;
    if (ncand == 0 || nkf == 0) return ORBX_OK;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    TRY(fit_cull(m));
    TRY(c.begin());
    TRY(cull_locked(m, C, K, O, c.st));
    return c.end();
}

int orbp_cull(orbp_map* m, const int32_t* cand, int ncand, const int32_t* kf_slot, const uint8_t* kf_oct, const int32_t* kf_nt, int kf_on_device, int nkf,
              int cap, int nlevels, int32_t* nmps, int32_t* nred, int32_t* cull, void* stream) {
    const orbp::CullList C{cand, ncand};
    const orbp::CullColumns K{{kf_slot, kf_nt, nkf, cap}, kf_oct, nlevels};
    const orbp::CullOut O{nmps, nred, cull};
    if (!m || orbp::check_cull(C, K, O, false, kf_on_device != 0) != ORBX_OK) return ORBX_ERR_ARG;
    if (ncand == 0 || nkf == 0) return ORBX_OK;
    Call c(m, stream);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    TRY(fit_cull(m));
    const orbp::CullBlock B(C, K, kf_on_device == 0);
    Staged s(c, m->block, B.L);
    TRY(s.fit());
    orbp::CullList dc;
    orbp::CullColumns dk;
    orbp::CullOut dout;
    B.stage(s.h, s.d, C, K, dc, dk, dout);
    TRY(s.run([&] { return cull_locked(m, dc, dk, dout, c.st); }));
    B.unpack(s.h, O);
    return ORBX_OK;
}

}  // extern "C"
