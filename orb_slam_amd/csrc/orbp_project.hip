// Local map-point table on gfx950: Frame::isInFrustum (reference src/Frame.cc:137-198) and the search windows of
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:57-72) for many poses per launch,
// over map points that stay in HBM.  include/orbp.h is the boundary and states the arithmetic.
//
// Data layout in HBM, per slot: geom = 8 floats (position, mean viewing direction, minDistance, maxDistance: two 16-byte
// loads), desc = 32 bytes (two 16-byte loads), live = 1 byte.
//
// Kernels:
//   k_put      one thread per stored point: scatters the host- or device-side arrays into the slots.
//   k_project  one workgroup (four waves) per view strides over the view's list with a running base.  Every thread tests one
//              entry; the visible ones are ranked inside their wave by ballot + mbcnt, the four wave totals meet in LDS, and
//              the survivor writes its window, list position and descriptor at base + rank: list order without atomics.
//              Three f64 multiply-adds, one f64 sqrt and two f64 divides per point; the stage is bound by the latency of
//              the gathered 64 bytes per entry.
//   k_project_source  the same walk for the two projection searches whose list is a source frame's features (orbp.h, ORBP_MODE_LAST_FRAME
//              and ORBP_MODE_KEYFRAME; reference src/ORBmatcher.cc:1507-1746): entry i is feature i of the last frame or of a key frame,
//              the test is the projection and the image bounds only, and a survivor writes the window th * factors[level] over the
//              levels [level-1, level+1], its angle and the source frame's (last frame) or the table's (key frame) descriptor.
//              The key point's octave and angle do not depend on the slot, so their loads leave with the list's and overlap the
//              dependent list -> live -> geometry chain that bounds the stage.
//   k_t2slot   orbp_track*: turns the search's feature -> query table into feature -> map slot through the list positions the
//              projection left (d_qpos); features without a match, or beyond the frame's count, get -1.
//   k_t2source orbp_track_source*: feature -> query becomes feature -> source feature index (and map slot).
// With one workgroup per view the one-view call walks its list as a serial chain of 256-entry tiles (two barriers and a dependent
// list -> live -> geometry load each): its latency grows linearly with the list length.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "orbp.h"
#include "orbx_host.h"

namespace orbp {

constexpr int TPB = 256;              // one workgroup: four waves
constexpr int WAVES = TPB / 64;

struct Factors {
    float f[ORBS_MAX_LEVELS];
    int n;
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

__device__ __forceinline__ int lane_rank(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// src/Frame.cc:137-198 for one point; true = visible.  Every operation is a single IEEE operation in the reference's order
// (the build has -ffp-contract=off; `0.0f + x` is not an identity in IEEE arithmetic and is kept).
__device__ __forceinline__ bool in_frustum(const orbp_view& V, const Factors& F, const float4 g0, const float4 g1, float& u, float& v,
                                           float& view_cos, int& level) {
    const float P[3] = {g0.x, g0.y, g0.z}, Pn[3] = {g0.w, g1.x, g1.y};
    const float dmin = g1.z, dmax = g1.w;
    float Pc[3];
    for (int r = 0; r < 3; r++) {
        float s = 0.0f;
        s = s + V.Rcw[r * 3] * P[0];
        s = s + V.Rcw[r * 3 + 1] * P[1];
        s = s + V.Rcw[r * 3 + 2] * P[2];
        Pc[r] = s + V.tcw[r];
    }
    if (Pc[2] < 0.0f) return false;
    const float invz = (float)(1.0 / (double)Pc[2]);
    u = V.fx * Pc[0] * invz + V.cx;
    v = V.fy * Pc[1] * invz + V.cy;
    if (u < (float)V.min_x || u > (float)V.max_x) return false;
    if (v < (float)V.min_y || v > (float)V.max_y) return false;
    if (u != u || v != v) return false;                    // the documented deviation: a NaN projection is not visible
    double PO[3];
    for (int k = 0; k < 3; k++) PO[k] = (double)(P[k] - V.Ow[k]);
    double s2 = 0.0, dot = 0.0;
    for (int k = 0; k < 3; k++) s2 = s2 + PO[k] * PO[k];
    const float dist = (float)sqrt(s2);
    if (dist < dmin || dist > dmax) return false;
    for (int k = 0; k < 3; k++) dot = dot + PO[k] * (double)Pn[k];
    view_cos = (float)(dot / (double)dist);
    if (view_cos < V.view_cos_limit) return false;
    const float ratio = dist / dmin;
    int lv = 0;
    for (int k = 0; k < F.n; k++) lv += F.f[k] < ratio ? 1 : 0;       // std::lower_bound on the ascending table
    level = lv >= F.n ? F.n - 1 : lv;
    return true;
}

__global__ __launch_bounds__(TPB) void k_project(const orbp_view* views, Factors F, int capacity, const float* geom, const uint8_t* tdesc,
                                                 const uint8_t* live, const int32_t* list, const int32_t* nlist, int lcap,
                                                 const uint8_t* skip, orbp_record* rec, float* qxyr, int32_t* qlev, uint8_t* qdesc,
                                                 int32_t* qpos, int32_t* nq, int32_t* nq_clamped, int32_t* overflow, int qcap) {
    __shared__ orbp_view V;
    __shared__ int wave_total[WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    if (tid < (int)(sizeof(orbp_view) / 4)) reinterpret_cast<uint32_t*>(&V)[tid] = reinterpret_cast<const uint32_t*>(views + p)[tid];
    __syncthreads();
    int n = list ? nlist[p] : capacity;
    n = n < 0 ? 0 : (n > lcap ? lcap : n);
    const bool known_mode = V.mode == ORBP_MODE_FRAME;
    if (!known_mode) n = 0;                                            // reported below: such a view sees nothing
    const size_t lb = (size_t)p * lcap, qb = (size_t)p * qcap;
    const float th = V.th;
    int base = 0;                                                      // visible entries before this tile (uniform)
    for (int i0 = 0; i0 < n; i0 += TPB) {
        const int i = i0 + tid;
        bool vis = false;
        float u = 0.0f, v = 0.0f, vc = 0.0f;
        int level = 0, slot = -1;
        if (i < n && !(skip && skip[lb + i])) {
            slot = list ? list[lb + i] : i;
            if (slot >= 0 && slot < capacity && live[slot]) {
                const float4* g = reinterpret_cast<const float4*>(geom) + (size_t)slot * 2;
                vis = in_frustum(V, F, g[0], g[1], u, v, vc, level);
            }
        }
        if (rec && i < n) {
            orbp_record r;
            r.in_view = vis ? 1 : 0;
            r.pad[0] = r.pad[1] = r.pad[2] = 0;
            r.u = vis ? u : 0.0f; r.v = vis ? v : 0.0f; r.view_cos = vis ? vc : 0.0f;
            r.level = vis ? level : 0;
            rec[lb + i] = r;
        }
        const unsigned long long m = __ballot(vis);
        if ((tid & 63) == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < WAVES; w++) {
            const int c = wave_total[w];
            before += w < wave ? c : 0;
            total += c;
        }
        const int q = before + lane_rank(m);
        if (vis && q < qcap) {
            float r = (double)vc > 0.998 ? 2.5f : 4.0f;                // RadiusByViewingCos: the float against a double
            if (th != 1.0f) r = r * th;
            float* o = qxyr + (qb + q) * 3;
            o[0] = u; o[1] = v; o[2] = r * F.f[level];
            qlev[(qb + q) * 2] = level - 1;
            qlev[(qb + q) * 2 + 1] = level;
            qpos[qb + q] = i;
            const uint4* d = reinterpret_cast<const uint4*>(tdesc) + (size_t)slot * 2;
            uint4* od = reinterpret_cast<uint4*>(qdesc) + (qb + q) * 2;
            od[0] = d[0]; od[1] = d[1];
        }
        base += total;
        __syncthreads();                                               // wave_total is rewritten by the next tile
    }
    if (tid == 0) {
        nq[p] = base;
        if (nq_clamped) nq_clamped[p] = base > qcap ? qcap : base;
        if (overflow) overflow[p] = !known_mode ? ORBX_ERR_ARG : (base > qcap ? 1 : 0);
    }
}

// Rcw * P + tcw as the reference's cv::Mat product evaluates it (in_frustum above)
__device__ __forceinline__ void to_camera(const orbp_view& V, const float P[3], float Pc[3]) {
    for (int r = 0; r < 3; r++) {
        float s = 0.0f;
        s = s + V.Rcw[r * 3] * P[0];
        s = s + V.Rcw[r * 3 + 1] * P[1];
        s = s + V.Rcw[r * 3 + 2] * P[2];
        Pc[r] = s + V.tcw[r];
    }
}

// src/ORBmatcher.cc:1529-1542 (= :1647-1660) for one point: no depth test; true = inside the image bounds
__device__ __forceinline__ bool project_source(const orbp_view& V, const float P[3], float& u, float& v) {
    float Pc[3];
    to_camera(V, P, Pc);
    const float invz = (float)(1.0 / (double)Pc[2]);
    u = V.fx * Pc[0] * invz + V.cx;
    v = V.fy * Pc[1] * invz + V.cy;
    if (u < (float)V.min_x || u > (float)V.max_x) return false;
    if (v < (float)V.min_y || v > (float)V.max_y) return false;
    return !(u != u || v != v);                            // the documented deviation: a NaN projection is not a query
}

// src/ORBmatcher.cc:1662-1669: the level predicted from the distance to the camera centre
__device__ __forceinline__ int predicted_level(const orbp_view& V, const Factors& F, const float P[3], float dmin) {
    double s2 = 0.0;
    for (int k = 0; k < 3; k++) {
        const double d = (double)(P[k] - V.Ow[k]);
        s2 = s2 + d * d;
    }
    const float ratio = (float)sqrt(s2) / dmin;
    int lv = 0;
    for (int k = 0; k < F.n; k++) lv += F.f[k] < ratio ? 1 : 0;       // std::lower_bound on the ascending table
    return lv >= F.n ? F.n - 1 : lv;
}

__global__ __launch_bounds__(TPB) void k_project_source(const orbp_view* views, Factors F, int capacity, const float* geom, const uint8_t* tdesc,
                                                        const uint8_t* live, const int32_t* list, const int32_t* nlist, int lcap,
                                                        const uint8_t* skip, const orbx_keypoint* src_kps, const uint8_t* src_desc, float* qxyr,
                                                        int32_t* qlev, uint8_t* qdesc, float* qangle, int32_t* qpos, int32_t* nq,
                                                        int32_t* nq_clamped, int32_t* overflow, int qcap) {
    __shared__ orbp_view V;
    __shared__ int wave_total[WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    if (tid < (int)(sizeof(orbp_view) / 4)) reinterpret_cast<uint32_t*>(&V)[tid] = reinterpret_cast<const uint32_t*>(views + p)[tid];
    __syncthreads();
    int n = nlist[p];
    n = n < 0 ? 0 : (n > lcap ? lcap : n);
    const bool from_last = V.mode == ORBP_MODE_LAST_FRAME;
    const bool known_mode = (from_last && src_desc) || V.mode == ORBP_MODE_KEYFRAME;
    if (!known_mode) n = 0;                                            // reported below: such a view sees nothing
    const size_t lb = (size_t)p * lcap, qb = (size_t)p * qcap;
    const float th = V.th;
    int base = 0;                                                      // queries before this tile (uniform)
    for (int i0 = 0; i0 < n; i0 += TPB) {
        const int i = i0 + tid;
        bool vis = false;
        float u = 0.0f, v = 0.0f, angle = 0.0f;
        int level = 0, slot = -1;
        if (i < n) {
            slot = list[lb + i];
            const int octave = src_kps[lb + i].octave;                 // independent of the slot: in flight with the list
            angle = src_kps[lb + i].angle;
            if (!(skip && skip[lb + i]) && slot >= 0 && slot < capacity && live[slot]) {
                const float4* g = reinterpret_cast<const float4*>(geom) + (size_t)slot * 2;
                const float4 g0 = g[0];
                const float P[3] = {g0.x, g0.y, g0.z};
                level = from_last ? octave : predicted_level(V, F, P, g[1].z);
                vis = level >= 0 && level < F.n && project_source(V, P, u, v);
            }
        }
        const unsigned long long m = __ballot(vis);
        if ((tid & 63) == 0) wave_total[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < WAVES; w++) {
            const int c = wave_total[w];
            before += w < wave ? c : 0;
            total += c;
        }
        const int q = before + lane_rank(m);
        if (vis && q < qcap) {
            float* o = qxyr + (qb + q) * 3;
            o[0] = u; o[1] = v; o[2] = th * F.f[level];
            qlev[(qb + q) * 2] = level - 1;
            qlev[(qb + q) * 2 + 1] = level + 1;
            qangle[qb + q] = angle;
            qpos[qb + q] = i;
            const uint4* d = from_last ? reinterpret_cast<const uint4*>(src_desc) + (lb + i) * 2 : reinterpret_cast<const uint4*>(tdesc) + (size_t)slot * 2;
            uint4* od = reinterpret_cast<uint4*>(qdesc) + (qb + q) * 2;
            od[0] = d[0]; od[1] = d[1];
        }
        base += total;
        __syncthreads();                                               // wave_total is rewritten by the next tile
    }
    if (tid == 0) {
        nq[p] = base;
        if (nq_clamped) nq_clamped[p] = base > qcap ? qcap : base;
        overflow[p] = !known_mode ? ORBX_ERR_ARG : (base > qcap ? 1 : 0);
    }
}

__global__ __launch_bounds__(TPB) void k_t2slot(const int32_t* t2q, const int32_t* qpos, const int32_t* list, const int32_t* nt, int cap, int qcap,
                                                int lcap, int32_t* t2slot) {
    const int p = blockIdx.y, idx = blockIdx.x * TPB + threadIdx.x;
    if (idx >= cap) return;
    int out = -1;
    if (idx < nt[p]) {
        const int q = t2q[(size_t)p * cap + idx];
        if (q >= 0 && q < qcap) {
            const int i = qpos[(size_t)p * qcap + q];
            out = list ? list[(size_t)p * lcap + i] : i;
        }
    }
    t2slot[(size_t)p * cap + idx] = out;
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
            slot = list[(size_t)p * lcap + pos];
        }
    }
    t2pos[(size_t)p * cap + idx] = pos;
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
    orbx::DevBuf geom, desc, d_live, d_tab, scratch, one, d_put;
    orbx::PinnedBuf h_tab, h_one, h_put;
    orbx::Stream own;
    orbx::Event chain, tab_done;
    bool chained = false, tab_pending = false;
    // device work on the map is ordered across the callers' streams
    hipError_t begin(hipStream_t st) { return chained ? hipStreamWaitEvent(st, chain, 0) : hipSuccess; }
    hipError_t end(hipStream_t st) {
        const hipError_t e = hipEventRecord(chain, st);
        if (e == hipSuccess) chained = true;
        return e;
    }
};

namespace {

struct DeviceScope {
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    int prev = -1;
    bool ok = false;
};

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

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
        if (m->chained) HIPCHK(m, hipEventSynchronize(m->chain));
        size_t want = std::max<size_t>(4096, m->h_tab.size());
        while (want < (size_t)n * 4) want *= 2;
        HIPCHK(m, m->h_tab.ensure(want, hipHostMallocDefault));
        HIPCHK(m, m->d_tab.ensure(want));
    }
    std::memcpy(m->h_tab.as(), slots, (size_t)n * 4);
    HIPCHK(m, hipMemcpyAsync(m->d_tab.as(), m->h_tab.as(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(m, hipEventRecord(m->tab_done, st));
    m->tab_pending = true;
    return ORBX_OK;
}

int put_locked(orbp_map* m, const int32_t* slots, int n, const float* d_pos, const float* d_normal, const float* d_min, const float* d_max,
               const uint8_t* d_desc, hipStream_t st) {
    HIPCHK(m, m->begin(st));
    const int rc = upload_slots(m, slots, n, st);
    if (rc != ORBX_OK) return rc;
    orbp::k_put<<<(n + orbp::TPB - 1) / orbp::TPB, orbp::TPB, 0, st>>>(n, m->d_tab.as<int32_t>(), d_pos, d_normal, d_min, d_max, d_desc,
                                                                       m->geom.as<float>(), m->desc.as<uint8_t>(), m->d_live.as<uint8_t>());
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, m->end(st));
    for (int i = 0; i < n; i++)
        if (!m->live[slots[i]]) { m->live[slots[i]] = 1; m->n_live++; }
    return ORBX_OK;
}

int fill_factors(const float* factors, int nlevels, orbp::Factors& F) {
    if (!factors || nlevels < 1 || nlevels > ORBS_MAX_LEVELS) return ORBX_ERR_ARG;
    std::memset(&F, 0, sizeof(F));
    for (int i = 0; i < nlevels; i++) F.f[i] = factors[i];
    F.n = nlevels;
    return ORBX_OK;
}

int check_walk(const orbp_map* m, const void* d_views, int nviews, const int32_t* d_list, const int32_t* d_nlist, int lcap, int qcap) {
    if (!m || nviews < 0 || nviews > ORBP_MAX_VIEWS || lcap < 1 || qcap < 1) return ORBX_ERR_ARG;
    if (nviews > 0 && !d_views) return ORBX_ERR_ARG;
    if (d_list ? !d_nlist : lcap < m->capacity) return ORBX_ERR_ARG;
    return ORBX_OK;
}

void launch_project(orbp_map* m, const orbp_view* d_views, int nviews, const orbp::Factors& F, const int32_t* d_list, const int32_t* d_nlist,
                    int lcap, const uint8_t* d_skip, orbp_record* d_rec, float* d_qxyr, int32_t* d_qlev, uint8_t* d_qdesc, int32_t* d_qpos,
                    int32_t* d_nq, int32_t* d_nq_clamped, int32_t* d_overflow, int qcap, hipStream_t st) {
    orbp::k_project<<<nviews, orbp::TPB, 0, st>>>(d_views, F, m->capacity, m->geom.as<float>(), m->desc.as<uint8_t>(), m->d_live.as<uint8_t>(),
                                                  d_list, d_nlist, lcap, d_skip, d_rec, d_qxyr, d_qlev, d_qdesc, d_qpos, d_nq, d_nq_clamped,
                                                  d_overflow, qcap);
}

// the query arrays between projection and search, carved from one buffer
struct Scratch {
    float* qxyr; int32_t* qlev; uint8_t* qdesc; int32_t* qpos; int32_t* nq_clamped; int32_t* q2t; int32_t* t2q;
    float* qangle;                                     // the source-frame searches only (with_angle)
    static size_t bytes(int nviews, int cap, int qcap, bool with_angle = false) {
        const size_t nqc = (size_t)nviews * qcap;
        return al256(nqc * 12) + al256(nqc * 8) + al256(nqc * 32) + al256(nqc * 4) + al256((size_t)nviews * 4) + al256(nqc * 4) +
               al256((size_t)nviews * cap * 4) + (with_angle ? al256(nqc * 4) : 0);
    }
    Scratch(uint8_t* b, int nviews, int cap, int qcap) {
        const size_t nqc = (size_t)nviews * qcap;
        qxyr = (float*)b; b += al256(nqc * 12);
        qlev = (int32_t*)b; b += al256(nqc * 8);
        qdesc = b; b += al256(nqc * 32);
        qpos = (int32_t*)b; b += al256(nqc * 4);
        nq_clamped = (int32_t*)b; b += al256((size_t)nviews * 4);
        q2t = (int32_t*)b; b += al256(nqc * 4);
        t2q = (int32_t*)b; b += al256((size_t)nviews * cap * 4);
        qangle = (float*)b;
    }
};

// grows a handle-owned device buffer; device work that may still read the old one is waited for first
int grow(orbp_map* m, orbx::DevBuf& buf, size_t bytes) {
    if (bytes <= buf.size()) return ORBX_OK;
    if (m->chained) HIPCHK(m, hipEventSynchronize(m->chain));
    HIPCHK(m, buf.ensure(bytes));
    return ORBX_OK;
}

int track_locked(orbp_map* m, const orbp_view* d_views, int nviews, const orbp::Factors& F, const int32_t* d_list, const int32_t* d_nlist, int lcap,
                 const uint8_t* d_skip, const orbf_bounds* b, float ratio, const orbx_keypoint* d_kps_un, const uint8_t* d_desc,
                 const int32_t* d_cell_off, const int32_t* d_cell_feat, const int32_t* d_nt, int cap, const uint8_t* d_claimed, int qcap,
                 orbp_record* d_rec, int32_t* d_t2slot, int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow, uint8_t* scratch, hipStream_t st) {
    const Scratch S(scratch, nviews, cap, qcap);
    HIPCHK(m, m->begin(st));
    launch_project(m, d_views, nviews, F, d_list, d_nlist, lcap, d_skip, d_rec, S.qxyr, S.qlev, S.qdesc, S.qpos, d_nq, S.nq_clamped, d_overflow, qcap, st);
    HIPCHK(m, hipGetLastError());
    const orbs_params prm{ORBS_RULE_MAPPOINTS, ORBS_TH_HIGH, ratio, 0};
    const int rc = orbs_window_search_batch_device(b, &prm, d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap, d_claimed, S.qxyr, S.qlev, S.qdesc,
                                                   nullptr, nullptr, S.nq_clamped, qcap, nviews, S.q2t, S.t2q, nullptr, nullptr, d_nmatches, st);
    if (rc != ORBX_OK) { (void)m->end(st); return rc; }
    orbp::k_t2slot<<<dim3((cap + orbp::TPB - 1) / orbp::TPB, nviews), orbp::TPB, 0, st>>>(S.t2q, S.qpos, d_list, d_nt, cap, qcap, lcap, d_t2slot);
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, m->end(st));
    return ORBX_OK;
}

void launch_project_source(orbp_map* m, const orbp_view* d_views, int nviews, const orbp::Factors& F, const int32_t* d_list, const int32_t* d_nlist,
                           int lcap, const uint8_t* d_skip, const orbx_keypoint* d_src_kps, const uint8_t* d_src_desc, float* d_qxyr, int32_t* d_qlev,
                           uint8_t* d_qdesc, float* d_qangle, int32_t* d_qpos, int32_t* d_nq, int32_t* d_nq_clamped, int32_t* d_overflow, int qcap,
                           hipStream_t st) {
    orbp::k_project_source<<<nviews, orbp::TPB, 0, st>>>(d_views, F, m->capacity, m->geom.as<float>(), m->desc.as<uint8_t>(), m->d_live.as<uint8_t>(),
                                                         d_list, d_nlist, lcap, d_skip, d_src_kps, d_src_desc, d_qxyr, d_qlev, d_qdesc, d_qangle, d_qpos,
                                                         d_nq, d_nq_clamped, d_overflow, qcap);
}

// what the source-frame walks need beyond check_walk: a list (entry i is feature i of the source frame) and its key points
int check_source(const orbp_map* m, const void* d_views, int nviews, const int32_t* d_list, const int32_t* d_nlist, int lcap, int qcap,
                 const void* d_src_kps, const void* d_src_desc) {
    if (!m || nviews < 0 || nviews > ORBP_MAX_VIEWS || lcap < 1 || qcap < 1) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_views || !d_list || !d_nlist || !d_src_kps || ((uintptr_t)d_src_desc & 15)) return ORBX_ERR_ARG;
    return ORBX_OK;
}

int track_source_locked(orbp_map* m, const orbp_view* d_views, int nviews, const orbp::Factors& F, const int32_t* d_list, const int32_t* d_nlist,
                        int lcap, const uint8_t* d_skip, const orbx_keypoint* d_src_kps, const uint8_t* d_src_desc, const orbf_bounds* b,
                        const orbs_params& prm, const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int32_t* d_cell_off,
                        const int32_t* d_cell_feat, const int32_t* d_nt, int cap, const uint8_t* d_claimed, int qcap, int32_t* d_t2pos,
                        int32_t* d_t2slot, int32_t* d_nmatches, int32_t* d_nq, int32_t* d_overflow, uint8_t* scratch, hipStream_t st) {
    const Scratch S(scratch, nviews, cap, qcap);
    HIPCHK(m, m->begin(st));
    launch_project_source(m, d_views, nviews, F, d_list, d_nlist, lcap, d_skip, d_src_kps, d_src_desc, S.qxyr, S.qlev, S.qdesc, S.qangle, S.qpos, d_nq,
                          S.nq_clamped, d_overflow, qcap, st);
    HIPCHK(m, hipGetLastError());
    const int rc = orbs_window_search_batch_device(b, &prm, d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap, d_claimed, S.qxyr, S.qlev, S.qdesc,
                                                   S.qangle, nullptr, S.nq_clamped, qcap, nviews, S.q2t, S.t2q, nullptr, nullptr, d_nmatches, st);
    if (rc != ORBX_OK) { (void)m->end(st); return rc; }
    orbp::k_t2source<<<dim3((cap + orbp::TPB - 1) / orbp::TPB, nviews), orbp::TPB, 0, st>>>(S.t2q, S.qpos, d_list, d_nt, cap, qcap, lcap, d_t2pos,
                                                                                           d_t2slot);
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, m->end(st));
    return ORBX_OK;
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
        m->d_live.ensure((size_t)capacity) != hipSuccess || m->own.ensure() != hipSuccess || m->chain.ensure() != hipSuccess ||
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
    if (m->chained) (void)hipEventSynchronize(m->chain);      // the last piece of device work on the map
    if (m->tab_pending) (void)hipEventSynchronize(m->tab_done);
    delete m;
}

int orbp_capacity(const orbp_map* m) { return m ? m->capacity : 0; }
int orbp_size(const orbp_map* m) { return m ? m->n_live : 0; }

int orbp_clear(orbp_map* m) {
    if (!m) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lk(m->mu);
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = m->own;
    HIPCHK(m, m->begin(st));
    HIPCHK(m, hipMemsetAsync(m->d_live.as(), 0, (size_t)m->capacity, st));
    HIPCHK(m, m->end(st));
    HIPCHK(m, hipStreamSynchronize(st));
    std::fill(m->live.begin(), m->live.end(), 0);
    m->n_live = 0;
    return ORBX_OK;
}

int orbp_put_device(orbp_map* m, const int32_t* slots, int n, const float* d_pos, const float* d_normal, const float* d_min_dist,
                    const float* d_max_dist, const uint8_t* d_desc, void* stream) {
    if (!m || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!slots || !d_pos || !d_normal || !d_min_dist || !d_max_dist) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lk(m->mu);
    if (check_slots(m, slots, n, true, d_desc == nullptr) != ORBX_OK) return ORBX_ERR_ARG;
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    return put_locked(m, slots, n, d_pos, d_normal, d_min_dist, d_max_dist, d_desc, stream ? (hipStream_t)stream : (hipStream_t)m->own);
}

int orbp_put(orbp_map* m, const int32_t* slots, int n, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
             const uint8_t* desc) {
    if (!m || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!slots || !pos || !normal || !min_dist || !max_dist) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lk(m->mu);
    if (check_slots(m, slots, n, true, desc == nullptr) != ORBX_OK) return ORBX_ERR_ARG;
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    // staged through the handle's pinned block (grown by doubling, kept): one copy up, no allocation in the steady state
    const size_t o_nrm = al256((size_t)n * 12), o_min = o_nrm + al256((size_t)n * 12), o_max = o_min + al256((size_t)n * 4);
    const size_t o_desc = o_max + al256((size_t)n * 4), total = o_desc + (desc ? al256((size_t)n * 32) : 0);
    hipStream_t st = m->own;
    if (m->h_put.size() < total) {
        if (m->chained) HIPCHK(m, hipEventSynchronize(m->chain));
        size_t want = std::max<size_t>(4096, m->h_put.size());
        while (want < total) want *= 2;
        HIPCHK(m, m->h_put.ensure(want, hipHostMallocDefault));
        HIPCHK(m, m->d_put.ensure(want));
    }
    uint8_t* h = m->h_put.as<uint8_t>();
    uint8_t* d = m->d_put.as<uint8_t>();
    std::memcpy(h, pos, (size_t)n * 12);
    std::memcpy(h + o_nrm, normal, (size_t)n * 12);
    std::memcpy(h + o_min, min_dist, (size_t)n * 4);
    std::memcpy(h + o_max, max_dist, (size_t)n * 4);
    if (desc) std::memcpy(h + o_desc, desc, (size_t)n * 32);
    HIPCHK(m, m->begin(st));
    HIPCHK(m, hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, st));
    const int rc = put_locked(m, slots, n, reinterpret_cast<const float*>(d), reinterpret_cast<const float*>(d + o_nrm),
                              reinterpret_cast<const float*>(d + o_min), reinterpret_cast<const float*>(d + o_max), desc ? d + o_desc : nullptr, st);
    if (rc != ORBX_OK) return rc;
    HIPCHK(m, hipStreamSynchronize(st));
    return ORBX_OK;
}

int orbp_erase(orbp_map* m, const int32_t* slots, int n) {
    if (!m || n < 0) return ORBX_ERR_ARG;
    if (n == 0) return ORBX_OK;
    if (!slots) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lk(m->mu);
    if (check_slots(m, slots, n, false, false) != ORBX_OK) return ORBX_ERR_ARG;
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = m->own;
    HIPCHK(m, m->begin(st));
    const int rc = upload_slots(m, slots, n, st);
    if (rc != ORBX_OK) return rc;
    orbp::k_erase<<<(n + orbp::TPB - 1) / orbp::TPB, orbp::TPB, 0, st>>>(n, m->d_tab.as<int32_t>(), m->d_live.as<uint8_t>());
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, m->end(st));
    HIPCHK(m, hipStreamSynchronize(st));
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
    if (m->chained) HIPCHK(m, hipEventSynchronize(m->chain));
    float g[8];
    HIPCHK(m, hipMemcpy(g, m->geom.as<float>() + (size_t)slot * 8, 32, hipMemcpyDeviceToHost));
    HIPCHK(m, hipMemcpy(desc, m->desc.as<uint8_t>() + (size_t)slot * 32, 32, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) { pos[k] = g[k]; normal[k] = g[3 + k]; }
    *min_dist = g[6];
    *max_dist = g[7];
    return ORBX_OK;
}

int orbp_project_batch_device(orbp_map* m, const orbp_view* d_views, int nviews, const float* factors, int nlevels, const int32_t* d_list,
                              const int32_t* d_nlist, int lcap, const uint8_t* d_skip, orbp_record* d_rec, float* d_qxyr, int32_t* d_qlev,
                              uint8_t* d_qdesc, int32_t* d_qpos, int32_t* d_nq, int32_t* d_overflow, int qcap, void* stream) {
    orbp::Factors F;
    if (check_walk(m, d_views, nviews, d_list, d_nlist, lcap, qcap) != ORBX_OK || fill_factors(factors, nlevels, F) != ORBX_OK) return ORBX_ERR_ARG;
    if (nviews == 0) return ORBX_OK;
    if (!d_qxyr || !d_qlev || !d_qdesc || !d_qpos || !d_nq || !d_overflow) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lk(m->mu);
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)m->own;
    HIPCHK(m, m->begin(st));
    launch_project(m, d_views, nviews, F, d_list, d_nlist, lcap, d_skip, d_rec, d_qxyr, d_qlev, d_qdesc, d_qpos, d_nq, nullptr, d_overflow, qcap, st);
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, m->end(st));
    return ORBX_OK;
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
    if (orbs_lds_bytes(cap, qcap) > 160 * 1024) return ORBX_ERR_CAPACITY;
    std::lock_guard<std::mutex> lk(m->mu);
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    const int rc = grow(m, m->scratch, Scratch::bytes(nviews, cap, qcap));
    if (rc != ORBX_OK) return rc;
    return track_locked(m, d_views, nviews, F, d_list, d_nlist, lcap, d_skip, b, ratio, d_kps_un, d_desc, d_cell_off, d_cell_feat, d_nt, cap, d_claimed,
                        qcap, d_rec, d_t2slot, d_nmatches, d_nq, d_overflow, m->scratch.as<uint8_t>(), stream ? (hipStream_t)stream : (hipStream_t)m->own);
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
    const int cap = std::max(nt, 1), lcap = std::max(nlist, 1);
    if (orbs_lds_bytes(cap, qcap) > 160 * 1024) return ORBX_ERR_CAPACITY;
    std::lock_guard<std::mutex> lk(m->mu);
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)m->own;
    // one pinned block up, one down: [view | nt | list | skip | frame (host form)] and [nq, overflow, nmatches | t2slot | rec]
    size_t o = 0;
    const size_t o_view = o; o += al256(sizeof(orbp_view));
    const size_t o_nt = o; o += 256;                                   // nt, nlist
    const size_t o_list = o; o += list ? al256((size_t)lcap * 4) : 0;
    const size_t o_skip = o; o += skip ? al256((size_t)lcap) : 0;
    const bool up_frame = !frame_on_device;
    const size_t o_kps = o; o += up_frame ? al256((size_t)cap * sizeof(orbx_keypoint)) : 0;
    const size_t o_desc = o; o += up_frame ? al256((size_t)cap * 32) : 0;
    const size_t o_coff = o; o += up_frame ? al256((size_t)(ORBF_GRID_CELLS + 1) * 4) : 0;
    const size_t o_cfeat = o; o += up_frame ? al256((size_t)cap * 4) : 0;
    const size_t o_claim = o; o += up_frame && claimed ? al256((size_t)cap) : 0;
    const size_t up_bytes = o;
    const size_t o_cnt = o; o += 256;                                  // nq, overflow, nmatches
    const size_t o_t2s = o; o += al256((size_t)cap * 4);
    const size_t o_rec = o; o += rec ? al256((size_t)lcap * sizeof(orbp_record)) : 0;
    const size_t io_bytes = o;
    const size_t total = io_bytes + Scratch::bytes(1, cap, qcap);
    if (m->h_one.size() < io_bytes) {
        if (m->chained) HIPCHK(m, hipEventSynchronize(m->chain));
        HIPCHK(m, m->h_one.ensure(io_bytes + io_bytes / 2, hipHostMallocDefault));
    }
    int rc = grow(m, m->one, total + total / 2);
    if (rc != ORBX_OK) return rc;
    uint8_t* h = m->h_one.as<uint8_t>();
    uint8_t* d = m->one.as<uint8_t>();
    std::memcpy(h + o_view, view, sizeof(orbp_view));
    reinterpret_cast<int32_t*>(h + o_nt)[0] = nt;
    reinterpret_cast<int32_t*>(h + o_nt)[1] = nlist;
    if (list) std::memcpy(h + o_list, list, (size_t)nlist * 4);
    if (skip) std::memcpy(h + o_skip, skip, (size_t)nlist);
    if (up_frame) {
        std::memcpy(h + o_kps, kps_un, (size_t)nt * sizeof(orbx_keypoint));
        std::memcpy(h + o_desc, desc, (size_t)nt * 32);
        std::memcpy(h + o_coff, cell_off, (size_t)(ORBF_GRID_CELLS + 1) * 4);
        std::memcpy(h + o_cfeat, cell_feat, (size_t)nt * 4);
        if (claimed) std::memcpy(h + o_claim, claimed, (size_t)nt);
    }
    HIPCHK(m, m->begin(st));
    HIPCHK(m, hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    int32_t* d_cnt = reinterpret_cast<int32_t*>(d + o_cnt);
    rc = track_locked(m, reinterpret_cast<const orbp_view*>(d + o_view), 1, F, list ? reinterpret_cast<const int32_t*>(d + o_list) : nullptr,
                      reinterpret_cast<const int32_t*>(d + o_nt) + 1, lcap, skip ? d + o_skip : nullptr, b, ratio,
                      up_frame ? reinterpret_cast<const orbx_keypoint*>(d + o_kps) : kps_un, up_frame ? d + o_desc : desc,
                      up_frame ? reinterpret_cast<const int32_t*>(d + o_coff) : cell_off, up_frame ? reinterpret_cast<const int32_t*>(d + o_cfeat) : cell_feat,
                      reinterpret_cast<const int32_t*>(d + o_nt), cap, up_frame ? (claimed ? d + o_claim : nullptr) : claimed, qcap,
                      rec ? reinterpret_cast<orbp_record*>(d + o_rec) : nullptr, reinterpret_cast<int32_t*>(d + o_t2s), d_cnt + 2, d_cnt, d_cnt + 1,
                      d + io_bytes, st);
    if (rc != ORBX_OK) return rc;
    HIPCHK(m, hipMemcpyAsync(h + o_cnt, d + o_cnt, io_bytes - o_cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(m, m->end(st));
    HIPCHK(m, hipStreamSynchronize(st));
    const int32_t* cnt = reinterpret_cast<const int32_t*>(h + o_cnt);
    if (nvisible) *nvisible = cnt[0];
    if (cnt[1]) return ORBX_ERR_CAPACITY;
    *nmatches = cnt[2];
    if (nt > 0) std::memcpy(t2slot, h + o_t2s, (size_t)nt * 4);
    if (rec && nlist > 0) std::memcpy(rec, h + o_rec, (size_t)nlist * sizeof(orbp_record));
    return ORBX_OK;
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
    std::lock_guard<std::mutex> lk(m->mu);
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)m->own;
    HIPCHK(m, m->begin(st));
    launch_project_source(m, d_views, nviews, F, d_list, d_nlist, lcap, d_skip, d_src_kps, d_src_desc, d_qxyr, d_qlev, d_qdesc, d_qangle, d_qpos, d_nq,
                          nullptr, d_overflow, qcap, st);
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, m->end(st));
    return ORBX_OK;
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
    if (orbs_lds_bytes(cap, qcap) > 160 * 1024) return ORBX_ERR_CAPACITY;
    std::lock_guard<std::mutex> lk(m->mu);
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    const int rc = grow(m, m->scratch, Scratch::bytes(nviews, cap, qcap, true));
    if (rc != ORBX_OK) return rc;
    return track_source_locked(m, d_views, nviews, F, d_list, d_nlist, lcap, d_skip, d_src_kps, d_src_desc, b, *prm, d_kps_un, d_desc, d_cell_off,
                               d_cell_feat, d_nt, cap, d_claimed, qcap, d_t2pos, d_t2slot, d_nmatches, d_nq, d_overflow, m->scratch.as<uint8_t>(),
                               stream ? (hipStream_t)stream : (hipStream_t)m->own);
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
    const int cap = std::max(nt, 1), lcap = std::max(nlist, 1);
    if (orbs_lds_bytes(cap, qcap) > 160 * 1024) return ORBX_ERR_CAPACITY;
    std::lock_guard<std::mutex> lk(m->mu);
    DeviceScope ds(m->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : (hipStream_t)m->own;
    // one pinned block up, one down: [view | nt, nlist | list | skip | source frame (host form) | frame (host form)] and
    // [nq, overflow, nmatches | t2pos | t2slot]
    const bool up_src = !src_on_device && nlist > 0, up_src_desc = up_src && from_last, up_frame = !frame_on_device;
    size_t o = 0;
    const size_t o_view = o; o += al256(sizeof(orbp_view));
    const size_t o_nt = o; o += 256;                                   // nt, nlist
    const size_t o_list = o; o += al256((size_t)lcap * 4);
    const size_t o_skip = o; o += skip ? al256((size_t)lcap) : 0;
    const size_t o_skps = o; o += up_src ? al256((size_t)lcap * sizeof(orbx_keypoint)) : 0;
    const size_t o_sdesc = o; o += up_src_desc ? al256((size_t)lcap * 32) : 0;
    const size_t o_kps = o; o += up_frame ? al256((size_t)cap * sizeof(orbx_keypoint)) : 0;
    const size_t o_desc = o; o += up_frame ? al256((size_t)cap * 32) : 0;
    const size_t o_coff = o; o += up_frame ? al256((size_t)(ORBF_GRID_CELLS + 1) * 4) : 0;
    const size_t o_cfeat = o; o += up_frame ? al256((size_t)cap * 4) : 0;
    const size_t o_claim = o; o += up_frame && claimed ? al256((size_t)cap) : 0;
    const size_t up_bytes = o;
    const size_t o_cnt = o; o += 256;                                  // nq, overflow, nmatches
    const size_t o_t2p = o; o += al256((size_t)cap * 4);
    const size_t o_t2s = o; o += t2slot ? al256((size_t)cap * 4) : 0;
    const size_t io_bytes = o;
    const size_t total = io_bytes + Scratch::bytes(1, cap, qcap, true);
    if (m->h_one.size() < io_bytes) {
        if (m->chained) HIPCHK(m, hipEventSynchronize(m->chain));
        HIPCHK(m, m->h_one.ensure(io_bytes + io_bytes / 2, hipHostMallocDefault));
    }
    int rc = grow(m, m->one, total + total / 2);
    if (rc != ORBX_OK) return rc;
    uint8_t* h = m->h_one.as<uint8_t>();
    uint8_t* d = m->one.as<uint8_t>();
    std::memcpy(h + o_view, view, sizeof(orbp_view));
    reinterpret_cast<int32_t*>(h + o_nt)[0] = nt;
    reinterpret_cast<int32_t*>(h + o_nt)[1] = nlist;
    if (nlist > 0) std::memcpy(h + o_list, list, (size_t)nlist * 4);
    if (skip && nlist > 0) std::memcpy(h + o_skip, skip, (size_t)nlist);
    if (up_src) std::memcpy(h + o_skps, src_kps, (size_t)nlist * sizeof(orbx_keypoint));
    if (up_src_desc) std::memcpy(h + o_sdesc, src_desc, (size_t)nlist * 32);
    if (up_frame) {
        std::memcpy(h + o_kps, kps_un, (size_t)nt * sizeof(orbx_keypoint));
        std::memcpy(h + o_desc, desc, (size_t)nt * 32);
        std::memcpy(h + o_coff, cell_off, (size_t)(ORBF_GRID_CELLS + 1) * 4);
        std::memcpy(h + o_cfeat, cell_feat, (size_t)nt * 4);
        if (claimed) std::memcpy(h + o_claim, claimed, (size_t)nt);
    }
    HIPCHK(m, m->begin(st));
    HIPCHK(m, hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
    int32_t* d_cnt = reinterpret_cast<int32_t*>(d + o_cnt);
    // with nlist == 0 nothing is read through the source pointers; the kernel still wants them non-NULL for a last-frame view
    const orbx_keypoint* d_skps = up_src ? reinterpret_cast<const orbx_keypoint*>(d + o_skps) : (nlist > 0 ? src_kps : reinterpret_cast<const orbx_keypoint*>(d));
    const uint8_t* d_sdesc = up_src_desc ? d + o_sdesc : (nlist > 0 ? src_desc : d);
    rc = track_source_locked(m, reinterpret_cast<const orbp_view*>(d + o_view), 1, F, reinterpret_cast<const int32_t*>(d + o_list),
                             reinterpret_cast<const int32_t*>(d + o_nt) + 1, lcap, skip ? d + o_skip : nullptr, d_skps, d_sdesc, b, *prm,
                             up_frame ? reinterpret_cast<const orbx_keypoint*>(d + o_kps) : kps_un, up_frame ? d + o_desc : desc,
                             up_frame ? reinterpret_cast<const int32_t*>(d + o_coff) : cell_off,
                             up_frame ? reinterpret_cast<const int32_t*>(d + o_cfeat) : cell_feat, reinterpret_cast<const int32_t*>(d + o_nt), cap,
                             up_frame ? (claimed ? d + o_claim : nullptr) : claimed, qcap, reinterpret_cast<int32_t*>(d + o_t2p),
                             t2slot ? reinterpret_cast<int32_t*>(d + o_t2s) : nullptr, d_cnt + 2, d_cnt, d_cnt + 1, d + io_bytes, st);
    if (rc != ORBX_OK) return rc;
    HIPCHK(m, hipMemcpyAsync(h + o_cnt, d + o_cnt, io_bytes - o_cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(m, m->end(st));
    HIPCHK(m, hipStreamSynchronize(st));
    const int32_t* cnt = reinterpret_cast<const int32_t*>(h + o_cnt);
    if (nvisible) *nvisible = cnt[0];
    if (cnt[1]) return ORBX_ERR_CAPACITY;
    *nmatches = cnt[2];
    if (nt > 0) {
        std::memcpy(t2pos, h + o_t2p, (size_t)nt * 4);
        if (t2slot) std::memcpy(t2slot, h + o_t2s, (size_t)nt * 4);
    }
    return ORBX_OK;
}

}  // extern "C"
