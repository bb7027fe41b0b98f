// The projection of ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>& vpMatched, int th)
// (reference src/ORBmatcher.cc:286-407, LoopClosing's search once a Sim3 is accepted) on gfx950, over the map-point table of orbp_project.hip.
// include/orbp.h is the boundary and states the arithmetic and the statuses (ORBP_MODE_LOOP); the host side lives in orbp_project.hip.
//
// The call this serves is one view with several thousand list entries, whose queries must come out in list order: the window search behind it
// lets a match claim its feature.  k_project walks such a list as a serial chain of 256-entry tiles in one workgroup; here the list is flat over
// (view, tile), and the order is restored by counting, in two launches that only the stream orders:
//   k_loop_test   one lane per entry, 256 per workgroup: the five tests of ORBP_MODE_FUSE (orbp::entry_test of orbp_device.h, the statement
//                 k_fuse calls too), the entry's record, and the tile's number of passing entries (ballot, the four wave totals meet in LDS)
//                 in the tile's own word.
//   k_loop_pack   the same grid: a workgroup adds the words of the tiles in front of it in its view, ranks its passing entries in list order
//                 again (orbx::tile_rank) and writes window, levels, list position and descriptor at base + rank while that is below qcap.  The
//                 view's last tile writes the view's counts.
// No atomics, no flags, no spin, no hand-off between workgroups inside a launch: every output word has one writer and is a plain vector store.
//   k_loop_gather (only when views name their key frame's row through d_frame) copies each view's row into the per-view layout the window search
//                 reads.
#include <hip/hip_runtime.h>

#include "orbp.h"
#include "orbp_device.h"
#include "orbp_host.h"

namespace orbp {

constexpr int LP_TPB = LOOP_TILE;
constexpr int LP_WAVES = LP_TPB / 64;

// a view of another mode, or one whose key frame is not there, sees nothing
__device__ __forceinline__ bool loop_view_known(const Loop& a, int p, int mode) {
    if (mode != ORBP_MODE_LOOP) return false;
    if (a.nframes == 0) return true;
    const int fr = a.frame ? a.frame[p] : p;
    return fr >= 0 && fr < a.nframes;
}

__global__ __launch_bounds__(LP_TPB) void k_loop_test(Loop a, Factors F) {
    __shared__ orbp_view V;
    __shared__ int wave_total[LP_WAVES];
    const int p = a.p0 + (int)blockIdx.y, tid = threadIdx.x;
    const Lists& L = a.L;
    const int n = clamped_count(L, p);
    const int i0 = (int)blockIdx.x * LP_TPB;
    if (i0 >= n) return;                                               // uniform: before the barrier
    stage_view(V, a.views, p);
    __syncthreads();
    const int i = i0 + tid;
    const size_t e = (size_t)p * L.lcap + i;
    const bool known = loop_view_known(a, p, V.mode);

    int status = ORBP_FUSE_SKIPPED, level = 0;
    float u = 0.0f, v = 0.0f;
    do {
        if (i >= n || !known || (L.skip && L.skip[e])) break;
        const int slot = L.list[e];
        if (slot < 0 || slot >= a.T.capacity || !a.T.live[slot]) break;
        const float4* g = reinterpret_cast<const float4*>(a.T.geom) + (size_t)slot * 2;
        status = entry_test(V, F, g[0], g[1], ORBP_LOOP_QUERY, u, v, level);
    } while (false);

    if (i < n) {
        orbp_fused r;
        r.u = u; r.v = v; r.level = level; r.status = status;
        a.rec[e] = r;
    }
    const unsigned long long m = __ballot(status == ORBP_LOOP_QUERY);
    if ((tid & 63) == 0) wave_total[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int w = 0; w < LP_WAVES; w++) c += wave_total[w];
        a.tile_count[(size_t)p * gridDim.x + blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(LP_TPB) void k_loop_pack(Loop a, Factors F) {
    __shared__ int wave_total[LP_WAVES];
    const int p = a.p0 + (int)blockIdx.y, tid = threadIdx.x, t = (int)blockIdx.x;
    const Lists& L = a.L;
    const int n = clamped_count(L, p);
    const int last = n > 0 ? (n - 1) / LP_TPB : 0;                      // an empty list: tile 0 reports the view
    if (t > last) return;                                              // uniform: before the barriers
    // the passing entries of the tiles in front of this one: k_loop_test wrote every one of those words (their tiles start below n)
    int part = 0;
    for (int j = tid; j < t; j += LP_TPB) part += a.tile_count[(size_t)p * gridDim.x + j];
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if ((tid & 63) == 0) wave_total[tid >> 6] = part;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < LP_WAVES; w++) base += wave_total[w];
    __syncthreads();                                                   // tile_rank rewrites wave_total

    const int i = t * LP_TPB + tid;
    const size_t e = (size_t)p * L.lcap + i;
    bool keep = false;
    int slot = -1;
    orbp_fused r{};
    if (i < n) {
        r = a.rec[e];
        slot = L.list[e];
        keep = r.status == ORBP_LOOP_QUERY && slot >= 0 && slot < a.T.capacity && r.level >= 0 && r.level < F.n;
    }
    const int q = orbx::tile_rank<LP_WAVES>(keep, wave_total, base);    // base: now through this tile
    if (keep && q < a.qcap) {
        const size_t o = (size_t)p * a.qcap + q;
        float* xyr = a.Q.qxyr + o * 3;
        xyr[0] = r.u; xyr[1] = r.v; xyr[2] = a.views[p].th * F.f[r.level];
        a.Q.qlev[o * 2] = r.level - 1;
        a.Q.qlev[o * 2 + 1] = r.level;
        a.Q.qpos[o] = i;
        const uint4* d = reinterpret_cast<const uint4*>(a.T.tdesc) + (size_t)slot * 2;
        uint4* od = reinterpret_cast<uint4*>(a.Q.qdesc) + o * 2;
        od[0] = d[0]; od[1] = d[1];
    }
    if (t == last && tid == 0) {
        const bool known = loop_view_known(a, p, a.views[p].mode);
        a.nq[p] = base;
        if (a.Q.nq_clamped) a.Q.nq_clamped[p] = base > a.qcap ? a.qcap : base;
        a.overflow[p] = !known ? ORBX_ERR_ARG : (base > a.qcap ? 1 : 0);
    }
}

__global__ __launch_bounds__(LP_TPB) void k_loop_gather(LoopGather g) {
    const int p = g.p0 + (int)blockIdx.y, j = (int)blockIdx.x * LP_TPB + (int)threadIdx.x;
    const FuseFrames& K = g.K;
    const int fr = K.frame ? K.frame[p] : p;
    const bool ok = fr >= 0 && fr < K.nframes;
    if (ok && j < K.cap) {
        const size_t s = (size_t)fr * K.cap + j, o = (size_t)p * K.cap + j;
        g.kps[o] = K.kps_un[s];
        g.cell_feat[o] = K.cell_feat[s];
        const uint4* sd = reinterpret_cast<const uint4*>(K.desc) + s * 2;
        uint4* od = reinterpret_cast<uint4*>(g.desc) + o * 2;
        od[0] = sd[0]; od[1] = sd[1];
    }
    if (j <= ORBF_GRID_CELLS) g.cell_off[(size_t)p * (ORBF_GRID_CELLS + 1) + j] = ok ? K.cell_off[(size_t)fr * (ORBF_GRID_CELLS + 1) + j] : 0;
    if (j == 0) g.nt[p] = ok ? K.nt[fr] : 0;
}

hipError_t launch_loop_project(const Loop& a, int nviews, const Factors& F, hipStream_t st) {
    const int tiles = loop_tiles(a.L.lcap);
    return for_view_chunks(nviews, [&](int p0, int np) {
        Loop b = a;
        b.p0 = p0;
        k_loop_test<<<dim3(tiles, np), LP_TPB, 0, st>>>(b, F);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        k_loop_pack<<<dim3(tiles, np), LP_TPB, 0, st>>>(b, F);
        return hipGetLastError();
    });
}

hipError_t launch_loop_gather(const LoopGather& g, int nviews, hipStream_t st) {
    const int most = g.K.cap > ORBF_GRID_CELLS + 1 ? g.K.cap : ORBF_GRID_CELLS + 1;
    return for_view_chunks(nviews, [&](int p0, int np) {
        LoopGather b = g;
        b.p0 = p0;
        k_loop_gather<<<dim3((most + LP_TPB - 1) / LP_TPB, np), LP_TPB, 0, st>>>(b);
        return hipGetLastError();
    });
}

}  // namespace orbp
