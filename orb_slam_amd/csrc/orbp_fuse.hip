// The search of ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th) (reference src/ORBmatcher.cc:1016-1134) on gfx950, for every call of
// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:373-450) in one launch, over the map-point table of orbp_project.hip and key frames in
// the batch layout.  include/orbp.h is the boundary and states the arithmetic and the statuses (ORBP_MODE_FUSE); the host side lives in
// orbp_project.hip.
//
// k_fuse: a flat grid over (view, list entry), one lane per entry, 256 lanes per workgroup.  Nothing couples two entries: no claim, no
//   second distance, no ratio, no rotation histogram, no order.  So there is no compaction, no per-problem staging and no commit, and a long
//   list of one view spreads over as many workgroups as it has tiles (the one-workgroup walk of k_project is a serial chain of tiles there).
//   A lane runs the five tests on its point (orbp::entry_test of orbp_device.h, the statement k_loop_test shares), opens the cell window
//   (orbf::window_cells) and scans it column by column (orbp::scan_window of orbp_device.h, the statement k_sim3 shares).  The point's descriptor
//   sits in eight registers, a candidate's arrives as two 16-byte loads; a strictly smaller distance replaces the best.
//   The stage is a chain of dependent loads (list -> live -> geometry -> cell offsets -> cell features -> key point -> descriptor) with a
//   handful of candidates at its end; what hides it is the number of entries in flight.  LDS holds the view only, and the one barrier is
//   the one behind staging it.  Plain vector stores, no atomics: every entry owns its outputs.
#include <hip/hip_runtime.h>

#include <climits>

#include "orbp.h"
#include "orbp_device.h"
#include "orbp_host.h"

namespace orbp {

constexpr int FU_TPB = 256;

__global__ __launch_bounds__(FU_TPB) void k_fuse(Fuse a, Factors F) {
    __shared__ orbp_view V;
    const int p = a.p0 + (int)blockIdx.y, tid = threadIdx.x;
    const Lists& L = a.L;
    const int n = clamped_count(L, p);
    const int i0 = (int)blockIdx.x * FU_TPB;
    if (i0 >= n) return;                                               // uniform: before the barrier
    stage_view(V, a.views, p);
    __syncthreads();
    const int i = i0 + tid;
    if (i >= n) return;
    const size_t e = (size_t)p * L.lcap + i;
    const int fr = a.K.frame ? a.K.frame[p] : p;
    const bool known = V.mode == ORBP_MODE_FUSE && fr >= 0 && fr < a.K.nframes;

    int status = ORBP_FUSE_SKIPPED, level = 0, best = INT_MAX, best_f = -1;
    float u = 0.0f, v = 0.0f;
    do {
        if (!known || (L.skip && L.skip[e])) break;
        const int slot = L.list[e];
        if (slot < 0 || slot >= a.T.capacity || !a.T.live[slot]) break;
        const float4* g = reinterpret_cast<const float4*>(a.T.geom) + (size_t)slot * 2;
        status = entry_test(V, F, g[0], g[1], ORBP_FUSE_EMPTY, u, v, level);
        if (status != ORBP_FUSE_EMPTY) break;
        const float radius = V.th * F.f[level];
        scan_window(a.b, a.K, fr, reinterpret_cast<const uint4*>(a.T.tdesc) + (size_t)slot * 2, u, v, radius, level, best, best_f);
        if (best_f < 0) break;
        status = best <= a.orb_dist ? ORBP_FUSE_FUSED : ORBP_FUSE_FAR;
    } while (false);

    a.out.best_idx[e] = status == ORBP_FUSE_FUSED ? best_f : -1;
    a.out.best_dist[e] = best;
    if (a.out.rec) {
        orbp_fused r;
        r.u = u; r.v = v; r.level = level; r.status = status;
        a.out.rec[e] = r;
    }
}

hipError_t launch_fuse(const Fuse& a, int nviews, const Factors& F, hipStream_t st) {
    const int tiles = (a.L.lcap + FU_TPB - 1) / FU_TPB;
    return for_view_chunks(nviews, [&](int p0, int np) {
        Fuse b = a;
        b.p0 = p0;
        k_fuse<<<dim3(tiles, np), FU_TPB, 0, st>>>(b, F);
        return hipGetLastError();
    });
}

}  // namespace orbp
