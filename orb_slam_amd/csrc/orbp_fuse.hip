// The search of ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th) (reference src/ORBmatcher.cc:1016-1134) on gfx950, for every call of
// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:373-450) in one launch, over the map-point table of orbp_project.hip and key frames in
// the batch layout.  include/orbp.h is the boundary and states the arithmetic and the statuses (ORBP_MODE_FUSE); the host side lives in
// orbp_project.hip.
//
// k_fuse: a flat grid over (view, list entry), one lane per entry, 256 lanes per workgroup.  Nothing couples two entries: no claim, no
//   second distance, no ratio, no rotation histogram, no order.  So there is no compaction, no per-problem staging and no commit, and a long
//   list of one view spreads over as many workgroups as it has tiles (the one-workgroup walk of k_project is a serial chain of tiles there).
//   A lane runs the five tests on its point (orbp::entry_test of orbp_device.h, the statement k_loop_test shares), opens the cell window
//   (orbf::window_cells) and scans it column by column: the cells of one grid column are neighbours in the CSR, so a column is one run
//   cell_off[ix*48 + y0] .. cell_off[ix*48 + y1 + 1] in the reference's order.  The point's descriptor sits in eight registers, a candidate's
//   arrives as two 16-byte loads; a strictly smaller distance replaces the best.
//   The stage is a chain of dependent loads (list -> live -> geometry -> cell offsets -> cell features -> key point -> descriptor) with a
//   handful of candidates at its end; what hides it is the number of entries in flight.  LDS holds the view only, and the one barrier is
//   the one behind staging it.  Plain vector stores, no atomics: every entry owns its outputs.
#include <hip/hip_runtime.h>

#include <climits>

#include "orbf_math.h"
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
        int x0, x1, y0, y1;
        if (!orbf::window_cells(a.b, u, v, radius, &x0, &x1, &y0, &y1)) break;
        int nt = a.K.nt[fr];
        nt = nt < 0 ? 0 : (nt > a.K.cap ? a.K.cap : nt);
        const size_t fb = (size_t)fr * a.K.cap;
        const int32_t* off = a.K.cell_off + (size_t)fr * (ORBF_GRID_CELLS + 1);
        const int32_t* feat = a.K.cell_feat + fb;
        const orbx_keypoint* kps = a.K.kps_un + fb;
        const uint4* kd = reinterpret_cast<const uint4*>(a.K.desc) + fb * 2;
        const uint4* td = reinterpret_cast<const uint4*>(a.T.tdesc) + (size_t)slot * 2;
        const uint4 qa = td[0], qb = td[1];
        const uint32_t q0 = qa.x, q1 = qa.y, q2 = qa.z, q3 = qa.w, q4 = qb.x, q5 = qb.y, q6 = qb.z, q7 = qb.w;
        for (int ix = x0; ix <= x1; ix++) {
            int j = off[ix * ORBF_GRID_ROWS + y0], jend = off[ix * ORBF_GRID_ROWS + y1 + 1];
            j = j < 0 ? 0 : j;                                         // a grid that breaks its contract reads nothing outside the row
            jend = jend > nt ? nt : jend;
            for (; j < jend; j++) {
                const int f = feat[j];
                if ((unsigned)f >= (unsigned)nt) continue;
                const orbx_keypoint kp = kps[f];
                if (fabsf(kp.x - u) > radius || fabsf(kp.y - v) > radius || kp.octave < level - 1 || kp.octave > level) continue;
                const uint4 ca = kd[(size_t)f * 2], cb = kd[(size_t)f * 2 + 1];
                const int d = __popc(q0 ^ ca.x) + __popc(q1 ^ ca.y) + __popc(q2 ^ ca.z) + __popc(q3 ^ ca.w) + __popc(q4 ^ cb.x) + __popc(q5 ^ cb.y) +
                              __popc(q6 ^ cb.z) + __popc(q7 ^ cb.w);
                if (d < best) { best = d; best_f = f; }
            }
        }
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
