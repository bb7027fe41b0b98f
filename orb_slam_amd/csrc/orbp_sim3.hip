// ORBmatcher::SearchBySim3(KeyFrame*, KeyFrame*, vector<MapPoint*>&, s12, R12, t12, th) (reference src/ORBmatcher.cc:1267-1505, LoopClosing::ComputeSim3's
// search for every candidate whose RANSAC converged) on gfx950, over the map-point table of orbp_project.hip and key frames in the batch layout.
// include/orbp.h is the boundary and states the arithmetic and the statuses (ORBP_MODE_SIM3); the host side lives in orbp_project.hip.
//
// k_sim3: k_fuse's shape (orbp_fuse.hip).  A flat grid over (direction row, 256-entry tile), one lane per entry; row 2p is direction 1 -> 2 of pair p
//   and row 2p + 1 direction 2 -> 1, so both directions of every pair are ONE launch: the stage is the same chain of dependent loads (list -> live
//   -> geometry -> cell offsets -> cell features -> key point -> descriptor), and what hides it is the number of entries in flight.  LDS holds
//   the row's direction record only (144 bytes, read at one address by every lane); the one barrier is the one behind staging it.  A lane runs
//   orbp::entry_test_sim3 and orbp::scan_window of orbp_device.h, the latter the statement k_fuse calls.  Plain vector stores: every entry owns
//   its outputs.  Tile 0 of a pair's first row also zeroes the pair's count, which only the next launch adds to.
// k_sim3_agree: the agreement (:1486-1502), a second launch behind it on the same stream, flat over (pair, 256 entries of direction 1 -> 2).  A lane
//   follows its vnMatch1 into direction 2 -> 1's row; a wave counts its agreed entries by ballot and adds them to the pair's count with one integer
//   atomic, whose result does not depend on the order.
#include <hip/hip_runtime.h>

#include <climits>

#include "orbp.h"
#include "orbp_device.h"
#include "orbp_host.h"

namespace orbp {

constexpr int S3_TPB = 256;

static_assert(sizeof(orbp_sim3_dir) % 16 == 0 && sizeof(orbp_sim3_dir) / 4 <= S3_TPB, "the direction record is staged one word per lane");

__global__ __launch_bounds__(S3_TPB) void k_sim3(Sim3 a, Factors F) {
    __shared__ orbp_sim3_dir D;
    const int p = a.p0 + (int)blockIdx.y, tid = threadIdx.x;
    const Lists& L = a.L;
    if (blockIdx.x == 0 && tid == 0 && !(p & 1)) a.nfound[p >> 1] = 0;
    const int n = clamped_count(L, p);
    const int i0 = (int)blockIdx.x * S3_TPB;
    if (i0 >= n) return;                                               // uniform: before the barrier
    stage_view(D, a.dirs, p);
    __syncthreads();
    const int i = i0 + tid;
    if (i >= n) return;
    const size_t e = (size_t)p * L.lcap + i;
    const int fr = a.K.frame ? a.K.frame[p] : p;
    const bool known = D.mode == ORBP_MODE_SIM3 && fr >= 0 && fr < a.K.nframes;

    int status = ORBP_FUSE_SKIPPED, level = 0, best = INT_MAX, best_f = -1;
    float u = 0.0f, v = 0.0f;
    do {
        if (!known || (L.skip && L.skip[e])) break;
        const int slot = L.list[e];
        if (slot < 0 || slot >= a.T.capacity || !a.T.live[slot]) break;
        const float4* g = reinterpret_cast<const float4*>(a.T.geom) + (size_t)slot * 2;
        status = entry_test_sim3(D, F, g[0], g[1], ORBP_FUSE_EMPTY, u, v, level);
        if (status != ORBP_FUSE_EMPTY) break;
        const float radius = D.th * F.f[level];
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

__global__ __launch_bounds__(S3_TPB) void k_sim3_agree(Sim3 a) {
    const int p = a.p0 + (int)blockIdx.y, tid = threadIdx.x;
    const Lists& L = a.L;
    const int n1 = clamped_count(L, 2 * p), n2 = clamped_count(L, 2 * p + 1);
    const int i1 = (int)blockIdx.x * S3_TPB + tid;
    bool agreed = false;
    if (i1 < n1) {
        const int32_t* m1 = a.out.best_idx + (size_t)(2 * p) * L.lcap;
        const int32_t* m2 = m1 + L.lcap;
        const int idx2 = m1[i1];
        agreed = idx2 >= 0 && idx2 < n2 && m2[idx2] == i1;            // beyond direction 2 -> 1's list nothing is read
        a.match12[(size_t)p * L.lcap + i1] = agreed ? idx2 : -1;
    }
    const unsigned long long m = __ballot(agreed);
    if ((tid & 63) == 0 && m) atomicAdd(a.nfound + p, __popcll(m));
}

hipError_t launch_sim3(const Sim3& a, int npairs, const Factors& F, hipStream_t st) {
    const int tiles = (a.L.lcap + S3_TPB - 1) / S3_TPB;
    hipError_t e = for_view_chunks(2 * npairs, [&](int p0, int np) {
        Sim3 b = a;
        b.p0 = p0;
        k_sim3<<<dim3(tiles, np), S3_TPB, 0, st>>>(b, F);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    return for_view_chunks(npairs, [&](int p0, int np) {
        Sim3 b = a;
        b.p0 = p0;
        k_sim3_agree<<<dim3(tiles, np), S3_TPB, 0, st>>>(b);
        return hipGetLastError();
    });
}

}  // namespace orbp
