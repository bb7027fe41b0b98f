// The local map on gfx950 (wave64): the key-frame votes of Tracking::UpdateReferenceKeyFrames (reference src/Tracking.cc:768-783) and
// KeyFrame::UpdateConnections (src/KeyFrame.cc:334-363), and the local point list of Tracking::UpdateReferencePoints (src/Tracking.cc:742-760) with
// the stamps of Tracking::SearchReferencePointsInFrustum's first loop (:678-694), over the map-point column of the resident key-frame rows.
// include/orbp.h is the boundary and states the contract; the host side lives in orbp_project.hip.
//
// Two words per (problem, slot) in the handle's scratch carry everything between the launches, and the stream is the only ordering:
//   k_local_mult<true>    one lane per query entry: an integer atomic add of 1 into the slot's word, so a slot held at two features counts twice and
//                         nothing depends on arrival order.
//   k_local_votes         one workgroup per (row, problem) strides the row's column coalesced, gathers the multiplicity of every live slot, and
//                         reduces: a shuffle sum per wave, the four wave totals in LDS, ONE plain store per row.  The votes need no atomics and no
//                         zeroing.  (A flat grid over (row, tile) with one atomic add per wave was the other shape: a row is at most 32 tiles, the
//                         grid is nkf * nproblems workgroups either way, and this one leaves every output word with one writer.)
//   k_local_first         flat over (tile, listed row, problem), one lane per feature: atomicMin of the walk position j*cap + i into the slot's word.
//   k_local_count         the same grid: an entry is kept when its position IS the slot's minimum; the tile's number of kept entries (ballot, the
//                         four wave totals meet in LDS) goes into the tile's own word.  Every workgroup of the grid writes its word.
//   k_local_pack          the same grid: a workgroup adds the words of the tiles in front of it in its problem, ranks its kept entries in walk
//                         order again (orbx::tile_rank) and writes slot and skip flag at base + rank while that is below lcap.  The problem's last
//                         tile writes the counts.  What k_loop_test / k_loop_pack do for the loop projection (orbp_loop.hip).
//   k_local_unfirst, k_local_mult<false>   put the words back (0xFFFFFFFF, 0) by walking the same entries again: plain stores of one value, so the
//                         scratch is reset without a host synchronisation and at the cost of what the call touched.
//   k_rows_mark<true>, k_rows_purge, k_rows_mark<false>   orbp_rows_purge_device: the dying slots are marked in problem 0's multiplicity words, one flat
//                         scan over the columns turns every entry that names a marked slot into -1, and the marks are put back.
// No workgroup waits for another inside a launch and no flag passes between them.  Every index is tested before it is used: a slot, a row
// or a count that is out of range reads nothing.
#include <hip/hip_runtime.h>

#include "orbp.h"
#include "orbp_device.h"
#include "orbp_host.h"

namespace orbp {

constexpr int LM_TPB = LOCAL_TILE;
constexpr int LM_WAVES = LM_TPB / 64;
constexpr uint32_t LM_UNSEEN = 0xFFFFFFFFu;            // LocalScratch::first between calls

template <bool SET>
__global__ __launch_bounds__(LM_TPB) void k_local_mult(Query Q, int capacity, uint32_t* mult) {
    const int p = blockIdx.y, j = (int)blockIdx.x * LM_TPB + (int)threadIdx.x;
    if (j >= clamp_count(Q.nq[p], Q.qcap)) return;
    const int s = Q.q[(size_t)p * Q.qcap + j];
    if (s < 0 || s >= capacity) return;
    uint32_t* w = mult + (size_t)p * capacity + s;
    if constexpr (SET) atomicAdd(w, 1u);
    else *w = 0u;
}

__global__ __launch_bounds__(LM_TPB) void k_local_votes(LocalVotes a) {
    __shared__ int wave_total[LM_WAVES];
    const int k = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const int nt = clamp_count(a.K.nt[k], a.K.cap);
    const int32_t* col = a.K.slot + (size_t)k * a.K.cap;
    const uint32_t* mult = a.S.mult + (size_t)p * a.T.capacity;
    int sum = 0;
    for (int i = tid; i < nt; i += LM_TPB) {
        const int s = col[i];
        if (s >= 0 && s < a.T.capacity && a.T.live[s]) sum += (int)mult[s];
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0) wave_total[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        int v = 0;
        for (int w = 0; w < LM_WAVES; w++) v += wave_total[w];
        a.votes[(size_t)p * a.K.nkf + k] = v;
    }
}

// Feature i of the j-th listed row of problem p: its slot when the row is listed and in range, the feature inside the row's count and the slot in
// range and live; else -1.  The walk position of the entry is j*cap + i.
__device__ __forceinline__ int local_entry(const LocalPoints& a, int p, int j, int i) {
    if (j >= clamp_count(a.R.nrows[p], a.R.rcap)) return -1;
    const int r = a.R.rows[(size_t)p * a.R.rcap + j];
    if (r < 0 || r >= a.K.nkf || i >= clamp_count(a.K.nt[r], a.K.cap)) return -1;
    const int s = a.K.slot[(size_t)r * a.K.cap + i];
    return s >= 0 && s < a.T.capacity && a.T.live[s] ? s : -1;
}

// SET: the least position per slot; else the word is put back
template <bool SET>
__global__ __launch_bounds__(LM_TPB) void k_local_first(LocalPoints a) {
    const int p = blockIdx.z, j = blockIdx.y, i = (int)blockIdx.x * LM_TPB + (int)threadIdx.x;
    const int s = local_entry(a, p, j, i);
    if (s < 0) return;
    uint32_t* w = a.S.first + (size_t)p * a.T.capacity + s;
    if constexpr (SET) atomicMin(w, (uint32_t)j * (uint32_t)a.K.cap + (uint32_t)i);
    else *w = LM_UNSEEN;
}

__device__ __forceinline__ bool local_keep(const LocalPoints& a, int p, int j, int i, int s) {
    return s >= 0 && a.S.first[(size_t)p * a.T.capacity + s] == (uint32_t)j * (uint32_t)a.K.cap + (uint32_t)i;
}

__global__ __launch_bounds__(LM_TPB) void k_local_count(LocalPoints a) {
    __shared__ int wave_total[LM_WAVES];
    const int p = blockIdx.z, j = blockIdx.y, tid = threadIdx.x, i = (int)blockIdx.x * LM_TPB + tid;
    const bool keep = local_keep(a, p, j, i, local_entry(a, p, j, i));
    const unsigned long long m = __ballot(keep);
    if ((tid & 63) == 0) wave_total[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        for (int w = 0; w < LM_WAVES; w++) c += wave_total[w];
        a.S.tile_count[((size_t)p * gridDim.y + j) * gridDim.x + blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(LM_TPB) void k_local_pack(LocalPoints a) {
    __shared__ int wave_total[LM_WAVES];
    const int p = blockIdx.z, j = blockIdx.y, tid = threadIdx.x, i = (int)blockIdx.x * LM_TPB + tid;
    const int me = j * (int)gridDim.x + (int)blockIdx.x, ntiles = (int)(gridDim.x * gridDim.y);
    const bool last = me == ntiles - 1;
    if (j >= clamp_count(a.R.nrows[p], a.R.rcap) && !last) return;      // uniform, before the barriers: nothing of this row is listed
    // the kept entries of the tiles in front of this one: k_local_count wrote every word of the grid
    const int32_t* tc = a.S.tile_count + (size_t)p * ntiles;
    int part = 0;
    for (int t = tid; t < me; t += LM_TPB) part += tc[t];
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if ((tid & 63) == 0) wave_total[tid >> 6] = part;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < LM_WAVES; w++) base += wave_total[w];
    __syncthreads();                                                   // tile_rank rewrites wave_total

    const int s = local_entry(a, p, j, i);
    const bool keep = local_keep(a, p, j, i, s);
    const int q = orbx::tile_rank<LM_WAVES>(keep, wave_total, base);    // base: now through this tile
    if (keep && q < a.O.lcap) {
        const size_t o = (size_t)p * a.O.lcap + q;
        a.O.list[o] = s;
        a.O.skip[o] = a.Q.q && a.S.mult[(size_t)p * a.T.capacity + s] ? 1 : 0;
    }
    if (last && tid == 0) {
        a.O.nlist[p] = base;
        a.O.overflow[p] = base > a.O.lcap ? 1 : 0;
    }
}

template <bool SET>
__global__ __launch_bounds__(LM_TPB) void k_rows_mark(int n, const int32_t* slots, int capacity, uint32_t* mark) {
    const int i = (int)blockIdx.x * LM_TPB + (int)threadIdx.x;
    if (i >= n) return;
    const int s = slots[i];
    if (s >= 0 && s < capacity) mark[s] = SET ? 1u : 0u;
}

__global__ __launch_bounds__(LM_TPB) void k_rows_purge(size_t nent, int32_t* kf_slot, int capacity, const uint32_t* mark) {
    const size_t e = (size_t)blockIdx.x * LM_TPB + threadIdx.x;
    if (e >= nent) return;
    const int s = kf_slot[e];
    if (s >= 0 && s < capacity && mark[s]) kf_slot[e] = -1;
}

#define LM_LAUNCHED() do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t launch_local_votes(const LocalVotes& a, int nproblems, hipStream_t st) {
    const dim3 qgrid((a.Q.qcap + LM_TPB - 1) / LM_TPB, nproblems);
    k_local_mult<true><<<qgrid, LM_TPB, 0, st>>>(a.Q, a.T.capacity, a.S.mult);
    LM_LAUNCHED();
    k_local_votes<<<dim3(a.K.nkf, nproblems), LM_TPB, 0, st>>>(a);
    LM_LAUNCHED();
    k_local_mult<false><<<qgrid, LM_TPB, 0, st>>>(a.Q, a.T.capacity, a.S.mult);
    return hipGetLastError();
}

hipError_t launch_local_points(const LocalPoints& a, int nproblems, hipStream_t st) {
    const dim3 qgrid((a.Q.qcap + LM_TPB - 1) / LM_TPB, nproblems), grid(local_tiles(a.K.cap), a.R.rcap, nproblems);
    if (a.Q.q) {
        k_local_mult<true><<<qgrid, LM_TPB, 0, st>>>(a.Q, a.T.capacity, a.S.mult);
        LM_LAUNCHED();
    }
    k_local_first<true><<<grid, LM_TPB, 0, st>>>(a);
    LM_LAUNCHED();
    k_local_count<<<grid, LM_TPB, 0, st>>>(a);
    LM_LAUNCHED();
    k_local_pack<<<grid, LM_TPB, 0, st>>>(a);
    LM_LAUNCHED();
    k_local_first<false><<<grid, LM_TPB, 0, st>>>(a);
    LM_LAUNCHED();
    if (a.Q.q) {
        k_local_mult<false><<<qgrid, LM_TPB, 0, st>>>(a.Q, a.T.capacity, a.S.mult);
        LM_LAUNCHED();
    }
    return hipSuccess;
}

hipError_t launch_rows_purge(const RowsPurge& a, hipStream_t st) {
    const int sblocks = (a.n + LM_TPB - 1) / LM_TPB;
    k_rows_mark<true><<<sblocks, LM_TPB, 0, st>>>(a.n, a.slots, a.capacity, a.mark);
    LM_LAUNCHED();
    k_rows_purge<<<(unsigned)((a.nent + LM_TPB - 1) / LM_TPB), LM_TPB, 0, st>>>(a.nent, a.kf_slot, a.capacity, a.mark);
    LM_LAUNCHED();
    k_rows_mark<false><<<sblocks, LM_TPB, 0, st>>>(a.n, a.slots, a.capacity, a.mark);
    return hipGetLastError();
}

}  // namespace orbp
