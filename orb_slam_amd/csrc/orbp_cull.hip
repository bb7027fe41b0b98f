// Key-frame culling on gfx950 (wave64): the decisions of LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:524-578) with what
// KeyFrame::SetBadFlag (src/KeyFrame.cc:497-515: the guard and the EraseObservation loop) and MapPoint::EraseObservation / SetBadFlag
// (src/MapPoint.cc:71-122) do to the observations between two candidates, over the slot and octave columns of the resident key-frame rows.
// include/orbp.h is the boundary and states the contract; the host side lives in orbp_project.hip.
//
// Eight words per slot in the handle's scratch hold the slot's observers by level (sixteen 16-bit counts, level l in word l >> 1 at bit
// 16 * (l & 1); a count is at most the number of rows, <= 65535, so a field cannot carry), one word per slot says that the point went bad
// inside this call.  The stream is the only ordering between the launches:
//   k_cull_build<true>    flat over all nkf*cap entries: one integer atomic add of the entry's level field.  Nothing depends on arrival order.
//   k_cull_count          one workgroup per candidate strides its row, gathers the eight words of every entry's slot, takes the total and the
//                         prefix up to octave + 1 with SWAR adds, and reduces nMPs and nRed (ballot + popcount per wave, the wave totals meet in
//                         LDS): one plain store each of nmps, nred, cull, against the INITIAL state.  These are final for every candidate up to
//                         and including the first one culled; in the common case, where nothing is culled, for all of them.
//   k_cull_walk           ONE workgroup of 1024 threads: the first culled candidate by a minimum over the flags (none: it returns at once), then the
//                         candidates behind it in order: erase the culled row (atomic subtract of the field; the value the atomic returns gives
//                         the slot's new total, <= 2 sets its dead word), barrier, recount the next candidate with the device function
//                         k_cull_count calls, overwrite its three outputs.  The erased rows are a bitmap in LDS.  Every loop bound is uniform,
//                         every barrier sits outside divergent code and no workgroup waits for another, so nothing here can hang.
//                         Every word of the level counts and of the dead flags is read in this kernel with a relaxed agent-scope atomic load,
//                         never a plain one: the atomics are performed at L2 and do not update the CU's L1, so a plain load behind a barrier
//                         may see the line as it was.
//   k_cull_build<false>   walks the same entries and puts the words back (level counts and dead flag 0) with plain stores.
// Every index is tested before it is used: a slot, a row, an octave or a count that is out of range reads nothing.
#include <hip/hip_runtime.h>

#include "orbp.h"
#include "orbp_device.h"
#include "orbp_host.h"

namespace orbp {

constexpr int CU_TPB = LOCAL_TILE;                     // k_cull_build, k_cull_count
constexpr int CU_WALK_TPB = 1024;                      // k_cull_walk
constexpr int CU_ROW_WORDS = (ORBP_LOCAL_MAX_ROWS + 32) / 32;   // the erased rows, one bit each

// Feature i of row r (r in range): its slot when the entry takes part (inside the row's count, the slot in range and live, the octave below
// nlevels), else -1
__device__ __forceinline__ int cull_entry(const Cull& a, int r, int i, int nt, int& oct) {
    if (i >= nt) return -1;
    const size_t e = (size_t)r * a.K.K.cap + i;
    const int s = a.K.K.slot[e];
    if (s < 0 || s >= a.T.capacity || !a.T.live[s]) return -1;
    oct = a.K.oct[e];
    return oct < a.K.nlevels ? s : -1;
}

// SET: the entry's observation is counted; else the words it touched are put back.  The scratch is put back by walking the inputs again, not from a
// log: the columns and the table's live bytes must be the same in both launches, which one call guarantees (it runs under the handle's lock and
// inside its event chain, and the walk in between changes neither).
template <bool SET>
__global__ __launch_bounds__(CU_TPB) void k_cull_build(Cull a) {
    const size_t e = (size_t)blockIdx.x * CU_TPB + threadIdx.x;
    if (e >= (size_t)a.K.K.nkf * a.K.K.cap) return;
    const int r = (int)(e / (size_t)a.K.K.cap), i = (int)(e - (size_t)r * a.K.K.cap);
    int oct = 0;
    const int s = cull_entry(a, r, i, clamp_count(a.K.K.nt[r], a.K.K.cap), oct);
    if (s < 0) return;
    uint32_t* w = a.S.hist + (size_t)s * CULL_WORDS + (oct >> 1);
    if constexpr (SET) atomicAdd(w, 1u << (16 * (oct & 1)));
    else { *w = 0u; a.S.dead[s] = 0u; }
}

// WALK: a word this launch changes, so past L1; else a plain load
template <bool WALK>
__device__ __forceinline__ uint32_t cull_word(const uint32_t* p) {
    if constexpr (WALK) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

__device__ __forceinline__ int cull_fields(uint32_t w) { return (int)(w & 0xFFFFu) + (int)(w >> 16); }

// nMPs and nRed of row r as the map stands, called by all NT threads of a workgroup (valid: r is in range and not erased; else both are 0 and
// nothing is read).  One barrier; the caller's next barrier lets wave_total be rewritten.
template <bool WALK, int NT>
__device__ __forceinline__ void cull_count(const Cull& a, int r, bool valid, int (&wave_total)[2][NT / 64], int& nmps, int& nred) {
    const int tid = threadIdx.x;
    const int nt = valid ? clamp_count(a.K.K.nt[r], a.K.K.cap) : 0;
    int wm = 0, wr = 0;
    for (int base = 0; base < nt; base += NT) {
        int oct = 0;
        const int s = cull_entry(a, r, base + tid, nt, oct);
        bool counted = false, redundant = false;
        if (s >= 0 && cull_word<WALK>(a.S.dead + s) == 0u) {
            counted = true;
            const uint32_t* h = a.S.hist + (size_t)s * CULL_WORDS;
            const int top = oct + 1;                                   // levels <= top count
            uint32_t all = 0u, below = 0u;
            for (int k = 0; k < CULL_WORDS; k++) {
                const uint32_t w = cull_word<WALK>(h + k);
                all += w;
                below += 2 * k + 1 <= top ? w : (2 * k == top ? (w & 0xFFFFu) : 0u);
            }
            redundant = cull_fields(all) > 3 && cull_fields(below) - 1 >= 3;
        }
        wm += __popcll(__ballot(counted));
        wr += __popcll(__ballot(redundant));
    }
    if ((tid & 63) == 0) { wave_total[0][tid >> 6] = wm; wave_total[1][tid >> 6] = wr; }
    __syncthreads();
    nmps = nred = 0;
    for (int w = 0; w < NT / 64; w++) { nmps += wave_total[0][w]; nred += wave_total[1][w]; }
}

// :575, one IEEE multiply and one compare
__device__ __forceinline__ int cull_decision(int nmps, int nred) { return (double)nred > 0.9 * (double)nmps ? 1 : 0; }

__global__ __launch_bounds__(CU_TPB) void k_cull_count(Cull a) {
    __shared__ int wave_total[2][CU_TPB / 64];
    const int c = blockIdx.x, r = a.C.cand[c];
    int nmps, nred;
    cull_count<false, CU_TPB>(a, r, r >= 0 && r < a.K.K.nkf, wave_total, nmps, nred);
    if (threadIdx.x == 0) { a.O.nmps[c] = nmps; a.O.nred[c] = nred; a.O.cull[c] = cull_decision(nmps, nred); }
}

// Row r (in range, not erased) loses its observations: every entry that takes part, dead or not.  A slot occurs once per row, so the lane that
// subtracts is the only one that changes the slot in this pass: the other seven words are as they were, its own is what the atomic returned.
__device__ __forceinline__ void cull_erase(const Cull& a, int r) {
    const int nt = clamp_count(a.K.K.nt[r], a.K.K.cap);
    for (int i = threadIdx.x; i < nt; i += CU_WALK_TPB) {
        int oct = 0;
        const int s = cull_entry(a, r, i, nt, oct);
        if (s < 0) continue;
        uint32_t* h = a.S.hist + (size_t)s * CULL_WORDS;
        const uint32_t one = 1u << (16 * (oct & 1));
        uint32_t all = atomicSub(h + (oct >> 1), one) - one;
        for (int k = 0; k < CULL_WORDS; k++)
            if (k != (oct >> 1)) all += cull_word<true>(h + k);
        // (were the precondition broken and the slot held twice in this row, two lanes would each see a total in which the other's subtraction may
        // or may not have landed: the dead decision would depend on timing, the addresses would not)
        if (cull_fields(all) <= 2) __hip_atomic_store(a.S.dead + s, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                  // the dead words are at L2 before the barrier lets anyone look
}

__global__ __launch_bounds__(CU_WALK_TPB) void k_cull_walk(Cull a) {
    __shared__ int wave_total[2][CU_WALK_TPB / 64];
    __shared__ uint32_t erased[CU_ROW_WORDS];
    __shared__ int first;
    const int tid = threadIdx.x, ncand = a.C.ncand;
    for (int w = tid; w < CU_ROW_WORDS; w += CU_WALK_TPB) erased[w] = 0u;
    if (tid == 0) first = ncand;
    __syncthreads();
    // the flags k_cull_count left: the launch boundary orders them, so plain loads
    int mine = ncand;
    for (int c = tid; c < ncand; c += CU_WALK_TPB)
        if (a.O.cull[c]) { mine = c; break; }
    if (mine < ncand) atomicMin(&first, mine);
    __syncthreads();
    const int c0 = first;
    if (c0 >= ncand) return;                                            // uniform: nothing is culled, every output is final
    int r = a.C.cand[c0];                                               // in range: its flag is set
    cull_erase(a, r);
    if (tid == 0) erased[r >> 5] |= 1u << (r & 31);
    __syncthreads();
    for (int c = c0 + 1; c < ncand; c++) {
        r = a.C.cand[c];
        const bool valid = r >= 0 && r < a.K.K.nkf && !((erased[r >> 5] >> (r & 31)) & 1u);
        int nmps, nred;
        cull_count<true, CU_WALK_TPB>(a, r, valid, wave_total, nmps, nred);
        const int cull = cull_decision(nmps, nred);
        if (tid == 0) { a.O.nmps[c] = nmps; a.O.nred[c] = nred; a.O.cull[c] = cull; }
        if (cull) {                                                     // uniform
            cull_erase(a, r);
            if (tid == 0) erased[r >> 5] |= 1u << (r & 31);
        }
        __syncthreads();
    }
}

#define CU_LAUNCHED() do { const hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)

hipError_t launch_cull(const Cull& a, hipStream_t st) {
    const unsigned eblocks = (unsigned)(((size_t)a.K.K.nkf * a.K.K.cap + CU_TPB - 1) / CU_TPB);
    k_cull_build<true><<<eblocks, CU_TPB, 0, st>>>(a);
    CU_LAUNCHED();
    k_cull_count<<<a.C.ncand, CU_TPB, 0, st>>>(a);
    CU_LAUNCHED();
    k_cull_walk<<<1, CU_WALK_TPB, 0, st>>>(a);
    CU_LAUNCHED();
    k_cull_build<false><<<eblocks, CU_TPB, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace orbp
