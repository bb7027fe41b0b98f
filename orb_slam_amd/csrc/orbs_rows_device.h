// Device code the searches over resident key-frame rows share (orbs_bow_rows.hip, orbs_tri_rows.hip): the walk of one query node against its
// train run, which the first kernel of both is (each brings its decision rule), and the second kernel of both, which turns the
// one-record-per-list-position scratch of a pair into its feature-indexed outputs.
#pragma once
#include <hip/hip_runtime.h>

#include "orbs_device.h"
#include "orbs_rows.h"

namespace orbs {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ unsigned long long lane_u64(unsigned long long v, int l) {
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}

// The claim state of a train run, one bit per list position, in registers: lane c holds the 64-bit masks of chunks c and c + 64 (cap <= 8192
// gives at most 128 chunks of 64 positions).
struct ClaimBits {
    unsigned long long m0 = 0, m1 = 0;
    template <class F> __device__ __forceinline__ void word(int c, F f) { if (c < 64) f(m0); else f(m1); }      // c is wave-uniform: a scalar branch
    __device__ __forceinline__ void put(int lane, int c, unsigned long long ballot) {
        if (lane == (c & 63)) word(c, [&](unsigned long long& w) { w = ballot; });
    }
    __device__ __forceinline__ unsigned long long chunk(int c) {                                          // wave-uniform
        unsigned long long v;
        word(c, [&](unsigned long long& w) { v = w; });
        return lane_u64(v, c & 63);
    }
    __device__ __forceinline__ void claim(int lane, int pos) {
        const int c = pos >> 6;
        if (lane == (c & 63)) word(c, [&](unsigned long long& w) { w |= 1ull << (pos & 63); });
    }
};

// What a rule's resolve() returns, wave-uniform: the two distances of the record, the list position to claim (-1: the query takes nothing) and,
// from a rule that keys by feature (Rule::by_feature), the feature there; else the walk looks it up at that position.
struct RowsPick { int best, second, pos, idx2; };

// One wave resolves query node j of row qr (pair p) against the run of the same node in row tr.  It finds the node in the train row's ascending
// fv_node by binary search and resolves the node's queries in list order.  The run is scanned in 64-entry chunks, lane l taking list positions
// l, l + 64, ... : one path for nodes of every size.  A run of up to 64 entries keeps its features, descriptors and the rule's Held state in
// registers for all queries; a longer one reads them again per query through L2.  Positions behind the run, features outside the train row and
// features claimed on entry start out set in the claim state.  Queries are loaded 64 at a time, one per lane with the rule's Query state, and
// broadcast by readlane; per query a lane offers its unclaimed candidates to the rule's Acc, and the rule's resolve() joins the lanes.  A lane
// collects its query's result and stores ONE record per list position of the query row (a node without a partner stores "never visited"), so
// the records of a pair are complete without having been initialised.  claimed, qvalid: the pair's flags, or null.
template <class Rule>
__device__ __forceinline__ void rows_node_walk(const BowStore& S, int p, int qr, int tr, int j, const uint8_t* claimed, const uint8_t* qvalid, bool rot,
                                               BowRec* rec, const Rule& rule) {
    const int lane = threadIdx.x & 63, cap = S.cap;
    const int32_t* qo = S.fv_off + (size_t)qr * (cap + 1);
    const uint32_t* qf = S.fv_feat + (size_t)qr * cap;
    const uint32_t* tn = S.fv_node + (size_t)tr * cap;
    const int32_t* to = S.fv_off + (size_t)tr * (cap + 1);
    const uint32_t* tf = S.fv_feat + (size_t)tr * cap;
    const int ntq = clampi(S.nt[qr], 0, cap), ntt = clampi(S.nt[tr], 0, cap), nft = clampi(S.nfv[tr], 0, cap);
    const int q0 = clampi(qo[j], 0, cap), q1 = clampi(qo[j + 1], q0, cap);

    // the node in the train row (both node lists ascend): replaces the merge walk
    const uint32_t node = S.fv_node[(size_t)qr * cap + j];
    int lo = 0, hi = nft;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (tn[mid] < node) lo = mid + 1; else hi = mid; }
    const bool common = lo < nft && tn[lo] == node;
    int t0 = 0, t1 = 0;
    if (common) { t0 = clampi(to[lo], 0, cap); t1 = clampi(to[lo + 1], t0, cap); }
    const int T = t1 - t0, nchunks = (T + 63) >> 6;
    const bool single = nchunks <= 1;
    const uint4* tdesc = reinterpret_cast<const uint4*>(S.desc) + (size_t)tr * cap * 2;
    const uint4* qdesc = reinterpret_cast<const uint4*>(S.desc) + (size_t)qr * cap * 2;
    const orbx_keypoint* tkp = S.kps + (size_t)tr * cap;
    const orbx_keypoint* qkp = S.kps + (size_t)qr * cap;

    // claim state on entry; for a run of one chunk its features, descriptors and what the rule holds of them stay in registers
    ClaimBits bits;
    int tidx = -1;
    uint4 td0 = make_uint4(0, 0, 0, 0), td1 = td0;
    typename Rule::Held held{};
    for (int c = 0; c < max(nchunks, 1); ++c) {                           // (an empty run: one chunk with every position taken)
        const int pos = c * 64 + lane;
        bool taken = true;
        if (pos < T) {
            const uint32_t f = tf[t0 + pos];
            if (f < (uint32_t)ntt) {
                taken = claimed && claimed[f] != 0;
                if (single) { tidx = (int)f; td0 = tdesc[2 * f]; td1 = tdesc[2 * f + 1]; held = rule.hold(tkp[f]); }
            }
        }
        bits.put(lane, c, __ballot(taken));
    }

    for (int qc = q0; qc < q1; qc += 64) {
        // this chunk's queries, one per lane
        const int k = qc + lane;
        int idx1 = -1;
        bool valid = false;
        uint4 qd0 = make_uint4(0, 0, 0, 0), qd1 = qd0;
        typename Rule::Query mine{};
        if (k < q1) {
            const uint32_t f = qf[k];
            if (f < (uint32_t)ntq) {
                idx1 = (int)f;
                valid = common && (!qvalid || qvalid[f] != 0);
                if (valid) { qd0 = qdesc[2 * f]; qd1 = qdesc[2 * f + 1]; mine = rule.query(qkp[f]); }
            }
        }
        int r_idx2 = -1, r_best = -1, r_second = -1;
        unsigned long long todo = __ballot(valid);
        while (todo) {                                                   // in list order; everything below is wave-uniform but the keys
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint4 b0 = lane_u4(qd0, l), b1 = lane_u4(qd1, l);
            const typename Rule::Query q = mine.of_lane(l);
            typename Rule::Acc acc;
            if (single) {
                if (!((bits.chunk(0) >> lane) & 1)) acc.offer(hamming_key(td0, td1, b0, b1), (uint32_t)tidx, lane, [&] { return held; }, q, rule);
            } else {
                for (int c = 0; c < nchunks; ++c) {
                    if ((bits.chunk(c) >> lane) & 1) continue;           // claimed, outside the row or behind the run: nothing is read
                    const int pos = c * 64 + lane;
                    const uint32_t f = tf[t0 + pos];
                    acc.offer(hamming_key(tdesc[2 * f], tdesc[2 * f + 1], b0, b1), f, pos, [&] { return rule.hold(tkp[f]); }, q, rule);
                }
            }
            const RowsPick r = rule.resolve(acc, lane);
            int idx2 = -1;
            if (r.pos >= 0) {
                idx2 = Rule::by_feature ? r.idx2 : single ? __builtin_amdgcn_readlane(tidx, r.pos) : (int)tf[t0 + r.pos];
                bits.claim(lane, r.pos);
            }
            if (lane == l) { r_idx2 = idx2; r_best = r.best; r_second = r.second; }
        }
        if (k < q1) {
            int bin = 255;
            if (rot && r_idx2 >= 0) bin = rot_bin(qkp[idx1].angle, tkp[r_idx2].angle);
            rec[(size_t)p * cap + k] = BowRec{r_idx2, bin, r_best, r_second};
        }
    }
}

// One workgroup of TPB threads finishes pair p = (query row qr, train row tr): it sets the pair's outputs to -1, walks the records of the query
// row's list, builds the rotation histogram in LDS (integer adds: the result does not depend on their order), takes the three maxima, writes the
// surviving matches to q2t / t2q, best / second of every listed query, and the count.  Without `rot` it only scatters and counts.  A filtered
// match kept its claim during the scan, as in the reference.  rec, O: the pair's records and outputs start at + p * cap.
template <int TPB>
__device__ __forceinline__ void rows_finish(bool rot, const BowStore& S, int qr, int tr, const BowOut& O, const BowRec* rec, int p) {
    __shared__ int hist[32];
    __shared__ int total;
    const int tid = threadIdx.x, cap = S.cap;
    const size_t ob = (size_t)p * cap;
    for (int i = tid; i < cap; i += TPB) {
        if (O.q2t) O.q2t[ob + i] = -1;
        if (O.t2q) O.t2q[ob + i] = -1;
        if (O.best) O.best[ob + i] = -1;
        if (O.second) O.second[ob + i] = -1;
    }
    if (tid < 32) hist[tid] = 0;
    if (tid == 0) total = 0;
    const bool known = (unsigned)qr < (unsigned)S.nrows && (unsigned)tr < (unsigned)S.nrows;
    __syncthreads();                                                     // the -1s are in place before any entry is written again
    if (!known) {
        if (tid == 0) O.nmatches[p] = 0;
        return;
    }
    const int32_t* qo = S.fv_off + (size_t)qr * (cap + 1);
    const uint32_t* qf = S.fv_feat + (size_t)qr * cap;
    const int nfq = clampi(S.nfv[qr], 0, cap);
    const int ntq = clampi(S.nt[qr], 0, cap), ntt = clampi(S.nt[tr], 0, cap);
    const int k0 = nfq > 0 ? clampi(qo[0], 0, cap) : 0, k1 = nfq > 0 ? clampi(qo[nfq], k0, cap) : 0;

    for (int k = k0 + tid; k < k1; k += TPB) {
        const uint32_t idx1 = qf[k];
        if (idx1 >= (uint32_t)ntq) continue;
        const BowRec r = rec[ob + k];
        if (O.best) O.best[ob + idx1] = r.best;
        if (O.second) O.second[ob + idx1] = r.second;
        if (rot && (unsigned)r.idx2 < (unsigned)ntt && (unsigned)r.bin < (unsigned)HISTO_LENGTH) atomicAdd(&hist[r.bin], 1);
    }
    __syncthreads();
    int i1 = -1, i2 = -1, i3 = -1;
    if (rot) three_maxima(hist, HISTO_LENGTH, i1, i2, i3);
    int cnt = 0;
    for (int k = k0 + tid; k < k1; k += TPB) {
        const uint32_t idx1 = qf[k];
        if (idx1 >= (uint32_t)ntq) continue;
        const BowRec r = rec[ob + k];
        if ((unsigned)r.idx2 >= (unsigned)ntt) continue;
        if (rot && (unsigned)r.bin < (unsigned)HISTO_LENGTH && r.bin != i1 && r.bin != i2 && r.bin != i3) continue;      // cleared; its claim held during the scan
        if (O.q2t) O.q2t[ob + idx1] = r.idx2;
        if (O.t2q) O.t2q[ob + r.idx2] = (int)idx1;
        cnt++;
    }
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) O.nmatches[p] = total;
}

constexpr int ROWS_FINISH_TPB = 256;

}  // namespace orbs
