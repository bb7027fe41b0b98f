// Host side of orbs_bow_rows_search* (include/orbs.h): what the two kernels of orbs_bow_rows.hip read and write, the argument checks that need
// no GPU, and the layout of the synchronous host form's block (one pinned copy up, one down).  Plain C++: tests/_probe/bow_rows_host.cpp runs it
// on the CPU.
#pragma once
#include <cmath>
#include <cstdint>

#include "orbs.h"
#include "orbx_host.h"

#pragma GCC visibility push(hidden)
namespace orbs {

// one match record per position of the query row's FeatureVector list: the train feature (-1 none), the rotation bin (255 none), the two
// distances the scan left (-1: the query was never visited)
struct BowRec { int32_t idx2, bin, best, second; };

// The rows of the key-frame store (row r at + r*cap, its FeatureVector offsets at + r*(cap+1)) ...
struct BowStore {
    const orbx_keypoint* kps;
    const uint8_t* desc;
    const int32_t* nt;
    const uint32_t* fv_node;
    const int32_t* fv_off;
    const uint32_t* fv_feat;
    const int32_t* nfv;
    int nrows, cap;
};
// ... the pairs searched over them with their per-pair flags ...
struct BowPairs {
    const int32_t* pair;
    int npairs;
    const uint8_t* qvalid;
    const uint8_t* claimed;
};
// ... and the per-pair outputs
struct BowOut { int32_t *q2t, *t2q, *best, *second, *nmatches; };

struct BowRows {
    BowStore S;
    BowPairs P;
    BowOut O;
    BowRec* rec;           // scratch: npairs * cap records
};

constexpr int BOW_ROWS_WAVES = 4;                              // (pair, node) waves of one workgroup of k_bow_rows
inline int bow_rows_blocks_per_pair(int cap) { return (cap + BOW_ROWS_WAVES - 1) / BOW_ROWS_WAVES; }

inline bool below_2g(long long v) { return v < (1LL << 31); }

// on_device: pairs, flags and outputs are device memory, so only presence and alignment can be checked; else the pairs are walked.
// rows_device: the store is read in place (descriptors in 16-byte pieces); host rows are copied into aligned slots.
inline int check_bow_rows(const orbs_params* prm, const BowPairs& P, const BowStore& S, const BowOut& O, bool on_device, bool rows_device) {
    if (!prm || prm->rule != ORBS_RULE_BOW || prm->th < 0 || prm->th > 256 || std::isnan(prm->ratio)) return ORBX_ERR_ARG;
    if (P.npairs < 0 || S.nrows < 1 || S.cap < 1 || S.cap > ORBF_MAX_FEATURES) return ORBX_ERR_ARG;
    if (!below_2g((long long)P.npairs * S.cap) || !below_2g((long long)S.nrows * (S.cap + 1)) ||
        !below_2g((long long)P.npairs * bow_rows_blocks_per_pair(S.cap)))
        return ORBX_ERR_ARG;
    if (P.npairs == 0) return ORBX_OK;
    if (!P.pair || !S.kps || !S.desc || !S.nt || !S.fv_node || !S.fv_off || !S.fv_feat || !S.nfv || !O.nmatches) return ORBX_ERR_ARG;
    auto misaligned = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
    if (rows_device && (misaligned(S.desc, 16) || misaligned(S.kps, 4) || misaligned(S.fv_node, 4) || misaligned(S.fv_off, 4) || misaligned(S.fv_feat, 4)))
        return ORBX_ERR_ARG;
    if (on_device && (misaligned(S.nt, 4) || misaligned(S.nfv, 4))) return ORBX_ERR_ARG;
    if (on_device)
        return misaligned(P.pair, 4) || misaligned(O.q2t, 4) || misaligned(O.t2q, 4) || misaligned(O.best, 4) || misaligned(O.second, 4) ||
                       misaligned(O.nmatches, 4)
                   ? ORBX_ERR_ARG
                   : ORBX_OK;
    for (int p = 0; p < 2 * P.npairs; p++)
        if (P.pair[p] < 0 || P.pair[p] >= S.nrows) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The block of the host form:
//   up    [pair | qvalid | claimed | nt | nfv | kps | desc | fv_node | fv_off | fv_feat]   (absent: the flags the caller passes none of, the rows'
//                                                                                          five large arrays when they are on the device; the counts
//                                                                                          nt and nfv are host arrays either way)
//   down  [nmatches | q2t | t2q | best | second]                                           (absent: the outputs the caller wants none of)
// behind it, device memory only: the records between the two kernels
struct BowRowsBlock {
    orbx::Layout L;
    orbx::Layout::Slot<int32_t> pair, nt, nfv, fv_off, nmatches, q2t, t2q, best, second;
    orbx::Layout::Slot<uint32_t> fv_node, fv_feat;
    orbx::Layout::Slot<uint8_t> qvalid, claimed, desc;
    orbx::Layout::Slot<orbx_keypoint> kps;
    orbx::Layout::Slot<BowRec> rec;
    int npairs, nrows;
    size_t nent, nfeat;                                // npairs * cap, nrows * cap
    BowRowsBlock(const BowPairs& p, const BowStore& s, const BowOut& o, bool rows_upload)
        : npairs(p.npairs), nrows(s.nrows), nent((size_t)p.npairs * s.cap), nfeat((size_t)s.nrows * s.cap) {
        pair = L.add<int32_t>(2 * (size_t)npairs); qvalid = L.add<uint8_t>(nent, p.qvalid != nullptr); claimed = L.add<uint8_t>(nent, p.claimed != nullptr);
        nt = L.add<int32_t>(nrows); nfv = L.add<int32_t>(nrows);
        kps = L.add<orbx_keypoint>(nfeat, rows_upload); desc = L.add<uint8_t>(nfeat * 32, rows_upload);
        fv_node = L.add<uint32_t>(nfeat, rows_upload); fv_off = L.add<int32_t>((size_t)nrows * (s.cap + 1), rows_upload); fv_feat = L.add<uint32_t>(nfeat, rows_upload);
        L.end_upload();
        nmatches = L.add<int32_t>(npairs);
        q2t = L.add<int32_t>(nent, o.q2t != nullptr); t2q = L.add<int32_t>(nent, o.t2q != nullptr);
        best = L.add<int32_t>(nent, o.best != nullptr); second = L.add<int32_t>(nent, o.second != nullptr);
        L.end_download();
        rec = L.add<BowRec>(nent);
    }
    // copies the caller's host arrays into the pinned block h and names everything inside the device block d; rows that are not part of the
    // block are passed through
    BowRows stage(uint8_t* h, uint8_t* d, const BowPairs& p, const BowStore& s) const {
        using orbx::Layout;
        BowRows a;
        a.P = {Layout::put(h, d, pair, p.pair, 2 * (size_t)npairs), npairs, Layout::put(h, d, qvalid, p.qvalid, nent), Layout::put(h, d, claimed, p.claimed, nent)};
        a.S = {Layout::put(h, d, kps, s.kps, nfeat), Layout::put(h, d, desc, s.desc, nfeat * 32), Layout::put(h, d, nt, s.nt, nrows),
               Layout::put(h, d, fv_node, s.fv_node, nfeat), Layout::put(h, d, fv_off, s.fv_off, (size_t)nrows * (s.cap + 1)),
               Layout::put(h, d, fv_feat, s.fv_feat, nfeat), Layout::put(h, d, nfv, s.nfv, nrows), s.nrows, s.cap};
        a.O = {Layout::at(d, q2t), Layout::at(d, t2q), Layout::at(d, best), Layout::at(d, second), Layout::at(d, nmatches)};
        a.rec = Layout::at(d, rec);
        return a;
    }
    // what the kernels wrote, out of the pinned block h into the caller's arrays (a null one is passed over)
    void unpack(const uint8_t* h, const BowOut& o) const {
        using orbx::Layout;
        uint8_t* b = const_cast<uint8_t*>(h);
        std::memcpy(o.nmatches, Layout::at(b, nmatches), (size_t)npairs * 4);
        if (o.q2t) std::memcpy(o.q2t, Layout::at(b, q2t), nent * 4);
        if (o.t2q) std::memcpy(o.t2q, Layout::at(b, t2q), nent * 4);
        if (o.best) std::memcpy(o.best, Layout::at(b, best), nent * 4);
        if (o.second) std::memcpy(o.second, Layout::at(b, second), nent * 4);
    }
};

}  // namespace orbs
#pragma GCC visibility pop
