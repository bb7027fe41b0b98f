// Host side of the searches over the rows of a resident key-frame store: orbs_bow_rows_search*, orbs_tri_rows_search* (include/orbs.h) and
// orbt_new_points_rows* (include/orbt.h).  What the kernels of orbs_bow_rows.hip and orbs_tri_rows.hip read and write, the argument checks that
// need no GPU, the layouts of the synchronous host forms' blocks (one pinned copy up, one down), and what the entry points keep per device with
// the two forms every search goes through.  Plain C++: tests/_probe/bow_rows_host.cpp and tests/_probe/tri_rows_host.cpp run it on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>

#include "orbs.h"
#include "orbt.h"
#include "orbx_host.h"

#pragma GCC visibility push(hidden)
namespace orbs {

// one match record per position of the query row's FeatureVector list: the train feature (-1 none), the rotation bin (255 none), the two
// distances the scan left (-1: the query was never visited; SearchByBoW: best and second, SearchForTriangulation: BestDist and the one taken)
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
// ... the pairs searched over them.  pair == NULL: ONE pair, (qr0, tr0), passed by value (the per-neighbour launches of the chain).
// qvalid of pair p at + p*qstride (qstride 0: one array for all pairs; SearchByBoW: cap), claimed and the outputs at + p*cap, F12 at + p*9
// (SearchByBoW: NULL) ...
struct RowPairs {
    const int32_t* pair;
    int npairs;
    const uint8_t* qvalid;
    int qstride;
    const uint8_t* claimed;
    const float* F12;
    int qr0, tr0;
};
// ... and the per-pair outputs
struct BowOut { int32_t *q2t, *t2q, *best, *second, *nmatches; };

struct BowRows {
    BowStore S;
    RowPairs P;
    BowOut O;
    BowRec* rec;           // scratch: npairs * cap records
};
struct TriRows : BowRows {
    float epi_thr[ORBS_MAX_LEVELS];    // orbs_epipolar_bound per octave of the train key point
    int th, check_orientation;
};

constexpr int ROWS_WAVES = 4;                                  // (pair, node) waves of one workgroup of k_bow_rows / k_tri_rows
inline int rows_blocks_per_pair(int cap) { return (cap + ROWS_WAVES - 1) / ROWS_WAVES; }

inline bool below_2g(long long v) { return v < (1LL << 31); }

// bytes of qvalid the pairs address
inline size_t tri_qvalid_bytes(const RowPairs& P, int cap) { return P.qstride == 0 || P.npairs == 0 ? (size_t)cap : (size_t)(P.npairs - 1) * P.qstride + cap; }

// on_device: pairs, flags and outputs are device memory, so only presence and alignment can be checked; else the pairs are walked.
// rows_device: the store is read in place (descriptors in 16-byte pieces); host rows are copied into aligned slots.
inline int check_bow_rows(const orbs_params* prm, const RowPairs& P, const BowStore& S, const BowOut& O, bool on_device, bool rows_device) {
    if (!prm || prm->rule != ORBS_RULE_BOW || prm->th < 0 || prm->th > 256 || std::isnan(prm->ratio)) return ORBX_ERR_ARG;
    if (P.npairs < 0 || S.nrows < 1 || S.cap < 1 || S.cap > ORBF_MAX_FEATURES) return ORBX_ERR_ARG;
    if (!below_2g((long long)P.npairs * S.cap) || !below_2g((long long)S.nrows * (S.cap + 1)) ||
        !below_2g((long long)P.npairs * rows_blocks_per_pair(S.cap)))
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

// check_bow_rows with the triangulation rule: the same refusals, and those of the arguments SearchForTriangulation adds
inline int check_tri_rows(const orbs_params* prm, const RowPairs& P, const BowStore& S, const BowOut& O, const float* level_sigma2, int nlevels,
                          bool on_device, bool rows_device) {
    if (!prm || prm->rule != ORBS_RULE_TRIANGULATION || !level_sigma2 || nlevels < 1 || nlevels > ORBS_MAX_LEVELS) return ORBX_ERR_ARG;
    if (P.qstride != 0 && P.qstride < S.cap) return ORBX_ERR_ARG;
    orbs_params b = *prm;              // ratio is unused by the rule
    b.rule = ORBS_RULE_BOW;
    b.ratio = 0.0f;
    const int rc = check_bow_rows(&b, P, S, O, on_device, rows_device);
    if (rc != ORBX_OK || P.npairs == 0) return rc;
    if (!below_2g((long long)P.npairs * P.qstride + S.cap)) return ORBX_ERR_ARG;
    if (!P.F12 || (on_device && ((uintptr_t)P.F12 & 3))) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The slots of a block that hold the store: [nt | nfv | kps | desc | fv_node | fv_off | fv_feat].  The counts nt and nfv are host arrays either
// way; the five large arrays are absent when the rows are on the device.
struct StoreSlots {
    orbx::Layout::Slot<int32_t> nt, nfv, fv_off;
    orbx::Layout::Slot<uint32_t> fv_node, fv_feat;
    orbx::Layout::Slot<uint8_t> desc;
    orbx::Layout::Slot<orbx_keypoint> kps;
    void reserve(orbx::Layout& L, const BowStore& s, bool rows_upload) {
        const size_t nfeat = (size_t)s.nrows * s.cap;
        nt = L.add<int32_t>(s.nrows); nfv = L.add<int32_t>(s.nrows);
        kps = L.add<orbx_keypoint>(nfeat, rows_upload); desc = L.add<uint8_t>(nfeat * 32, rows_upload);
        fv_node = L.add<uint32_t>(nfeat, rows_upload); fv_off = L.add<int32_t>((size_t)s.nrows * (s.cap + 1), rows_upload); fv_feat = L.add<uint32_t>(nfeat, rows_upload);
    }
    // copies the caller's host arrays into the pinned block h and names them inside the device block d; rows that are not part of the block are
    // passed through
    BowStore put(uint8_t* h, uint8_t* d, const BowStore& s) const {
        using orbx::Layout;
        const size_t nfeat = (size_t)s.nrows * s.cap;
        return {Layout::put(h, d, kps, s.kps, nfeat), Layout::put(h, d, desc, s.desc, nfeat * 32), Layout::put(h, d, nt, s.nt, (size_t)s.nrows),
                Layout::put(h, d, fv_node, s.fv_node, nfeat), Layout::put(h, d, fv_off, s.fv_off, (size_t)s.nrows * (s.cap + 1)),
                Layout::put(h, d, fv_feat, s.fv_feat, nfeat), Layout::put(h, d, nfv, s.nfv, (size_t)s.nrows), s.nrows, s.cap};
    }
};

// The block of orbs_bow_rows_search and orbs_tri_rows_search:
//   up    [pair | F12 | qvalid | claimed | nt | nfv | kps | desc | fv_node | fv_off | fv_feat]   (absent: F12 when the pairs carry none, the flags
//                                                                                                the caller passes none of, the rows' five large arrays)
//   down  [nmatches | q2t | t2q | best | second]                                                 (absent: the outputs the caller wants none of)
// behind it, device memory only: the records between the two kernels
struct RowsBlock : StoreSlots {
    orbx::Layout L;
    orbx::Layout::Slot<int32_t> pair, nmatches, q2t, t2q, best, second;
    orbx::Layout::Slot<uint8_t> qvalid, claimed;
    orbx::Layout::Slot<float> F12;
    orbx::Layout::Slot<BowRec> rec;
    int npairs;
    size_t nent, nqv;                                  // npairs * cap, bytes of qvalid
    RowsBlock(const RowPairs& p, const BowStore& s, const BowOut& o, bool rows_upload)
        : npairs(p.npairs), nent((size_t)p.npairs * s.cap), nqv(tri_qvalid_bytes(p, s.cap)) {
        pair = L.add<int32_t>(2 * (size_t)npairs); F12 = L.add<float>(9 * (size_t)npairs, p.F12 != nullptr);
        qvalid = L.add<uint8_t>(nqv, p.qvalid != nullptr); claimed = L.add<uint8_t>(nent, p.claimed != nullptr);
        reserve(L, s, rows_upload);
        L.end_upload();
        nmatches = L.add<int32_t>(npairs);
        q2t = L.add<int32_t>(nent, o.q2t != nullptr); t2q = L.add<int32_t>(nent, o.t2q != nullptr);
        best = L.add<int32_t>(nent, o.best != nullptr); second = L.add<int32_t>(nent, o.second != nullptr);
        L.end_download();
        rec = L.add<BowRec>(nent);
    }
    // copies the caller's host arrays into the pinned block h and names everything inside the device block d
    BowRows stage(uint8_t* h, uint8_t* d, const RowPairs& p, const BowStore& s) const {
        using orbx::Layout;
        BowRows a;
        a.P = {Layout::put(h, d, pair, p.pair, 2 * (size_t)npairs), npairs, Layout::put(h, d, qvalid, p.qvalid, nqv), p.qstride,
               Layout::put(h, d, claimed, p.claimed, nent), Layout::put(h, d, F12, p.F12, 9 * (size_t)npairs), 0, 0};
        a.S = put(h, d, s);
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

// ---- what the entry points keep, and the two forms of a search ----------------------------------------------------------------------------

// Per device: the records of the device forms, the block of the host forms, and the event chain that orders the calls which share them across
// their callers' streams.  Grown on first use and kept for the life of the process.  Tag: the translation unit's own type, so that SearchByBoW and
// SearchForTriangulation keep separate instances and their calls are not ordered against each other.
template <class Tag>
struct RowsKeep {
    std::mutex mu;
    int device = 0;
    hipStream_t own = nullptr;          // a NULL stream is the device's default stream
    orbx::Chain chain;
    std::string err;
    orbx::DevBuf rec;
    orbx::Block block;
    static RowsKeep* get() {
        static std::mutex mu;
        static std::map<int, std::unique_ptr<RowsKeep>> keeps;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        std::lock_guard<std::mutex> lk(mu);
        std::unique_ptr<RowsKeep>& k = keeps[dev];
        if (!k) {
            std::unique_ptr<RowsKeep> n(new RowsKeep);
            n->device = dev;
            if (n->chain.ev.ensure() != hipSuccess) return nullptr;
            k = std::move(n);
        }
        return k.get();
    }
    // the records hold `need` bytes; the first call of a size waits for the chain, since earlier calls may still use the old records
    int ensure_rec(size_t need) {
        if (rec.size() >= need) return ORBX_OK;
        HIPCHK(this, chain.wait());
        HIPCHK(this, rec.ensure(orbx::doubled(rec.size(), need)));
        return ORBX_OK;
    }
};

// The device form of a search whose arguments the caller has checked: everything is device memory, the records are the kept ones, and
// launch(rows, stream) -> hipError_t enqueues the two kernels behind the keep's earlier calls.
template <class Tag, class Launch>
int rows_device_form(const RowPairs& P, const BowStore& S, const BowOut& O, void* stream, Launch launch) {
    RowsKeep<Tag>* m = RowsKeep<Tag>::get();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<RowsKeep<Tag>> c(m, stream);
    TRY(m->ensure_rec((size_t)P.npairs * S.cap * sizeof(BowRec)));
    TRY(c.begin());
    HIPCHK(m, launch(BowRows{S, P, O, m->rec.template as<BowRec>()}, c.st));
    return c.end();
}

// The synchronous host form: the caller's host arrays go through the kept block (rows_upload: the store's large arrays too), and the outputs
// the caller asked for come back.
template <class Tag, class Launch>
int rows_host_form(const RowPairs& P, const BowStore& S, const BowOut& O, bool rows_upload, void* stream, Launch launch) {
    RowsKeep<Tag>* m = RowsKeep<Tag>::get();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<RowsKeep<Tag>> c(m, stream);
    const RowsBlock B(P, S, O, rows_upload);
    orbx::Staged<RowsKeep<Tag>> s(c, m->block, B.L);
    TRY(s.fit());
    const BowRows a = B.stage(s.h, s.d, P, S);
    TRY(s.run([&]() -> int {
        HIPCHK(m, launch(a, c.st));
        return ORBX_OK;
    }));
    B.unpack(s.h, O);
    return ORBX_OK;
}

// ---- the chain of orbt_new_points_rows* ------------------------------------------------------------------------------------------------

// what k_triangulate writes per pair (include/orbt.h), pair p at + p*cap resp. + p*ocap
struct NewPointsOut {
    uint8_t* status;
    float *x3d, *v;
    int32_t *match12, *acc_idx;
    float* acc_x3d;
    int32_t *count, *overflow;
    int ocap;
};

// The HOST list of pairs of the chain: rows in range, one query row (the pairs share its "no map point yet" flags), train rows distinct from each
// other and from the query row (a row searched twice, or on both sides, would not see what the earlier triangulation accepted on its other side).
inline int check_chain_pairs(const int32_t* pair, int npairs, int nrows) {
    if (npairs < 0 || npairs > ORBT_MAX_PAIRS) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    if (!pair) return ORBX_ERR_ARG;
    for (int p = 0; p < npairs; p++) {
        const int q = pair[2 * p], t = pair[2 * p + 1];
        if (q < 0 || q >= nrows || t < 0 || t >= nrows || q != pair[0] || t == q) return ORBX_ERR_ARG;
        for (int o = 0; o < p; o++)
            if (pair[2 * o + 1] == t) return ORBX_ERR_ARG;
    }
    return ORBX_OK;
}

inline int check_new_points(const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* pairs, const RowPairs& P, const BowStore& S,
                            const BowOut& O, const NewPointsOut& N, const float* factors1, const float* sigma2_1, const float* factors2,
                            const float* sigma2_2, int nlevels, bool on_device, bool rows_device) {
    if (!factors1 || !sigma2_1 || !factors2) return ORBX_ERR_ARG;
    int rc = check_tri_rows(prm, P, S, O, sigma2_2, nlevels, on_device, rows_device);
    if (rc != ORBX_OK) return rc;
    if (P.qstride != 0 || N.ocap < 1 || !below_2g((long long)npairs * N.ocap * 3) || !below_2g((long long)npairs * S.cap * 4)) return ORBX_ERR_ARG;
    if ((rc = check_chain_pairs(pair, npairs, S.nrows)) != ORBX_OK || npairs == 0) return rc;
    if (!pairs || !P.qvalid || !P.claimed || !O.q2t || !N.status || !N.x3d || !N.match12 || !N.acc_idx || !N.acc_x3d || !N.count || !N.overflow)
        return ORBX_ERR_ARG;
    auto misaligned = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };
    if (on_device && (misaligned(pairs, 4) || misaligned(N.x3d, 4) || misaligned(N.v, 16) || misaligned(N.match12, 4) || misaligned(N.acc_idx, 4) ||
                      misaligned(N.acc_x3d, 4) || misaligned(N.count, 4) || misaligned(N.overflow, 4)))
        return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The block of orbt_new_points_rows:
//   up    [pairs | F12 | qvalid | claimed | nt | nfv | kps | desc | fv_node | fv_off | fv_feat]
//   down  [qvalid' | claimed' | nmatches | count | overflow | q2t | t2q | status | x3d | v | match12 | acc_idx | acc_x3d]
// The chain updates the two flag arrays in place: they go up in the first span, are copied on the device into the second (qvalid', claimed'), and
// the kernels work on those.  Behind it, device memory only: the records of one pair.
struct NewPointsBlock : StoreSlots {
    orbx::Layout L;
    orbx::Layout::Slot<orbt_pair> pairs;
    orbx::Layout::Slot<float> F12, x3d, v, acc_x3d;
    orbx::Layout::Slot<uint8_t> qvalid, claimed, qvalid_out, claimed_out, status;
    orbx::Layout::Slot<int32_t> nmatches, count, overflow, q2t, t2q, match12, acc_idx;
    orbx::Layout::Slot<BowRec> rec;
    int npairs, cap;
    size_t nent, nacc;                                 // npairs * cap, npairs * ocap
    NewPointsBlock(int npairs_, const BowStore& s, bool want_t2q, bool want_v, int ocap, bool rows_upload)
        : npairs(npairs_), cap(s.cap), nent((size_t)npairs_ * s.cap), nacc((size_t)npairs_ * ocap) {
        pairs = L.add<orbt_pair>(npairs); F12 = L.add<float>(9 * (size_t)npairs);
        qvalid = L.add<uint8_t>(cap); claimed = L.add<uint8_t>(nent);
        reserve(L, s, rows_upload);
        L.end_upload();
        qvalid_out = L.add<uint8_t>(cap); claimed_out = L.add<uint8_t>(nent);
        nmatches = L.add<int32_t>(npairs); count = L.add<int32_t>(npairs); overflow = L.add<int32_t>(npairs);
        q2t = L.add<int32_t>(nent); t2q = L.add<int32_t>(nent, want_t2q);
        status = L.add<uint8_t>(nent); x3d = L.add<float>(nent * 3); v = L.add<float>(nent * 4, want_v);
        match12 = L.add<int32_t>(nent); acc_idx = L.add<int32_t>(nacc * 2); acc_x3d = L.add<float>(nacc * 3);
        L.end_download();
        rec = L.add<BowRec>(cap);
    }
};

}  // namespace orbs
#pragma GCC visibility pop
