// Host side of orbs_tri_rows_search* (include/orbs.h) and orbt_new_points_rows* (include/orbt.h): what the kernels of orbs_tri_rows.hip read and
// write, the argument checks that need no GPU, and the layouts of the two synchronous host forms' blocks (one pinned copy up, one down).  The rows,
// the outputs and the records are those of orbs_bow_rows.h.  Plain C++: tests/_probe/tri_rows_host.cpp runs it on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbs.h"
#include "orbs_bow_rows.h"
#include "orbt.h"
#include "orbx_host.h"

#pragma GCC visibility push(hidden)
namespace orbs {

// The pairs searched over the rows.  pair == NULL: ONE pair, (qr0, tr0), passed by value (the per-neighbour launches of the chain).
// qvalid of pair p at + p*qstride (qstride 0: one array for all pairs), claimed and the outputs at + p*cap, F12 at + p*9.
struct TriPairs {
    const int32_t* pair;
    int npairs;
    const uint8_t* qvalid;
    int qstride;
    const uint8_t* claimed;
    const float* F12;
    int qr0, tr0;
};

struct TriRows {
    BowStore S;
    TriPairs P;
    BowOut O;
    BowRec* rec;                       // scratch: npairs * cap records (idx2, bin, BestDist, the distance taken)
    float epi_thr[ORBS_MAX_LEVELS];    // orbs_epipolar_bound per octave of the train key point
    int th, check_orientation;
};

constexpr int TRI_ROWS_WAVES = 4;      // (pair, node) waves of one workgroup of k_tri_rows: the grid is bow_rows_blocks_per_pair(cap) per pair

// bytes of qvalid the pairs address
inline size_t tri_qvalid_bytes(const TriPairs& P, int cap) { return P.qstride == 0 || P.npairs == 0 ? (size_t)cap : (size_t)(P.npairs - 1) * P.qstride + cap; }

// check_bow_rows with the triangulation rule: the same refusals, and those of the arguments SearchForTriangulation adds
inline int check_tri_rows(const orbs_params* prm, const TriPairs& P, const BowStore& S, const BowOut& O, const float* level_sigma2, int nlevels,
                          bool on_device, bool rows_device) {
    if (!prm || prm->rule != ORBS_RULE_TRIANGULATION || !level_sigma2 || nlevels < 1 || nlevels > ORBS_MAX_LEVELS) return ORBX_ERR_ARG;
    if (P.qstride != 0 && P.qstride < S.cap) return ORBX_ERR_ARG;
    orbs_params b = *prm;              // ratio is unused by the rule
    b.rule = ORBS_RULE_BOW;
    b.ratio = 0.0f;
    const int rc = check_bow_rows(&b, BowPairs{P.pair, P.npairs, P.qvalid, P.claimed}, S, O, on_device, rows_device);
    if (rc != ORBX_OK || P.npairs == 0) return rc;
    if (!below_2g((long long)P.npairs * P.qstride + S.cap)) return ORBX_ERR_ARG;
    if (!P.F12 || (on_device && ((uintptr_t)P.F12 & 3))) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// The block of orbs_tri_rows_search:
//   up    [pair | F12 | qvalid | claimed | nt | nfv | kps | desc | fv_node | fv_off | fv_feat]   (absent as in BowRowsBlock)
//   down  [nmatches | q2t | t2q | best | second]
// behind it, device memory only: the records between the two kernels
struct TriRowsBlock {
    orbx::Layout L;
    orbx::Layout::Slot<int32_t> pair, nt, nfv, fv_off, nmatches, q2t, t2q, best, second;
    orbx::Layout::Slot<uint32_t> fv_node, fv_feat;
    orbx::Layout::Slot<uint8_t> qvalid, claimed, desc;
    orbx::Layout::Slot<float> F12;
    orbx::Layout::Slot<orbx_keypoint> kps;
    orbx::Layout::Slot<BowRec> rec;
    int npairs, nrows;
    size_t nent, nfeat, nqv;                           // npairs * cap, nrows * cap, bytes of qvalid
    TriRowsBlock(const TriPairs& p, const BowStore& s, const BowOut& o, bool rows_upload)
        : npairs(p.npairs), nrows(s.nrows), nent((size_t)p.npairs * s.cap), nfeat((size_t)s.nrows * s.cap), nqv(tri_qvalid_bytes(p, s.cap)) {
        pair = L.add<int32_t>(2 * (size_t)npairs); F12 = L.add<float>(9 * (size_t)npairs);
        qvalid = L.add<uint8_t>(nqv, p.qvalid != nullptr); claimed = L.add<uint8_t>(nent, p.claimed != nullptr);
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
    // copies the caller's host arrays into the pinned block h and names everything inside the device block d (th, the bounds: the caller's)
    TriRows stage(uint8_t* h, uint8_t* d, const TriPairs& p, const BowStore& s) const {
        using orbx::Layout;
        TriRows a{};
        a.P = {Layout::put(h, d, pair, p.pair, 2 * (size_t)npairs), npairs, Layout::put(h, d, qvalid, p.qvalid, nqv), p.qstride,
               Layout::put(h, d, claimed, p.claimed, nent), Layout::put(h, d, F12, p.F12, 9 * (size_t)npairs), 0, 0};
        a.S = {Layout::put(h, d, kps, s.kps, nfeat), Layout::put(h, d, desc, s.desc, nfeat * 32), Layout::put(h, d, nt, s.nt, nrows),
               Layout::put(h, d, fv_node, s.fv_node, nfeat), Layout::put(h, d, fv_off, s.fv_off, (size_t)nrows * (s.cap + 1)),
               Layout::put(h, d, fv_feat, s.fv_feat, nfeat), Layout::put(h, d, nfv, s.nfv, nrows), s.nrows, s.cap};
        a.O = {Layout::at(d, q2t), Layout::at(d, t2q), Layout::at(d, best), Layout::at(d, second), Layout::at(d, nmatches)};
        a.rec = Layout::at(d, rec);
        return a;
    }
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

inline int check_new_points(const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* pairs, const TriPairs& P, const BowStore& S,
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
struct NewPointsBlock {
    orbx::Layout L;
    orbx::Layout::Slot<orbt_pair> pairs;
    orbx::Layout::Slot<float> F12, x3d, v, acc_x3d;
    orbx::Layout::Slot<uint8_t> qvalid, claimed, desc, qvalid_out, claimed_out, status;
    orbx::Layout::Slot<int32_t> nt, nfv, fv_off, nmatches, count, overflow, q2t, t2q, match12, acc_idx;
    orbx::Layout::Slot<uint32_t> fv_node, fv_feat;
    orbx::Layout::Slot<orbx_keypoint> kps;
    orbx::Layout::Slot<BowRec> rec;
    int npairs, nrows, cap, ocap;
    size_t nent, nfeat, nacc;
    NewPointsBlock(int npairs_, const BowStore& s, bool want_t2q, bool want_v, int ocap_, bool rows_upload)
        : npairs(npairs_), nrows(s.nrows), cap(s.cap), ocap(ocap_), nent((size_t)npairs_ * s.cap), nfeat((size_t)s.nrows * s.cap),
          nacc((size_t)npairs_ * ocap_) {
        pairs = L.add<orbt_pair>(npairs); F12 = L.add<float>(9 * (size_t)npairs);
        qvalid = L.add<uint8_t>(cap); claimed = L.add<uint8_t>(nent);
        nt = L.add<int32_t>(nrows); nfv = L.add<int32_t>(nrows);
        kps = L.add<orbx_keypoint>(nfeat, rows_upload); desc = L.add<uint8_t>(nfeat * 32, rows_upload);
        fv_node = L.add<uint32_t>(nfeat, rows_upload); fv_off = L.add<int32_t>((size_t)nrows * (cap + 1), rows_upload); fv_feat = L.add<uint32_t>(nfeat, rows_upload);
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
