// ORBmatcher::SearchByBoW (reference src/ORBmatcher.cc:155-281 key frame / frame, :715-850 key frame / key frame) over the rows of a resident
// key-frame store, every (query row, train row) pair of a call in one launch.  include/orbs.h is the boundary (ORBS_RULE_BOW states the rule);
// orbs_rows.h holds the host side.
//
// A feature lies under exactly one node of its FeatureVector, and the "already matched" state a query sees can only have been written by earlier
// queries of the same node: every common node is an independent small greedy problem, and only the rotation histogram and the count join them.
//
// k_bow_rows: a flat grid over (pair, query node), one WAVE per node, four per workgroup, no LDS and no barrier: rows_node_walk of
//   orbs_rows_device.h (the binary search of the node in the train row, the train run in 64-entry chunks, the claim bits in registers, one
//   record per list position of the query row) with BowRule.  A lane keeps the two smallest keys (distance << 16 | list position) of its
//   positions; the wave minimum, taken twice (the owner of the first steps to its second key in between), gives exactly the reference's
//   bestDist1 / bestDist2 with the first listed candidate on ties.
// k_bow_rows_finish: one workgroup per pair behind it on the same stream: rows_finish of orbs_rows_device.h, which the triangulation search over
//   rows (orbs_tri_rows.hip) ends with too.
#include <hip/hip_runtime.h>

#include <climits>

#include "orbs.h"
#include "orbs_rows.h"
#include "orbs_rows_device.h"

namespace orbs {

// The rule of SearchByBoW: nothing is held of a train key point or of a query beyond their descriptors; candidates are keyed by LIST POSITION.
struct BowRule {
    static constexpr bool by_feature = false;
    int th;
    float ratio;
    struct Held {};
    struct Query { __device__ Query of_lane(int) const { return {}; } };
    __device__ Held hold(const orbx_keypoint&) const { return {}; }
    __device__ Query query(const orbx_keypoint&) const { return {}; }
    struct Acc {
        uint32_t k1 = KEY_NONE, k2 = KEY_NONE;                           // the lane's two smallest keys
        template <class GetHeld>
        __device__ __forceinline__ void offer(uint32_t dist, uint32_t, int pos, GetHeld, const Query&, const BowRule&) {
            const uint32_t key = (dist << 16) | (uint32_t)pos;
            if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
        }
    };
    __device__ __forceinline__ RowsPick resolve(Acc& a, int lane) const {
        const uint32_t kb = wave_min_u32(a.k1);
        if (kb != KEY_NONE && lane == (int)(kb & 63)) a.k1 = a.k2;       // list position c*64 + lane: the owner steps to its second key
        const uint32_t ks = wave_min_u32(a.k1);
        const int bd = kb == KEY_NONE ? INT_MAX : (int)(kb >> 16), sd = ks == KEY_NONE ? INT_MAX : (int)(ks >> 16);
        const bool take = bd <= th && (float)bd < ratio * (float)sd;     // :224-226 / :793-795 (th = TH_LOW - 1 there)
        return {bd, sd, take ? (int)(kb & 0xFFFFu) : -1, -1};
    }
};

__global__ __launch_bounds__(ROWS_WAVES * 64) void k_bow_rows(orbs_params prm, BowRows a, int blocks_per_pair) {
    const int p = (int)(blockIdx.x / (unsigned)blocks_per_pair);
    const int j = uni((int)(blockIdx.x % (unsigned)blocks_per_pair) * ROWS_WAVES + (int)(threadIdx.x >> 6));         // the query node of this wave
    const int cap = a.S.cap;
    const int qr = a.P.pair[2 * p], tr = a.P.pair[2 * p + 1];
    if ((unsigned)qr >= (unsigned)a.S.nrows || (unsigned)tr >= (unsigned)a.S.nrows) return;      // the pair finds nothing: k_bow_rows_finish says so
    if (j >= clampi(a.S.nfv[qr], 0, cap)) return;
    rows_node_walk(a.S, p, qr, tr, j, a.P.claimed ? a.P.claimed + (size_t)p * cap : nullptr, a.P.qvalid ? a.P.qvalid + (size_t)p * a.P.qstride : nullptr,
                   prm.check_orientation != 0, a.rec, BowRule{prm.th, prm.ratio});
}

__global__ __launch_bounds__(ROWS_FINISH_TPB) void k_bow_rows_finish(orbs_params prm, BowRows a) {
    const int p = blockIdx.x;
    rows_finish<ROWS_FINISH_TPB>(prm.check_orientation != 0, a.S, a.P.pair[2 * p], a.P.pair[2 * p + 1], a.O, a.rec, p);
}

static hipError_t launch_bow_rows(const orbs_params& prm, const BowRows& a, hipStream_t st) {
    const int bpp = rows_blocks_per_pair(a.S.cap);
    k_bow_rows<<<dim3((unsigned)a.P.npairs * (unsigned)bpp), ROWS_WAVES * 64, 0, st>>>(prm, a, bpp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_bow_rows_finish<<<dim3((unsigned)a.P.npairs), ROWS_FINISH_TPB, 0, st>>>(prm, a);
    return hipGetLastError();
}

struct BowKeep;                        // this translation unit's RowsKeep: its records, block and chain are not those of orbs_tri_rows.hip

}  // namespace orbs

extern "C" {

int orbs_bow_rows_search_batch_device(const orbs_params* prm, const int32_t* d_pair, int npairs, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                      const int32_t* d_nt, const uint32_t* d_fv_node, const int32_t* d_fv_off, const uint32_t* d_fv_feat,
                                      const int32_t* d_nfv, int nrows, int cap, const uint8_t* d_qvalid, const uint8_t* d_claimed, int32_t* d_q2t,
                                      int32_t* d_t2q, int32_t* d_best, int32_t* d_second, int32_t* d_nmatches, void* stream) {
    using namespace orbs;
    const RowPairs P{d_pair, npairs, d_qvalid, cap, d_claimed, nullptr, 0, 0};
    const BowStore S{d_kps, d_desc, d_nt, d_fv_node, d_fv_off, d_fv_feat, d_nfv, nrows, cap};
    const BowOut O{d_q2t, d_t2q, d_best, d_second, d_nmatches};
    if (check_bow_rows(prm, P, S, O, true, true) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    orbs_params prm2 = *prm;
    prm2.check_orientation = prm->check_orientation ? 1 : 0;
    return rows_device_form<BowKeep>(P, S, O, stream, [&](const BowRows& a, hipStream_t st) { return launch_bow_rows(prm2, a, st); });
}

int orbs_bow_rows_search(const orbs_params* prm, const int32_t* pair, int npairs, const orbx_keypoint* kps, const uint8_t* desc, const int32_t* nt,
                         const uint32_t* fv_node, const int32_t* fv_off, const uint32_t* fv_feat, const int32_t* nfv, int nrows, int cap,
                         int rows_on_device, const uint8_t* qvalid, const uint8_t* claimed, int32_t* q2t, int32_t* t2q, int32_t* best, int32_t* second,
                         int32_t* nmatches, void* stream) {
    using namespace orbs;
    const RowPairs P{pair, npairs, qvalid, cap, claimed, nullptr, 0, 0};
    const BowStore S{kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap};
    const BowOut O{q2t, t2q, best, second, nmatches};
    if (check_bow_rows(prm, P, S, O, false, rows_on_device != 0) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    orbs_params prm2 = *prm;
    prm2.check_orientation = prm->check_orientation ? 1 : 0;
    return rows_host_form<BowKeep>(P, S, O, rows_on_device == 0, stream, [&](const BowRows& a, hipStream_t st) { return launch_bow_rows(prm2, a, st); });
}

}  // extern "C"
