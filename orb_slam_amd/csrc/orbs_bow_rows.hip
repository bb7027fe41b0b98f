// ORBmatcher::SearchByBoW (reference src/ORBmatcher.cc:155-281 key frame / frame, :715-850 key frame / key frame) over the rows of a resident
// key-frame store, every (query row, train row) pair of a call in one launch.  include/orbs.h is the boundary (ORBS_RULE_BOW states the rule);
// orbs_bow_rows.h holds the host side.
//
// A feature lies under exactly one node of its FeatureVector, and the "already matched" state a query sees can only have been written by earlier
// queries of the same node: every common node is an independent small greedy problem, and only the rotation histogram and the count join them.
//
// k_bow_rows: a flat grid over (pair, query node), one WAVE per node, four per workgroup, no LDS and no barrier.  The wave finds its node in the
//   train row's ascending fv_node by binary search (what k_bow_ranges does for the list search) and resolves the node's queries in list order
//   against the node's train run.  The run is scanned in 64-entry chunks, lane l taking list positions l, l + 64, ... : this is the path for nodes
//   of every size (a three-level vocabulary puts hundreds of features under one node); there is no workgroup-wide form.  A run of up to 64
//   entries (the usual case: about ten) keeps its features and descriptors in registers for all queries; a longer one reads them again per
//   query through L2.  The claim state is one bit per list position: lane c holds the 64-bit masks of chunks c and c + 64 (cap <= 8192 gives at
//   most 128 chunks), read by readlane, so nothing of it is in memory.  Positions behind the run, features outside the train row and features
//   claimed on entry start out set.  A lane keeps the two smallest keys (distance << 16 | list position) of its positions; the wave minimum, taken
//   twice (the owner of the first steps to its second key in between), gives exactly the reference's bestDist1 / bestDist2 with the first
//   listed candidate on ties.  Queries are loaded 64 at a time, one per lane, and broadcast by readlane; a lane collects its query's result and
//   stores ONE 16-byte record per list position of the query row (a node without a partner stores "never visited"), so the records of a pair
//   are complete without having been initialised.
// k_bow_rows_finish: one workgroup per pair behind it on the same stream: rows_finish of orbs_rows_device.h, which the triangulation search over
//   rows (orbs_tri_rows.hip) ends with too.
#include <hip/hip_runtime.h>

#include <climits>
#include <map>
#include <memory>
#include <mutex>

#include "orbs.h"
#include "orbs_bow_rows.h"
#include "orbs_rows_device.h"

namespace orbs {

__global__ __launch_bounds__(BOW_ROWS_WAVES * 64) void k_bow_rows(orbs_params prm, BowRows a, int blocks_per_pair) {
    const int lane = threadIdx.x & 63;
    const int p = (int)(blockIdx.x / (unsigned)blocks_per_pair);
    const int j = uni((int)(blockIdx.x % (unsigned)blocks_per_pair) * BOW_ROWS_WAVES + (int)(threadIdx.x >> 6));     // the query node of this wave
    const int cap = a.S.cap;
    const int qr = a.P.pair[2 * p], tr = a.P.pair[2 * p + 1];
    if ((unsigned)qr >= (unsigned)a.S.nrows || (unsigned)tr >= (unsigned)a.S.nrows) return;      // the pair finds nothing: k_bow_rows_finish says so
    if (j >= clampi(a.S.nfv[qr], 0, cap)) return;
    const int32_t* qo = a.S.fv_off + (size_t)qr * (cap + 1);
    const uint32_t* qf = a.S.fv_feat + (size_t)qr * cap;
    const uint32_t* tn = a.S.fv_node + (size_t)tr * cap;
    const int32_t* to = a.S.fv_off + (size_t)tr * (cap + 1);
    const uint32_t* tf = a.S.fv_feat + (size_t)tr * cap;
    const int ntq = clampi(a.S.nt[qr], 0, cap), ntt = clampi(a.S.nt[tr], 0, cap), nft = clampi(a.S.nfv[tr], 0, cap);
    const int q0 = clampi(qo[j], 0, cap), q1 = clampi(qo[j + 1], q0, cap);

    // the node in the train row (both node lists ascend): replaces the merge walk
    const uint32_t node = a.S.fv_node[(size_t)qr * cap + j];
    int lo = 0, hi = nft;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (tn[mid] < node) lo = mid + 1; else hi = mid; }
    const bool common = lo < nft && tn[lo] == node;
    int t0 = 0, t1 = 0;
    if (common) { t0 = clampi(to[lo], 0, cap); t1 = clampi(to[lo + 1], t0, cap); }
    const int T = t1 - t0, nchunks = (T + 63) >> 6;
    const bool single = nchunks <= 1;
    const uint8_t* claimed = a.P.claimed ? a.P.claimed + (size_t)p * cap : nullptr;
    const uint4* tdesc = reinterpret_cast<const uint4*>(a.S.desc) + (size_t)tr * cap * 2;
    const uint4* qdesc = reinterpret_cast<const uint4*>(a.S.desc) + (size_t)qr * cap * 2;

    // claim state on entry; for a run of one chunk its features and descriptors stay in registers
    unsigned long long cm0 = 0, cm1 = 0;
    int tidx = -1;
    uint4 td0 = make_uint4(0, 0, 0, 0), td1 = td0;
    for (int c = 0; c < max(nchunks, 1); ++c) {                           // (an empty run: one chunk with every position taken)
        const int pos = c * 64 + lane;
        bool taken = true;
        if (pos < T) {
            const uint32_t f = tf[t0 + pos];
            if (f < (uint32_t)ntt) {
                taken = claimed && claimed[f] != 0;
                if (single) { tidx = (int)f; td0 = tdesc[2 * f]; td1 = tdesc[2 * f + 1]; }
            }
        }
        const unsigned long long m = __ballot(taken);
        if (lane == (c & 63)) { if (c < 64) cm0 = m; else cm1 = m; }
    }

    const bool rot = prm.check_orientation != 0;
    for (int qc = q0; qc < q1; qc += 64) {
        // this chunk's queries, one per lane
        const int k = qc + lane;
        int idx1 = -1;
        bool valid = false;
        uint4 qd0 = make_uint4(0, 0, 0, 0), qd1 = qd0;
        if (k < q1) {
            const uint32_t f = qf[k];
            if (f < (uint32_t)ntq) {
                idx1 = (int)f;
                valid = common && (!a.P.qvalid || a.P.qvalid[(size_t)p * cap + f] != 0);
                if (valid) { qd0 = qdesc[2 * f]; qd1 = qdesc[2 * f + 1]; }
            }
        }
        int r_idx2 = -1, r_best = -1, r_second = -1;
        unsigned long long todo = __ballot(valid);
        while (todo) {                                                   // in list order; everything below is wave-uniform but the keys
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint4 b0 = lane_u4(qd0, l), b1 = lane_u4(qd1, l);
            uint32_t k1 = KEY_NONE, k2 = KEY_NONE;                       // the lane's two smallest keys
            if (single) {
                const unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(cm0 >> 32), 0) << 32) |
                                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cm0, 0);
                if (!((m >> lane) & 1)) k1 = (hamming_key(td0, td1, b0, b1) << 16) | (uint32_t)lane;
            } else {
                for (int c = 0; c < nchunks; ++c) {
                    const unsigned long long cm = c < 64 ? cm0 : cm1;
                    const unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(cm >> 32), c & 63) << 32) |
                                                 (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cm, c & 63);
                    if ((m >> lane) & 1) continue;                       // claimed, outside the row or behind the run: nothing is read
                    const int pos = c * 64 + lane;
                    const uint32_t f = tf[t0 + pos];
                    const uint32_t key = (hamming_key(tdesc[2 * f], tdesc[2 * f + 1], b0, b1) << 16) | (uint32_t)pos;
                    if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
                }
            }
            const uint32_t kb = wave_min_u32(k1);
            if (kb != KEY_NONE && lane == (int)(kb & 63)) k1 = k2;       // list position c*64 + lane: the owner steps to its second key
            const uint32_t ks = wave_min_u32(k1);
            const int bd = kb == KEY_NONE ? INT_MAX : (int)(kb >> 16), sd = ks == KEY_NONE ? INT_MAX : (int)(ks >> 16);
            int idx2 = -1;
            if (bd <= prm.th && (float)bd < prm.ratio * (float)sd) {     // :224-226 / :793-795 (th = TH_LOW - 1 there)
                const int bpos = (int)(kb & 0xFFFFu), c = bpos >> 6;
                idx2 = single ? __builtin_amdgcn_readlane(tidx, bpos) : (int)tf[t0 + bpos];
                if (lane == (c & 63)) { if (c < 64) cm0 |= 1ull << (bpos & 63); else cm1 |= 1ull << (bpos & 63); }
            }
            if (lane == l) { r_idx2 = idx2; r_best = bd; r_second = sd; }
        }
        if (k < q1) {
            int bin = 255;
            if (rot && r_idx2 >= 0) bin = rot_bin(a.S.kps[(size_t)qr * cap + idx1].angle, a.S.kps[(size_t)tr * cap + r_idx2].angle);
            a.rec[(size_t)p * cap + k] = BowRec{r_idx2, bin, r_best, r_second};
        }
    }
}

constexpr int BOW_FINISH_TPB = ROWS_FINISH_TPB;

__global__ __launch_bounds__(BOW_FINISH_TPB) void k_bow_rows_finish(orbs_params prm, BowRows a) {
    const int p = blockIdx.x;
    rows_finish<BOW_FINISH_TPB>(prm.check_orientation != 0, a.S, a.P.pair[2 * p], a.P.pair[2 * p + 1], a.O, a.rec, p);
}

static hipError_t launch_bow_rows(const orbs_params& prm, const BowRows& a, hipStream_t st) {
    const int bpp = bow_rows_blocks_per_pair(a.S.cap);
    k_bow_rows<<<dim3((unsigned)a.P.npairs * (unsigned)bpp), BOW_ROWS_WAVES * 64, 0, st>>>(prm, a, bpp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_bow_rows_finish<<<dim3((unsigned)a.P.npairs), BOW_FINISH_TPB, 0, st>>>(prm, a);
    return hipGetLastError();
}

// What the entry points keep per device: the records of the device form, the block of the host form, and the event chain that orders the calls
// which share them across their callers' streams.  Grown on first use and kept for the life of the process.
struct BowRowsKeep {
    std::mutex mu;
    int device = 0;
    hipStream_t own = nullptr;          // a NULL stream is the device's default stream
    orbx::Chain chain;
    std::string err;
    orbx::DevBuf rec;
    orbx::Block block;
};

static BowRowsKeep* bow_rows_keep() {
    static std::mutex mu;
    static std::map<int, std::unique_ptr<BowRowsKeep>> keeps;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    std::unique_ptr<BowRowsKeep>& k = keeps[dev];
    if (!k) {
        std::unique_ptr<BowRowsKeep> n(new BowRowsKeep);
        n->device = dev;
        if (n->chain.ev.ensure() != hipSuccess) return nullptr;
        k = std::move(n);
    }
    return k.get();
}

}  // namespace orbs

#define TRY(x) do { const int rc_ = (x); if (rc_ != ORBX_OK) return rc_; } while (0)

extern "C" {

int orbs_bow_rows_search_batch_device(const orbs_params* prm, const int32_t* d_pair, int npairs, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                      const int32_t* d_nt, const uint32_t* d_fv_node, const int32_t* d_fv_off, const uint32_t* d_fv_feat,
                                      const int32_t* d_nfv, int nrows, int cap, const uint8_t* d_qvalid, const uint8_t* d_claimed, int32_t* d_q2t,
                                      int32_t* d_t2q, int32_t* d_best, int32_t* d_second, int32_t* d_nmatches, void* stream) {
    using namespace orbs;
    const BowPairs P{d_pair, npairs, d_qvalid, d_claimed};
    const BowStore S{d_kps, d_desc, d_nt, d_fv_node, d_fv_off, d_fv_feat, d_nfv, nrows, cap};
    const BowOut O{d_q2t, d_t2q, d_best, d_second, d_nmatches};
    if (check_bow_rows(prm, P, S, O, true, true) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    BowRowsKeep* m = bow_rows_keep();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<BowRowsKeep> c(m, stream);
    const size_t need = (size_t)npairs * cap * sizeof(BowRec);
    if (m->rec.size() < need) {                                          // first call of this size: earlier calls may still use the old records
        HIPCHK(m, m->chain.wait());
        HIPCHK(m, m->rec.ensure(orbx::doubled(m->rec.size(), need)));
    }
    TRY(c.begin());
    orbs_params prm2 = *prm;
    prm2.check_orientation = prm->check_orientation ? 1 : 0;
    HIPCHK(m, launch_bow_rows(prm2, BowRows{S, P, O, m->rec.as<BowRec>()}, c.st));
    return c.end();
}

int orbs_bow_rows_search(const orbs_params* prm, const int32_t* pair, int npairs, const orbx_keypoint* kps, const uint8_t* desc, const int32_t* nt,
                         const uint32_t* fv_node, const int32_t* fv_off, const uint32_t* fv_feat, const int32_t* nfv, int nrows, int cap,
                         int rows_on_device, const uint8_t* qvalid, const uint8_t* claimed, int32_t* q2t, int32_t* t2q, int32_t* best, int32_t* second,
                         int32_t* nmatches, void* stream) {
    using namespace orbs;
    const BowPairs P{pair, npairs, qvalid, claimed};
    const BowStore S{kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap};
    const BowOut O{q2t, t2q, best, second, nmatches};
    if (check_bow_rows(prm, P, S, O, false, rows_on_device != 0) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    BowRowsKeep* m = bow_rows_keep();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<BowRowsKeep> c(m, stream);
    const BowRowsBlock B(P, S, O, rows_on_device == 0);
    orbx::Staged<BowRowsKeep> s(c, m->block, B.L);
    TRY(s.fit());
    const BowRows a = B.stage(s.h, s.d, P, S);
    orbs_params prm2 = *prm;
    prm2.check_orientation = prm->check_orientation ? 1 : 0;
    TRY(s.run([&]() -> int {
        HIPCHK(m, launch_bow_rows(prm2, a, c.st));
        return ORBX_OK;
    }));
    B.unpack(s.h, O);
    return ORBX_OK;
}

}  // extern "C"
