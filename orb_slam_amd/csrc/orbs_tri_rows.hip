// ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:852-1014) over the rows of a resident key-frame store, and the chain
// search -> finish -> triangulate per neighbour of LocalMapping::CreateNewMapPoints over the same rows.  include/orbs.h and include/orbt.h are the
// boundary (ORBS_RULE_TRIANGULATION states the rule); orbs_tri_rows.h holds the host side.
//
// As in SearchByBoW (orbs_bow_rows.hip) a feature lies under exactly one node of its FeatureVector, and vbMatched2[idx2] is only read by queries of
// the node that wrote it: every common node is an independent greedy problem, and only the rotation histogram and the count join them.  What a
// query takes is the smallest (dist, idx2) among the candidates that are unclaimed, have dist <= th and lie on the query's epipolar line, provided
// its distance is at most 2 * BestDist, BestDist being the smallest distance among the unclaimed candidates with dist <= th, on the line or not:
// the reference walks its sorted vDistIndex up to DistTh = 2 * BestDist and takes the first entry that passes CheckDistEpipolarLine.  That is one
// epipolar test per lane and two wave minima; there is no sequential walk of a sorted list.
//
// k_tri_rows: a flat grid over (pair, query node), one WAVE per node, four per workgroup.  The wave finds its node in the train row's ascending
//   fv_node by binary search and resolves the node's queries in list order against the node's train run, scanned in 64-entry chunks, lane l
//   taking list positions l, l + 64, ... : one path for nodes of every size.  A run of up to 64 entries keeps its features, descriptors, key
//   point positions and epipolar bounds in registers for all queries; a longer one reads them again per query through L2.  The claim state is
//   one bit per list position, in registers, as in k_bow_rows.  A lane keeps its smallest distance and its smallest passing key
//   (distance << 16 | idx2: keyed by FEATURE, which is the order of the reference's sort, so the list need not ascend within a node).  Queries
//   are loaded 64 at a time, one per lane, each lane computing its query's line l = x1' F12 once; a lane collects its query's result and stores ONE
//   16-byte record per list position of the query row (idx2, rotation bin, BestDist, the distance taken; "never visited" for a node without a
//   partner), so the records of a pair are complete without having been initialised.  The only LDS is the 16-entry table of epipolar bounds.
// k_tri_rows_finish: one workgroup per pair behind it on the same stream: rows_finish of orbs_rows_device.h.
// The chain enqueues, per neighbour, k_tri_rows and k_tri_rows_finish for ONE pair given by value and the unchanged k_triangulate
// (orbt_triangulate_batch_device with row-offset pointers), which clears / sets the two flag arrays the next neighbour's search reads.
#include <hip/hip_runtime.h>

#include <climits>
#include <map>
#include <memory>
#include <mutex>

#include "orbs.h"
#include "orbs_rows_device.h"
#include "orbs_tri_rows.h"
#include "orbt.h"

namespace orbs {

__global__ __launch_bounds__(TRI_ROWS_WAVES * 64) void k_tri_rows(TriRows a, int blocks_per_pair) {
    __shared__ float thr[ORBS_MAX_LEVELS];
#pragma unroll
    for (int i = 0; i < ORBS_MAX_LEVELS; ++i) if (threadIdx.x == i) thr[i] = a.epi_thr[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int p = (int)(blockIdx.x / (unsigned)blocks_per_pair);
    const int j = uni((int)(blockIdx.x % (unsigned)blocks_per_pair) * TRI_ROWS_WAVES + (int)(threadIdx.x >> 6));     // the query node of this wave
    const int cap = a.S.cap;
    const int qr = a.P.pair ? a.P.pair[2 * p] : a.P.qr0, tr = a.P.pair ? a.P.pair[2 * p + 1] : a.P.tr0;
    if ((unsigned)qr >= (unsigned)a.S.nrows || (unsigned)tr >= (unsigned)a.S.nrows) return;      // the pair finds nothing: k_tri_rows_finish says so
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
    const uint8_t* qvalid = a.P.qvalid ? a.P.qvalid + (size_t)p * a.P.qstride : nullptr;
    const uint4* tdesc = reinterpret_cast<const uint4*>(a.S.desc) + (size_t)tr * cap * 2;
    const uint4* qdesc = reinterpret_cast<const uint4*>(a.S.desc) + (size_t)qr * cap * 2;
    const orbx_keypoint* tkp = a.S.kps + (size_t)tr * cap;
    const orbx_keypoint* qkp = a.S.kps + (size_t)qr * cap;
    float F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = a.P.F12[(size_t)p * 9 + i];

    // claim state on entry; for a run of one chunk its features, descriptors, positions and bounds stay in registers
    unsigned long long cm0 = 0, cm1 = 0;
    int tidx = -1;
    uint4 td0 = make_uint4(0, 0, 0, 0), td1 = td0;
    float tx = 0.f, ty = 0.f, tthr = 0.f;
    for (int c = 0; c < max(nchunks, 1); ++c) {                           // (an empty run: one chunk with every position taken)
        const int pos = c * 64 + lane;
        bool taken = true;
        if (pos < T) {
            const uint32_t f = tf[t0 + pos];
            if (f < (uint32_t)ntt) {
                taken = claimed && claimed[f] != 0;                       // `if(vbMatched2[idx2] || pMP2) continue;`
                if (single) {
                    tidx = (int)f; td0 = tdesc[2 * f]; td1 = tdesc[2 * f + 1];
                    tx = tkp[f].x; ty = tkp[f].y; tthr = thr[epi_level(tkp[f].octave)];
                }
            }
        }
        const unsigned long long m = __ballot(taken);
        if (lane == (c & 63)) { if (c < 64) cm0 = m; else cm1 = m; }
    }

    const bool rot = a.check_orientation != 0;
    for (int qc = q0; qc < q1; qc += 64) {
        // this chunk's queries, one per lane, each with its epipolar line
        const int k = qc + lane;
        int idx1 = -1;
        bool valid = false;
        uint4 qd0 = make_uint4(0, 0, 0, 0), qd1 = qd0;
        EpiLine E{0.f, 0.f, 0.f, 0.f, a.th};
        if (k < q1) {
            const uint32_t f = qf[k];
            if (f < (uint32_t)ntq) {
                idx1 = (int)f;
                valid = common && (!qvalid || qvalid[f] != 0);             // `if(pMP1) continue;`
                if (valid) { qd0 = qdesc[2 * f]; qd1 = qdesc[2 * f + 1]; E = epi_line(qkp[f].x, qkp[f].y, F, a.th); }
            }
        }
        int r_idx2 = -1, r_best = -1, r_taken = -1;
        unsigned long long todo = __ballot(valid);
        while (todo) {                                                   // in list order; everything below is wave-uniform but the keys
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint4 b0 = lane_u4(qd0, l), b1 = lane_u4(qd1, l);
            const EpiLine e{lane_f(E.a, l), lane_f(E.b, l), lane_f(E.c, l), lane_f(E.den, l), a.th};
            uint32_t md = KEY_NONE, mk = KEY_NONE;                       // the lane's smallest distance, its smallest key ON the line
            int mpos = 0;                                                // the list position of mk
            if (single) {
                const unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(cm0 >> 32), 0) << 32) |
                                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cm0, 0);
                if (!((m >> lane) & 1)) {
                    const uint32_t d = hamming_key(td0, td1, b0, b1);
                    if ((int)d <= a.th) {                                // `if(dist>TH_LOW) continue;`
                        md = d;
                        if (epi_ok(e, tx, ty, tthr)) { mk = (d << 16) | (uint32_t)tidx; mpos = lane; }
                    }
                }
            } else {
                for (int c = 0; c < nchunks; ++c) {
                    const unsigned long long cm = c < 64 ? cm0 : cm1;
                    const unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(cm >> 32), c & 63) << 32) |
                                                 (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cm, c & 63);
                    if ((m >> lane) & 1) continue;                       // claimed, outside the row or behind the run: nothing is read
                    const int pos = c * 64 + lane;
                    const uint32_t f = tf[t0 + pos];
                    const uint32_t d = hamming_key(tdesc[2 * f], tdesc[2 * f + 1], b0, b1);
                    if ((int)d > a.th) continue;
                    md = min(md, d);
                    const uint32_t key = (d << 16) | f;
                    if (key < mk && epi_ok(e, tkp[f].x, tkp[f].y, thr[epi_level(tkp[f].octave)])) { mk = key; mpos = pos; }
                }
            }
            const uint32_t kb = wave_min_u32(md);                        // BestDist = vDistIndex.front().first
            const uint32_t kw = wave_min_u32(mk);                        // the first entry of the sorted list that is on the line
            const int bd = kb == KEY_NONE ? INT_MAX : (int)kb;
            int idx2 = -1, dt = INT_MAX;
            if (kw != KEY_NONE && (int)(kw >> 16) <= 2 * bd) {           // `if(vDistIndex[id].first>DistTh) break;` (src/ORBmatcher.cc:927-957)
                const int owner = __ffsll((long long)__ballot(mk == kw)) - 1;
                const int bpos = __builtin_amdgcn_readlane(mpos, owner), c = bpos >> 6;
                idx2 = (int)(kw & 0xFFFFu);
                dt = (int)(kw >> 16);
                if (lane == (c & 63)) { if (c < 64) cm0 |= 1ull << (bpos & 63); else cm1 |= 1ull << (bpos & 63); }      // vbMatched2[idx2] = true
            }
            if (lane == l) { r_idx2 = idx2; r_best = bd; r_taken = dt; }
        }
        if (k < q1) {
            int bin = 255;
            if (rot && r_idx2 >= 0) bin = rot_bin(qkp[idx1].angle, tkp[r_idx2].angle);
            a.rec[(size_t)p * cap + k] = BowRec{r_idx2, bin, r_best, r_taken};
        }
    }
}

__global__ __launch_bounds__(ROWS_FINISH_TPB) void k_tri_rows_finish(TriRows a) {
    const int p = blockIdx.x;
    rows_finish<ROWS_FINISH_TPB>(a.check_orientation != 0, a.S, a.P.pair ? a.P.pair[2 * p] : a.P.qr0, a.P.pair ? a.P.pair[2 * p + 1] : a.P.tr0, a.O,
                                 a.rec, p);
}

static hipError_t launch_tri_rows(const TriRows& a, hipStream_t st) {
    const int bpp = bow_rows_blocks_per_pair(a.S.cap);
    k_tri_rows<<<dim3((unsigned)a.P.npairs * (unsigned)bpp), TRI_ROWS_WAVES * 64, 0, st>>>(a, bpp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_tri_rows_finish<<<dim3((unsigned)a.P.npairs), ROWS_FINISH_TPB, 0, st>>>(a);
    return hipGetLastError();
}

static void fill_params(TriRows& a, const orbs_params* prm, const float* level_sigma2, int nlevels) {
    for (int i = 0; i < ORBS_MAX_LEVELS; ++i) a.epi_thr[i] = orbs_epipolar_bound(level_sigma2[i < nlevels ? i : nlevels - 1]);
    a.th = prm->th;
    a.check_orientation = prm->check_orientation ? 1 : 0;
}

// What the entry points keep per device: the records of the device forms, the block of the host forms, and the event chain that orders the calls
// which share them across their callers' streams.  Grown on first use and kept for the life of the process.
struct TriRowsKeep {
    std::mutex mu;
    int device = 0;
    hipStream_t own = nullptr;          // a NULL stream is the device's default stream
    orbx::Chain chain;
    std::string err;
    orbx::DevBuf rec;
    orbx::Block block;
};

static TriRowsKeep* tri_rows_keep() {
    static std::mutex mu;
    static std::map<int, std::unique_ptr<TriRowsKeep>> keeps;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    std::unique_ptr<TriRowsKeep>& k = keeps[dev];
    if (!k) {
        std::unique_ptr<TriRowsKeep> n(new TriRowsKeep);
        n->device = dev;
        if (n->chain.ev.ensure() != hipSuccess) return nullptr;
        k = std::move(n);
    }
    return k.get();
}

// search p, finish p, triangulate p for p = 0 .. npairs-1 on st: nothing but launches.  `pair` is the HOST list; P, O and N name the device arrays
// of all pairs (P.qvalid shared, written by the triangulation; P.claimed per pair, written too).
static int enqueue_chain(TriRowsKeep* m, hipStream_t st, const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* d_pairs,
                         const TriPairs& P, const BowStore& S, const BowOut& O, const NewPointsOut& N, BowRec* rec, const float* factors1,
                         const float* sigma2_1, const float* factors2, const float* sigma2_2, int nlevels) {
    const size_t cap = (size_t)S.cap;
    TriRows a{};
    a.S = S;
    a.rec = rec;
    fill_params(a, prm, sigma2_2, nlevels);
    for (int p = 0; p < npairs; p++) {
        const int qr = pair[2 * p], tr = pair[2 * p + 1];
        const size_t e = (size_t)p * cap, o = (size_t)p * N.ocap;
        uint8_t* claimed = const_cast<uint8_t*>(P.claimed) + e;
        a.P = TriPairs{nullptr, 1, P.qvalid, 0, claimed, P.F12 + (size_t)p * 9, qr, tr};
        a.O = BowOut{O.q2t + e, O.t2q ? O.t2q + e : nullptr, nullptr, nullptr, O.nmatches + p};
        HIPCHK(m, launch_tri_rows(a, st));
        const int rc = orbt_triangulate_batch_device(d_pairs + p, 1, factors1, sigma2_1, factors2, sigma2_2, nlevels, S.kps + (size_t)qr * cap, S.nt + qr,
                                                     S.cap, 0, S.kps + (size_t)tr * cap, S.nt + tr, S.cap, O.q2t + e, nullptr, S.nt + qr, S.cap,
                                                     N.status + e, N.x3d + e * 3, N.v ? N.v + e * 4 : nullptr, N.match12 + e, N.acc_idx + o * 2,
                                                     N.acc_x3d + o * 3, N.count + p, N.overflow + p, N.ocap, const_cast<uint8_t*>(P.qvalid), claimed, st);
        if (rc != ORBX_OK) return rc;
    }
    return ORBX_OK;
}

}  // namespace orbs

#define TRY(x) do { const int rc_ = (x); if (rc_ != ORBX_OK) return rc_; } while (0)

extern "C" {

int orbs_tri_rows_search_batch_device(const orbs_params* prm, const int32_t* d_pair, int npairs, const float* d_F12, const float* level_sigma2,
                                      int nlevels, const orbx_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nt, const uint32_t* d_fv_node,
                                      const int32_t* d_fv_off, const uint32_t* d_fv_feat, const int32_t* d_nfv, int nrows, int cap,
                                      const uint8_t* d_qvalid, int qstride, const uint8_t* d_claimed, int32_t* d_q2t, int32_t* d_t2q, int32_t* d_best,
                                      int32_t* d_second, int32_t* d_nmatches, void* stream) {
    using namespace orbs;
    const TriPairs P{d_pair, npairs, d_qvalid, qstride, d_claimed, d_F12, 0, 0};
    const BowStore S{d_kps, d_desc, d_nt, d_fv_node, d_fv_off, d_fv_feat, d_nfv, nrows, cap};
    const BowOut O{d_q2t, d_t2q, d_best, d_second, d_nmatches};
    if (check_tri_rows(prm, P, S, O, level_sigma2, nlevels, true, true) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    TriRowsKeep* m = tri_rows_keep();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<TriRowsKeep> c(m, stream);
    const size_t need = (size_t)npairs * cap * sizeof(BowRec);
    if (m->rec.size() < need) {                                          // first call of this size: earlier calls may still use the old records
        HIPCHK(m, m->chain.wait());
        HIPCHK(m, m->rec.ensure(orbx::doubled(m->rec.size(), need)));
    }
    TRY(c.begin());
    TriRows a{S, P, O, m->rec.as<BowRec>(), {}, 0, 0};
    fill_params(a, prm, level_sigma2, nlevels);
    HIPCHK(m, launch_tri_rows(a, c.st));
    return c.end();
}

int orbs_tri_rows_search(const orbs_params* prm, const int32_t* pair, int npairs, const float* F12, const float* level_sigma2, int nlevels,
                         const orbx_keypoint* kps, const uint8_t* desc, const int32_t* nt, const uint32_t* fv_node, const int32_t* fv_off,
                         const uint32_t* fv_feat, const int32_t* nfv, int nrows, int cap, int rows_on_device, const uint8_t* qvalid, int qstride,
                         const uint8_t* claimed, int32_t* q2t, int32_t* t2q, int32_t* best, int32_t* second, int32_t* nmatches, void* stream) {
    using namespace orbs;
    const TriPairs P{pair, npairs, qvalid, qstride, claimed, F12, 0, 0};
    const BowStore S{kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap};
    const BowOut O{q2t, t2q, best, second, nmatches};
    if (check_tri_rows(prm, P, S, O, level_sigma2, nlevels, false, rows_on_device != 0) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    TriRowsKeep* m = tri_rows_keep();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<TriRowsKeep> c(m, stream);
    const TriRowsBlock B(P, S, O, rows_on_device == 0);
    orbx::Staged<TriRowsKeep> s(c, m->block, B.L);
    TRY(s.fit());
    TriRows a = B.stage(s.h, s.d, P, S);
    fill_params(a, prm, level_sigma2, nlevels);
    TRY(s.run([&]() -> int {
        HIPCHK(m, launch_tri_rows(a, c.st));
        return ORBX_OK;
    }));
    B.unpack(s.h, O);
    return ORBX_OK;
}

int orbt_new_points_rows_device(const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* d_pairs, const float* d_F12,
                                const float* factors1, const float* sigma2_1, const float* factors2, const float* sigma2_2, int nlevels,
                                const orbx_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nt, const uint32_t* d_fv_node,
                                const int32_t* d_fv_off, const uint32_t* d_fv_feat, const int32_t* d_nfv, int nrows, int cap, uint8_t* d_qvalid,
                                uint8_t* d_claimed, int32_t* d_q2t, int32_t* d_t2q, int32_t* d_nmatches, uint8_t* d_status, float* d_x3d, float* d_v,
                                int32_t* d_match12, int32_t* d_acc_idx, float* d_acc_x3d, int32_t* d_count, int32_t* d_overflow, int ocap,
                                void* stream) {
    using namespace orbs;
    const TriPairs P{pair, npairs, d_qvalid, 0, d_claimed, d_F12, 0, 0};
    const BowStore S{d_kps, d_desc, d_nt, d_fv_node, d_fv_off, d_fv_feat, d_nfv, nrows, cap};
    const BowOut O{d_q2t, d_t2q, nullptr, nullptr, d_nmatches};
    const NewPointsOut N{d_status, d_x3d, d_v, d_match12, d_acc_idx, d_acc_x3d, d_count, d_overflow, ocap};
    if (check_new_points(prm, pair, npairs, d_pairs, P, S, O, N, factors1, sigma2_1, factors2, sigma2_2, nlevels, true, true) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    TriRowsKeep* m = tri_rows_keep();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<TriRowsKeep> c(m, stream);
    const size_t need = (size_t)cap * sizeof(BowRec);                    // the pairs run one behind the other: they share the records of one
    if (m->rec.size() < need) {
        HIPCHK(m, m->chain.wait());
        HIPCHK(m, m->rec.ensure(orbx::doubled(m->rec.size(), need)));
    }
    TRY(c.begin());
    TRY(enqueue_chain(m, c.st, prm, pair, npairs, d_pairs, P, S, O, N, m->rec.as<BowRec>(), factors1, sigma2_1, factors2, sigma2_2, nlevels));
    return c.end();
}

int orbt_new_points_rows(const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* pairs, const float* F12, const float* factors1,
                         const float* sigma2_1, const float* factors2, const float* sigma2_2, int nlevels, const orbx_keypoint* kps,
                         const uint8_t* desc, const int32_t* nt, const uint32_t* fv_node, const int32_t* fv_off, const uint32_t* fv_feat,
                         const int32_t* nfv, int nrows, int cap, int rows_on_device, uint8_t* qvalid, uint8_t* claimed, int32_t* q2t, int32_t* t2q,
                         int32_t* nmatches, uint8_t* status, float* x3d, float* v, int32_t* match12, int32_t* acc_idx, float* acc_x3d, int32_t* count,
                         int32_t* overflow, int ocap, void* stream) {
    using namespace orbs;
    using orbx::Layout;
    const TriPairs P{pair, npairs, qvalid, 0, claimed, F12, 0, 0};
    const BowStore S{kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap};
    const BowOut O{q2t, t2q, nullptr, nullptr, nmatches};
    const NewPointsOut N{status, x3d, v, match12, acc_idx, acc_x3d, count, overflow, ocap};
    if (check_new_points(prm, pair, npairs, pairs, P, S, O, N, factors1, sigma2_1, factors2, sigma2_2, nlevels, false, rows_on_device != 0) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    TriRowsKeep* m = tri_rows_keep();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<TriRowsKeep> c(m, stream);
    const NewPointsBlock B(npairs, S, t2q != nullptr, v != nullptr, ocap, rows_on_device == 0);
    orbx::Staged<TriRowsKeep> s(c, m->block, B.L);
    TRY(s.fit());
    uint8_t *h = s.h, *d = s.d;
    const orbt_pair* d_pairs = Layout::put(h, d, B.pairs, pairs, (size_t)npairs);
    const float* d_F12 = Layout::put(h, d, B.F12, F12, 9 * (size_t)npairs);
    const uint8_t* d_qv_in = Layout::put(h, d, B.qvalid, (const uint8_t*)qvalid, (size_t)cap);
    const uint8_t* d_cl_in = Layout::put(h, d, B.claimed, (const uint8_t*)claimed, B.nent);
    const BowStore DS{Layout::put(h, d, B.kps, kps, B.nfeat), Layout::put(h, d, B.desc, desc, B.nfeat * 32), Layout::put(h, d, B.nt, nt, (size_t)nrows),
                      Layout::put(h, d, B.fv_node, fv_node, B.nfeat), Layout::put(h, d, B.fv_off, fv_off, (size_t)nrows * (cap + 1)),
                      Layout::put(h, d, B.fv_feat, fv_feat, B.nfeat), Layout::put(h, d, B.nfv, nfv, (size_t)nrows), nrows, cap};
    const TriPairs DP{pair, npairs, Layout::at(d, B.qvalid_out), 0, Layout::at(d, B.claimed_out), d_F12, 0, 0};
    const BowOut DO{Layout::at(d, B.q2t), Layout::at(d, B.t2q), nullptr, nullptr, Layout::at(d, B.nmatches)};
    const NewPointsOut DN{Layout::at(d, B.status), Layout::at(d, B.x3d), Layout::at(d, B.v), Layout::at(d, B.match12), Layout::at(d, B.acc_idx),
                          Layout::at(d, B.acc_x3d), Layout::at(d, B.count), Layout::at(d, B.overflow), ocap};
    TRY(s.run([&]() -> int {
        // the flags the chain updates in place live in the span that comes back; entries the kernels leave alone (behind a row's count) are defined
        HIPCHK(m, hipMemcpyAsync(Layout::at(d, B.qvalid_out), d_qv_in, (size_t)cap, hipMemcpyDeviceToDevice, c.st));
        HIPCHK(m, hipMemcpyAsync(Layout::at(d, B.claimed_out), d_cl_in, B.nent, hipMemcpyDeviceToDevice, c.st));
        HIPCHK(m, hipMemsetAsync(d + B.nmatches.off, 0, B.L.upload() + B.L.download() - B.nmatches.off, c.st));
        return enqueue_chain(m, c.st, prm, pair, npairs, d_pairs, DP, DS, DO, DN, Layout::at(d, B.rec), factors1, sigma2_1, factors2, sigma2_2, nlevels);
    }));
    std::memcpy(qvalid, Layout::at(h, B.qvalid_out), (size_t)cap);
    std::memcpy(claimed, Layout::at(h, B.claimed_out), B.nent);
    std::memcpy(nmatches, Layout::at(h, B.nmatches), (size_t)npairs * 4);
    std::memcpy(count, Layout::at(h, B.count), (size_t)npairs * 4);
    std::memcpy(overflow, Layout::at(h, B.overflow), (size_t)npairs * 4);
    std::memcpy(q2t, Layout::at(h, B.q2t), B.nent * 4);
    if (t2q) std::memcpy(t2q, Layout::at(h, B.t2q), B.nent * 4);
    std::memcpy(status, Layout::at(h, B.status), B.nent);
    std::memcpy(x3d, Layout::at(h, B.x3d), B.nent * 12);
    if (v) std::memcpy(v, Layout::at(h, B.v), B.nent * 16);
    std::memcpy(match12, Layout::at(h, B.match12), B.nent * 4);
    std::memcpy(acc_idx, Layout::at(h, B.acc_idx), B.nacc * 8);
    std::memcpy(acc_x3d, Layout::at(h, B.acc_x3d), B.nacc * 12);
    return ORBX_OK;
}

}  // extern "C"
