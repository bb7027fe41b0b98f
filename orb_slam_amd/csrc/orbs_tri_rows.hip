// ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:852-1014) over the rows of a resident key-frame store, and the chain
// search -> finish -> triangulate per neighbour of LocalMapping::CreateNewMapPoints over the same rows.  include/orbs.h and include/orbt.h are the
// boundary (ORBS_RULE_TRIANGULATION states the rule); orbs_rows.h holds the host side.
//
// As in SearchByBoW (orbs_bow_rows.hip) a feature lies under exactly one node of its FeatureVector, and vbMatched2[idx2] is only read by queries of
// the node that wrote it: every common node is an independent greedy problem, and only the rotation histogram and the count join them.  What a
// query takes is the smallest (dist, idx2) among the candidates that are unclaimed, have dist <= th and lie on the query's epipolar line, provided
// its distance is at most 2 * BestDist, BestDist being the smallest distance among the unclaimed candidates with dist <= th, on the line or not:
// the reference walks its sorted vDistIndex up to DistTh = 2 * BestDist and takes the first entry that passes CheckDistEpipolarLine.  That is one
// epipolar test per lane and two wave minima; there is no sequential walk of a sorted list.
//
// k_tri_rows: a flat grid over (pair, query node), one WAVE per node, four per workgroup: rows_node_walk of orbs_rows_device.h (what k_bow_rows
//   is too) with TriRule.  A run of up to 64 entries keeps its key point positions and epipolar bounds in registers next to its features and
//   descriptors.  A lane keeps its smallest distance and its smallest passing key (distance << 16 | idx2); each lane computes its query's line
//   l = x1' F12 once.  The record holds idx2, the rotation bin, BestDist and the distance taken.  The only LDS is the 16-entry table of
//   epipolar bounds.
// k_tri_rows_finish: one workgroup per pair behind it on the same stream: rows_finish of orbs_rows_device.h.
// The chain enqueues, per neighbour, k_tri_rows and k_tri_rows_finish for ONE pair given by value and the unchanged k_triangulate
// (orbt_triangulate_batch_device with row-offset pointers), which clears / sets the two flag arrays the next neighbour's search reads.
#include <hip/hip_runtime.h>

#include <climits>

#include "orbs.h"
#include "orbs_rows.h"
#include "orbs_rows_device.h"
#include "orbt.h"

namespace orbs {

// The rule of SearchForTriangulation: a train key point is held as its position and the epipolar bound of its octave, a query as its epipolar line;
// candidates are keyed by FEATURE (the order of the reference's sort, so the list need not ascend within a node), and nothing above `th` is kept.
struct TriRule {
    static constexpr bool by_feature = true;
    const float* F;                    // F12 of the pair
    const float* thr;                  // the bound per octave
    int th;
    struct Held { float x, y, thr; };
    struct Query {
        EpiLine E;
        __device__ __forceinline__ Query of_lane(int l) const { return {EpiLine{lane_f(E.a, l), lane_f(E.b, l), lane_f(E.c, l), lane_f(E.den, l), E.th}}; }
    };
    __device__ __forceinline__ Held hold(const orbx_keypoint& kp) const { return {kp.x, kp.y, thr[epi_level(kp.octave)]}; }
    __device__ __forceinline__ Query query(const orbx_keypoint& kp) const { return {epi_line(kp.x, kp.y, F, th)}; }      // l = x1' F12, once per query
    struct Acc {
        uint32_t md = KEY_NONE, mk = KEY_NONE;                           // the lane's smallest distance, its smallest key ON the line
        int mpos = 0;                                                    // the list position of mk
        template <class GetHeld>
        __device__ __forceinline__ void offer(uint32_t dist, uint32_t f, int pos, GetHeld held, const Query& q, const TriRule& r) {
            if ((int)dist > r.th) return;                                // `if(dist>TH_LOW) continue;`
            md = min(md, dist);
            const uint32_t key = (dist << 16) | f;
            if (key >= mk) return;                                       // the line is tested only for a key that would lower the minimum
            const Held h = held();
            if (epi_ok(q.E, h.x, h.y, h.thr)) { mk = key; mpos = pos; }
        }
    };
    __device__ __forceinline__ RowsPick resolve(Acc& a, int) const {
        const uint32_t kb = wave_min_u32(a.md);                          // BestDist = vDistIndex.front().first
        const uint32_t kw = wave_min_u32(a.mk);                          // the first entry of the sorted list that is on the line
        const int bd = kb == KEY_NONE ? INT_MAX : (int)kb;
        if (kw == KEY_NONE || (int)(kw >> 16) > 2 * bd) return {bd, INT_MAX, -1, -1};      // `if(vDistIndex[id].first>DistTh) break;` (src/ORBmatcher.cc:927-957)
        const int owner = __ffsll((long long)__ballot(a.mk == kw)) - 1;
        return {bd, (int)(kw >> 16), __builtin_amdgcn_readlane(a.mpos, owner), (int)(kw & 0xFFFFu)};      // the walk sets vbMatched2[idx2]
    }
};

__global__ __launch_bounds__(ROWS_WAVES * 64) void k_tri_rows(TriRows a, int blocks_per_pair) {
    __shared__ float thr[ORBS_MAX_LEVELS];
#pragma unroll
    for (int i = 0; i < ORBS_MAX_LEVELS; ++i) if (threadIdx.x == i) thr[i] = a.epi_thr[i];
    __syncthreads();
    const int p = (int)(blockIdx.x / (unsigned)blocks_per_pair);
    const int j = uni((int)(blockIdx.x % (unsigned)blocks_per_pair) * ROWS_WAVES + (int)(threadIdx.x >> 6));         // the query node of this wave
    const int cap = a.S.cap;
    const int qr = a.P.pair ? a.P.pair[2 * p] : a.P.qr0, tr = a.P.pair ? a.P.pair[2 * p + 1] : a.P.tr0;
    if ((unsigned)qr >= (unsigned)a.S.nrows || (unsigned)tr >= (unsigned)a.S.nrows) return;      // the pair finds nothing: k_tri_rows_finish says so
    if (j >= clampi(a.S.nfv[qr], 0, cap)) return;
    float F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = a.P.F12[(size_t)p * 9 + i];
    rows_node_walk(a.S, p, qr, tr, j, a.P.claimed ? a.P.claimed + (size_t)p * cap : nullptr, a.P.qvalid ? a.P.qvalid + (size_t)p * a.P.qstride : nullptr,
                   a.check_orientation != 0, a.rec, TriRule{F, thr, a.th});
}

__global__ __launch_bounds__(ROWS_FINISH_TPB) void k_tri_rows_finish(TriRows a) {
    const int p = blockIdx.x;
    rows_finish<ROWS_FINISH_TPB>(a.check_orientation != 0, a.S, a.P.pair ? a.P.pair[2 * p] : a.P.qr0, a.P.pair ? a.P.pair[2 * p + 1] : a.P.tr0, a.O,
                                 a.rec, p);
}

static hipError_t launch_tri_rows(const TriRows& a, hipStream_t st) {
    const int bpp = rows_blocks_per_pair(a.S.cap);
    k_tri_rows<<<dim3((unsigned)a.P.npairs * (unsigned)bpp), ROWS_WAVES * 64, 0, st>>>(a, bpp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_tri_rows_finish<<<dim3((unsigned)a.P.npairs), ROWS_FINISH_TPB, 0, st>>>(a);
    return hipGetLastError();
}

// the rows with what the rule adds to them
static TriRows with_params(const BowRows& r, const orbs_params* prm, const float* level_sigma2, int nlevels) {
    TriRows a{r, {}, prm->th, prm->check_orientation ? 1 : 0};
    for (int i = 0; i < ORBS_MAX_LEVELS; ++i) a.epi_thr[i] = orbs_epipolar_bound(level_sigma2[i < nlevels ? i : nlevels - 1]);
    return a;
}

struct TriKeep;                        // this translation unit's RowsKeep: its records, block and chain are not those of orbs_bow_rows.hip

// search p, finish p, triangulate p for p = 0 .. npairs-1 on st: nothing but launches.  `pair` is the HOST list; P, O and N name the device arrays
// of all pairs (P.qvalid shared, written by the triangulation; P.claimed per pair, written too).
static int enqueue_chain(RowsKeep<TriKeep>* m, hipStream_t st, const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* d_pairs,
                         const RowPairs& P, const BowStore& S, const BowOut& O, const NewPointsOut& N, BowRec* rec, const float* factors1,
                         const float* sigma2_1, const float* factors2, const float* sigma2_2, int nlevels) {
    const size_t cap = (size_t)S.cap;
    TriRows a = with_params(BowRows{S, P, O, rec}, prm, sigma2_2, nlevels);
    for (int p = 0; p < npairs; p++) {
        const int qr = pair[2 * p], tr = pair[2 * p + 1];
        const size_t e = (size_t)p * cap, o = (size_t)p * N.ocap;
        uint8_t* claimed = const_cast<uint8_t*>(P.claimed) + e;
        a.P = RowPairs{nullptr, 1, P.qvalid, 0, claimed, P.F12 + (size_t)p * 9, qr, tr};
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

extern "C" {

int orbs_tri_rows_search_batch_device(const orbs_params* prm, const int32_t* d_pair, int npairs, const float* d_F12, const float* level_sigma2,
                                      int nlevels, const orbx_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nt, const uint32_t* d_fv_node,
                                      const int32_t* d_fv_off, const uint32_t* d_fv_feat, const int32_t* d_nfv, int nrows, int cap,
                                      const uint8_t* d_qvalid, int qstride, const uint8_t* d_claimed, int32_t* d_q2t, int32_t* d_t2q, int32_t* d_best,
                                      int32_t* d_second, int32_t* d_nmatches, void* stream) {
    using namespace orbs;
    const RowPairs P{d_pair, npairs, d_qvalid, qstride, d_claimed, d_F12, 0, 0};
    const BowStore S{d_kps, d_desc, d_nt, d_fv_node, d_fv_off, d_fv_feat, d_nfv, nrows, cap};
    const BowOut O{d_q2t, d_t2q, d_best, d_second, d_nmatches};
    if (check_tri_rows(prm, P, S, O, level_sigma2, nlevels, true, true) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    return rows_device_form<TriKeep>(P, S, O, stream, [&](const BowRows& a, hipStream_t st) { return launch_tri_rows(with_params(a, prm, level_sigma2, nlevels), st); });
}

int orbs_tri_rows_search(const orbs_params* prm, const int32_t* pair, int npairs, const float* F12, const float* level_sigma2, int nlevels,
                         const orbx_keypoint* kps, const uint8_t* desc, const int32_t* nt, const uint32_t* fv_node, const int32_t* fv_off,
                         const uint32_t* fv_feat, const int32_t* nfv, int nrows, int cap, int rows_on_device, const uint8_t* qvalid, int qstride,
                         const uint8_t* claimed, int32_t* q2t, int32_t* t2q, int32_t* best, int32_t* second, int32_t* nmatches, void* stream) {
    using namespace orbs;
    const RowPairs P{pair, npairs, qvalid, qstride, claimed, F12, 0, 0};
    const BowStore S{kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap};
    const BowOut O{q2t, t2q, best, second, nmatches};
    if (check_tri_rows(prm, P, S, O, level_sigma2, nlevels, false, rows_on_device != 0) != ORBX_OK) return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    return rows_host_form<TriKeep>(P, S, O, rows_on_device == 0, stream,
                                   [&](const BowRows& a, hipStream_t st) { return launch_tri_rows(with_params(a, prm, level_sigma2, nlevels), st); });
}

int orbt_new_points_rows_device(const orbs_params* prm, const int32_t* pair, int npairs, const orbt_pair* d_pairs, const float* d_F12,
                                const float* factors1, const float* sigma2_1, const float* factors2, const float* sigma2_2, int nlevels,
                                const orbx_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_nt, const uint32_t* d_fv_node,
                                const int32_t* d_fv_off, const uint32_t* d_fv_feat, const int32_t* d_nfv, int nrows, int cap, uint8_t* d_qvalid,
                                uint8_t* d_claimed, int32_t* d_q2t, int32_t* d_t2q, int32_t* d_nmatches, uint8_t* d_status, float* d_x3d, float* d_v,
                                int32_t* d_match12, int32_t* d_acc_idx, float* d_acc_x3d, int32_t* d_count, int32_t* d_overflow, int ocap,
                                void* stream) {
    using namespace orbs;
    const RowPairs P{pair, npairs, d_qvalid, 0, d_claimed, d_F12, 0, 0};
    const BowStore S{d_kps, d_desc, d_nt, d_fv_node, d_fv_off, d_fv_feat, d_nfv, nrows, cap};
    const BowOut O{d_q2t, d_t2q, nullptr, nullptr, d_nmatches};
    const NewPointsOut N{d_status, d_x3d, d_v, d_match12, d_acc_idx, d_acc_x3d, d_count, d_overflow, ocap};
    if (check_new_points(prm, pair, npairs, d_pairs, P, S, O, N, factors1, sigma2_1, factors2, sigma2_2, nlevels, true, true) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    RowsKeep<TriKeep>* m = RowsKeep<TriKeep>::get();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<RowsKeep<TriKeep>> c(m, stream);
    TRY(m->ensure_rec((size_t)cap * sizeof(BowRec)));                    // the pairs run one behind the other: they share the records of one
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
    const RowPairs P{pair, npairs, qvalid, 0, claimed, F12, 0, 0};
    const BowStore S{kps, desc, nt, fv_node, fv_off, fv_feat, nfv, nrows, cap};
    const BowOut O{q2t, t2q, nullptr, nullptr, nmatches};
    const NewPointsOut N{status, x3d, v, match12, acc_idx, acc_x3d, count, overflow, ocap};
    if (check_new_points(prm, pair, npairs, pairs, P, S, O, N, factors1, sigma2_1, factors2, sigma2_2, nlevels, false, rows_on_device != 0) != ORBX_OK)
        return ORBX_ERR_ARG;
    if (npairs == 0) return ORBX_OK;
    RowsKeep<TriKeep>* m = RowsKeep<TriKeep>::get();
    if (!m) return ORBX_ERR_DEVICE;
    orbx::Call<RowsKeep<TriKeep>> c(m, stream);
    const NewPointsBlock B(npairs, S, t2q != nullptr, v != nullptr, ocap, rows_on_device == 0);
    orbx::Staged<RowsKeep<TriKeep>> s(c, m->block, B.L);
    TRY(s.fit());
    uint8_t *h = s.h, *d = s.d;
    const orbt_pair* d_pairs = Layout::put(h, d, B.pairs, pairs, (size_t)npairs);
    const float* d_F12 = Layout::put(h, d, B.F12, F12, 9 * (size_t)npairs);
    const uint8_t* d_qv_in = Layout::put(h, d, B.qvalid, (const uint8_t*)qvalid, (size_t)cap);
    const uint8_t* d_cl_in = Layout::put(h, d, B.claimed, (const uint8_t*)claimed, B.nent);
    const BowStore DS = B.put(h, d, S);
    const RowPairs DP{pair, npairs, Layout::at(d, B.qvalid_out), 0, Layout::at(d, B.claimed_out), d_F12, 0, 0};
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
