// The host side of orbs_tri_rows_search* and orbt_new_points_rows* on the CPU against tests/_probe/hip_stub: the argument checks
// (orbs::check_tri_rows, check_chain_pairs, check_new_points: every ORBX_ERR_ARG condition include/orbs.h and include/orbt.h list), the layout,
// staging and unpacking of the two host forms' blocks (orbs::RowsBlock of orbs_rows.h with its F12 slot, NewPointsBlock), whose copies run over
// heap blocks of exactly the computed sizes, and what LocalMapPointsNewPoints.cc packs per call (orb_slam_amd/cpp/NewPointsPacking.h).
// tests/test_tri_rows_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a program.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "NewPointsPacking.h"
#include "orbs_rows.h"

using namespace orbs;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {
struct Mat3 {                                  // the little of cv::Mat that PackF12 reads
    int rows, cols;
    float v[12];
    bool empty() const { return rows == 0 || cols == 0; }
    template <class T> const T& at(int r, int c) const { return v[r * cols + c]; }
};
}  // namespace

int main() {
    const int npairs = 3, nrows = 4, cap = 7, ocap = 5;
    const orbs_params prm{ORBS_RULE_TRIANGULATION, ORBS_TH_LOW, 0.0f, 0};
    std::vector<int32_t> pair = {0, 1, 0, 3, 0, 2}, nt = {7, 2, 0, 5}, nfv = {3, 1, 0, 2};
    std::vector<uint8_t> desc_store((size_t)nrows * cap * 32 + 16, 0xAB);
    uint8_t* desc = desc_store.data() + ((16 - ((uintptr_t)desc_store.data() & 15)) & 15);         // 16-byte aligned
    std::vector<orbx_keypoint> kps((size_t)nrows * cap);
    for (size_t i = 0; i < kps.size(); i++) kps[i].octave = (int)i;
    std::vector<uint32_t> fv_node((size_t)nrows * cap, 5), fv_feat((size_t)nrows * cap, 6);
    std::vector<int32_t> fv_off((size_t)nrows * (cap + 1), 3);
    fv_off.back() = 9;
    std::vector<uint8_t> qvalid((size_t)npairs * cap, 1), claimed((size_t)npairs * cap, 2);
    std::vector<float> F12(9 * npairs, 0.5f), sigma2 = {1.0f, 1.44f, 2.0736f};
    F12.back() = 7.0f;
    std::vector<int32_t> q2t((size_t)npairs * cap, -7), t2q(q2t), best(q2t), second(q2t), nm(npairs, -7);
    const RowPairs P{pair.data(), npairs, qvalid.data(), cap, claimed.data(), F12.data(), 0, 0};
    const BowStore S{kps.data(), desc, nt.data(), fv_node.data(), fv_off.data(), fv_feat.data(), nfv.data(), nrows, cap};
    const BowOut O{q2t.data(), t2q.data(), best.data(), second.data(), nm.data()};
    {
        // orbs_tri_rows_search*: the checks, host form and device form
        for (int dev = 0; dev < 2; dev++) {
            const bool d = dev != 0;
            auto chk = [&](const orbs_params* q, const RowPairs& p, const BowStore& s, const BowOut& o, const float* s2 = nullptr, int nl = 3) {
                return check_tri_rows(q, p, s, o, s2 ? s2 : sigma2.data(), nl, d, d);
            };
            CHECK(chk(&prm, P, S, O) == ORBX_OK);
            CHECK(chk(nullptr, P, S, O) == ORBX_ERR_ARG);
            orbs_params q = prm;
            q.rule = ORBS_RULE_BOW;
            CHECK(chk(&q, P, S, O) == ORBX_ERR_ARG);
            q = prm; q.th = -1;
            CHECK(chk(&q, P, S, O) == ORBX_ERR_ARG);
            q.th = 257;
            CHECK(chk(&q, P, S, O) == ORBX_ERR_ARG);
            q.th = 256; q.ratio = std::nanf("");                                    // the ratio is not read
            CHECK(chk(&q, P, S, O) == ORBX_OK);
            CHECK(check_tri_rows(&prm, P, S, O, nullptr, 3, d, d) == ORBX_ERR_ARG);
            CHECK(chk(&prm, P, S, O, nullptr, 0) == ORBX_ERR_ARG && chk(&prm, P, S, O, nullptr, ORBS_MAX_LEVELS + 1) == ORBX_ERR_ARG);
            RowPairs p2 = P;
            p2.npairs = -1;
            CHECK(chk(&prm, p2, S, O) == ORBX_ERR_ARG);
            p2 = RowPairs{nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 0};           // no pairs: nothing is looked at
            CHECK(chk(&prm, p2, BowStore{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1}, BowOut{}) == ORBX_OK);
            p2 = P; p2.pair = nullptr;
            CHECK(chk(&prm, p2, S, O) == ORBX_ERR_ARG);
            p2 = P; p2.F12 = nullptr;
            CHECK(chk(&prm, p2, S, O) == ORBX_ERR_ARG);
            p2 = P; p2.qvalid = nullptr; p2.claimed = nullptr;
            CHECK(chk(&prm, p2, S, O) == ORBX_OK);
            p2 = P; p2.qstride = 0;                                                 // one array for all pairs
            CHECK(chk(&prm, p2, S, O) == ORBX_OK);
            p2.qstride = cap - 1;
            CHECK(chk(&prm, p2, S, O) == ORBX_ERR_ARG);
            p2.qstride = -1;
            CHECK(chk(&prm, p2, S, O) == ORBX_ERR_ARG);
            p2 = P; p2.npairs = 306783379;                                          // ceil(2^31 / 7): npairs * cap reaches 2^31
            CHECK(chk(&prm, p2, S, O) == ORBX_ERR_ARG);
            p2 = P; p2.npairs = 2; p2.qstride = 1 << 30;                            // npairs * qstride + cap reaches 2^31
            CHECK(chk(&prm, p2, S, O) == ORBX_ERR_ARG);
            BowStore s2 = S;
            s2.cap = 0;
            CHECK(chk(&prm, P, s2, O) == ORBX_ERR_ARG);
            s2.cap = ORBF_MAX_FEATURES + 1;
            CHECK(chk(&prm, P, s2, O) == ORBX_ERR_ARG);
            s2 = S; s2.nrows = 0;
            CHECK(chk(&prm, P, s2, O) == ORBX_ERR_ARG);
            s2 = S; s2.nrows = 268435456;                                           // nrows * (cap + 1) reaches 2^31
            CHECK(chk(&prm, P, s2, O) == ORBX_ERR_ARG);
            const void** members[] = {(const void**)&s2.kps, (const void**)&s2.desc, (const void**)&s2.nt, (const void**)&s2.fv_node, (const void**)&s2.fv_off,
                                      (const void**)&s2.fv_feat, (const void**)&s2.nfv};
            for (const void** mbr : members) {
                s2 = S;
                *mbr = nullptr;
                CHECK(chk(&prm, P, s2, O) == ORBX_ERR_ARG);
            }
            BowOut o2 = O;
            o2.nmatches = nullptr;
            CHECK(chk(&prm, P, S, o2) == ORBX_ERR_ARG);
            o2 = BowOut{nullptr, nullptr, nullptr, nullptr, nm.data()};             // the four arrays are optional
            CHECK(chk(&prm, P, S, o2) == ORBX_OK);
        }
        // alignment: device descriptors are read in 16-byte pieces, device words are words; host arrays are copied into aligned slots
        BowStore s2 = S;
        s2.desc = desc + 4;
        CHECK(check_tri_rows(&prm, P, s2, O, sigma2.data(), 3, false, false) == ORBX_OK);
        CHECK(check_tri_rows(&prm, P, s2, O, sigma2.data(), 3, false, true) == ORBX_ERR_ARG);
        RowPairs p2 = P;
        p2.F12 = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(F12.data()) + 2);
        CHECK(check_tri_rows(&prm, p2, S, O, sigma2.data(), 3, true, true) == ORBX_ERR_ARG);
        CHECK(check_tri_rows(&prm, p2, S, O, sigma2.data(), 3, false, false) == ORBX_OK);
        BowOut o2 = O;
        o2.t2q = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(t2q.data()) + 2);
        CHECK(check_tri_rows(&prm, P, S, o2, sigma2.data(), 3, true, true) == ORBX_ERR_ARG);
        // the host form walks the pairs; the device form reports a row out of range per pair
        std::vector<int32_t> bad = pair;
        bad[3] = nrows;
        p2 = P; p2.pair = bad.data();
        CHECK(check_tri_rows(&prm, p2, S, O, sigma2.data(), 3, false, false) == ORBX_ERR_ARG);
        CHECK(check_tri_rows(&prm, p2, S, O, sigma2.data(), 3, true, true) == ORBX_OK);
    }
    {
        // the block of orbs_tri_rows_search with everything in it: slots at multiples of 256, one span up, one down, the records behind
        const RowsBlock B(P, S, O, true);
        CHECK(B.pair.off == 0 && B.F12.off == 256 && B.qvalid.off == 512 && B.claimed.off == 768 && B.nt.off == 1024 && B.nfv.off == 1280 && B.kps.off == 1536);
        CHECK(B.desc.off == 1536 + 1024 && B.fv_node.off == 2560 + 1024 && B.fv_off.off == 3584 + 256 && B.fv_feat.off == 3840 + 256);
        const size_t up = B.L.upload();
        CHECK(up == 4096 + 256 && B.nmatches.off == up && B.q2t.off == up + 256 && B.second.off == up + 1024 && B.L.download() == 1280);
        CHECK(B.rec.off == up + 1280 && B.L.total() == up + 1280 + 512 && B.nqv == (size_t)(npairs - 1) * cap + cap);
        std::vector<uint8_t> h(B.L.upload() + B.L.download()), d(B.L.total());
        const BowRows a = B.stage(h.data(), d.data(), P, S);
        CHECK((const uint8_t*)a.P.pair == d.data() && (const uint8_t*)a.P.F12 == d.data() + 256 && a.P.qvalid == d.data() + 512 && a.P.claimed == d.data() + 768);
        CHECK(a.P.npairs == npairs && a.P.qstride == cap && (const uint8_t*)a.S.nt == d.data() + 1024 && (const uint8_t*)a.S.kps == d.data() + 1536);
        CHECK(a.S.desc == d.data() + 2560 && (const uint8_t*)a.S.fv_feat == d.data() + 4096 && a.S.nrows == nrows && a.S.cap == cap);
        CHECK((uint8_t*)a.O.nmatches == d.data() + up && (uint8_t*)a.O.second == d.data() + up + 1024 && (uint8_t*)a.rec == d.data() + up + 1280);
        CHECK(reinterpret_cast<const int32_t*>(h.data())[5] == 2 && reinterpret_cast<const float*>(h.data() + 256)[9 * npairs - 1] == 7.0f);
        CHECK(h[512 + npairs * cap - 1] == 1 && h[768 + npairs * cap - 1] == 2 && reinterpret_cast<const int32_t*>(h.data() + 1024)[3] == 5);
        CHECK(reinterpret_cast<const orbx_keypoint*>(h.data() + 1536)[nrows * cap - 1].octave == nrows * cap - 1 && h[2560 + nrows * cap * 32 - 1] == 0xAB);
        for (int i = 0; i < npairs * cap; i++) { orbx::Layout::at(h.data(), B.q2t)[i] = 100 + i; orbx::Layout::at(h.data(), B.best)[i] = 200 + i; }
        for (int p = 0; p < npairs; p++) orbx::Layout::at(h.data(), B.nmatches)[p] = 10 + p;
        B.unpack(h.data(), BowOut{q2t.data(), nullptr, best.data(), nullptr, nm.data()});
        CHECK(q2t[0] == 100 && q2t[npairs * cap - 1] == 100 + npairs * cap - 1 && best[3] == 203 && t2q[0] == -7 && second[0] == -7 && nm[2] == 12);
        // one qvalid array for all pairs takes cap bytes; resident rows and absent arrays take no room
        RowPairs p2 = P;
        p2.qstride = 0; p2.claimed = nullptr;
        const RowsBlock C(p2, S, BowOut{nullptr, t2q.data(), nullptr, nullptr, nm.data()}, false);
        CHECK(C.nqv == (size_t)cap && !C.claimed.present && !C.kps.present && !C.desc.present && !C.fv_feat.present && C.nt.present && C.nfv.present);
        CHECK(!C.q2t.present && C.t2q.present && C.L.upload() == 1280 && C.L.download() == 512 && C.L.total() == 1280 + 512 + 512);
        std::vector<uint8_t> h2(C.L.upload() + C.L.download()), d2(C.L.total());
        const BowRows c = C.stage(h2.data(), d2.data(), p2, S);
        CHECK(!c.P.claimed && c.S.kps == kps.data() && c.S.desc == desc && c.S.fv_off == fv_off.data() && !c.O.q2t && (uint8_t*)c.O.t2q == d2.data() + 1280 + 256);
    }
    {
        // orbt_new_points_rows*: the pair list
        const int32_t ok[] = {0, 1, 0, 3, 0, 2};
        CHECK(check_chain_pairs(ok, 3, nrows) == ORBX_OK && check_chain_pairs(nullptr, 0, nrows) == ORBX_OK);
        CHECK(check_chain_pairs(nullptr, 1, nrows) == ORBX_ERR_ARG && check_chain_pairs(ok, -1, nrows) == ORBX_ERR_ARG);
        CHECK(check_chain_pairs(ok, ORBT_MAX_PAIRS + 1, nrows) == ORBX_ERR_ARG);
        const int32_t twice[] = {0, 1, 0, 3, 0, 1}, self[] = {0, 1, 0, 0}, other_query[] = {0, 1, 2, 3}, past[] = {0, 1, 0, 4}, neg[] = {0, -1};
        CHECK(check_chain_pairs(twice, 3, nrows) == ORBX_ERR_ARG && check_chain_pairs(self, 2, nrows) == ORBX_ERR_ARG);
        CHECK(check_chain_pairs(other_query, 2, nrows) == ORBX_ERR_ARG && check_chain_pairs(past, 2, nrows) == ORBX_ERR_ARG);
        CHECK(check_chain_pairs(neg, 1, nrows) == ORBX_ERR_ARG);
        // ... and the arguments of both forms
        std::vector<orbt_pair> poses(npairs);
        std::vector<float> fac = {1.0f, 1.2f, 1.44f};
        std::vector<uint8_t> status((size_t)npairs * cap);
        std::vector<float> x3d((size_t)npairs * cap * 3), v_store((size_t)npairs * cap * 4 + 4), ax((size_t)npairs * ocap * 3);
        float* v = v_store.data() + ((16 - ((uintptr_t)v_store.data() & 15)) & 15) / 4;
        std::vector<int32_t> m12((size_t)npairs * cap), ai((size_t)npairs * ocap * 2), count(npairs), overflow(npairs);
        RowPairs Q = P;
        Q.qstride = 0;
        const BowOut QO{q2t.data(), t2q.data(), nullptr, nullptr, nm.data()};
        const NewPointsOut N{status.data(), x3d.data(), v, m12.data(), ai.data(), ax.data(), count.data(), overflow.data(), ocap};
        for (int dev = 0; dev < 2; dev++) {
            const bool d = dev != 0;
            auto chk = [&](const RowPairs& p, const BowOut& o, const NewPointsOut& n, const orbs_params* q = nullptr) {
                return check_new_points(q ? q : &prm, p.pair, npairs, poses.data(), p, S, o, n, fac.data(), sigma2.data(), fac.data(), sigma2.data(), 3, d, d);
            };
            CHECK(chk(Q, QO, N) == ORBX_OK);
            orbs_params q = prm;
            q.rule = ORBS_RULE_BOW;
            CHECK(chk(Q, QO, N, &q) == ORBX_ERR_ARG);
            CHECK(check_new_points(&prm, Q.pair, npairs, poses.data(), Q, S, QO, N, nullptr, sigma2.data(), fac.data(), sigma2.data(), 3, d, d) == ORBX_ERR_ARG);
            CHECK(check_new_points(&prm, Q.pair, npairs, poses.data(), Q, S, QO, N, fac.data(), nullptr, fac.data(), sigma2.data(), 3, d, d) == ORBX_ERR_ARG);
            CHECK(check_new_points(&prm, Q.pair, npairs, poses.data(), Q, S, QO, N, fac.data(), sigma2.data(), nullptr, sigma2.data(), 3, d, d) == ORBX_ERR_ARG);
            CHECK(check_new_points(&prm, Q.pair, npairs, poses.data(), Q, S, QO, N, fac.data(), sigma2.data(), fac.data(), nullptr, 3, d, d) == ORBX_ERR_ARG);
            CHECK(check_new_points(&prm, Q.pair, npairs, poses.data(), Q, S, QO, N, fac.data(), sigma2.data(), fac.data(), sigma2.data(), 17, d, d) == ORBX_ERR_ARG);
            CHECK(check_new_points(&prm, Q.pair, npairs, nullptr, Q, S, QO, N, fac.data(), sigma2.data(), fac.data(), sigma2.data(), 3, d, d) == ORBX_ERR_ARG);
            RowPairs p2 = Q;
            p2.qstride = cap;                                                       // the pairs share one flag array
            CHECK(chk(p2, QO, N) == ORBX_ERR_ARG);
            p2 = Q; p2.qvalid = nullptr;
            CHECK(chk(p2, QO, N) == ORBX_ERR_ARG);
            p2 = Q; p2.claimed = nullptr;
            CHECK(chk(p2, QO, N) == ORBX_ERR_ARG);
            p2 = Q; p2.pair = twice;
            CHECK(chk(p2, QO, N) == ORBX_ERR_ARG);
            BowOut o2 = QO;
            o2.q2t = nullptr;
            CHECK(chk(Q, o2, N) == ORBX_ERR_ARG);
            o2 = QO; o2.t2q = nullptr;
            CHECK(chk(Q, o2, N) == ORBX_OK);
            NewPointsOut n2 = N;
            n2.ocap = 0;
            CHECK(chk(Q, QO, n2) == ORBX_ERR_ARG);
            n2 = N; n2.v = nullptr;
            CHECK(chk(Q, QO, n2) == ORBX_OK);
            void** outs[] = {(void**)&n2.status, (void**)&n2.x3d, (void**)&n2.match12, (void**)&n2.acc_idx, (void**)&n2.acc_x3d, (void**)&n2.count, (void**)&n2.overflow};
            for (void** mbr : outs) {
                n2 = N;
                *mbr = nullptr;
                CHECK(chk(Q, QO, n2) == ORBX_ERR_ARG);
            }
            n2 = N; n2.v = v + 1;                                                   // written as float4 on the device
            CHECK(chk(Q, QO, n2) == (d ? ORBX_ERR_ARG : ORBX_OK));
        }
        // the block of orbt_new_points_rows: the flags go up in the first span and come back in the second
        const NewPointsBlock B(npairs, S, true, true, ocap, true);
        CHECK(B.pairs.off == 0 && sizeof(orbt_pair) == 160 && B.F12.off == 512 && B.qvalid.off == 768 && B.claimed.off == 1024 && B.nt.off == 1280 && B.kps.off == 1792);
        const size_t up = B.L.upload();
        CHECK(up == 4352 + 256 && B.qvalid_out.off == up && B.claimed_out.off == up + 256 && B.nmatches.off == up + 512 && B.overflow.off == up + 1024);
        CHECK(B.q2t.off == up + 1280 && B.t2q.off == up + 1536 && B.status.off == up + 1792 && B.x3d.off == up + 2048 && B.v.off == up + 2304 && (B.v.off & 15) == 0);
        CHECK(B.match12.off == up + 2304 + 512 && B.acc_idx.off == up + 3072 && B.acc_x3d.off == up + 3328 && B.L.download() == 3584 && B.rec.off == up + 3584);
        CHECK(B.L.total() == up + 3584 + 256 && B.nent == (size_t)npairs * cap && B.nacc == (size_t)npairs * ocap);
        const NewPointsBlock C(npairs, S, false, false, ocap, false);
        CHECK(!C.t2q.present && !C.v.present && !C.kps.present && !C.fv_off.present && C.nt.present && C.qvalid_out.off == C.L.upload() && C.L.upload() == 1792);
    }
    {
        // what the drop-in packs: flags on the POINTER (a bad point holds its slot), slots behind the vector are 0; F12 row major
        int a = 0, b = 0;
        std::vector<int*> pts = {&a, nullptr, &b, nullptr, nullptr};
        std::vector<uint8_t> f(cap, 9);
        ORB_SLAM::PackPointFlags(pts, false, cap, f.data());                        // "holds no map point yet"
        CHECK(f[0] == 0 && f[1] == 1 && f[2] == 0 && f[3] == 1 && f[4] == 1 && f[5] == 0 && f[6] == 0);
        ORB_SLAM::PackPointFlags(pts, true, cap, f.data());                         // "holds a map point"
        CHECK(f[0] == 1 && f[1] == 0 && f[2] == 1 && f[3] == 0 && f[4] == 0 && f[5] == 0 && f[6] == 0);
        ORB_SLAM::PackPointFlags(pts, true, 2, f.data());                           // a store narrower than the key frame: nothing behind cap is written
        CHECK(f[0] == 1 && f[1] == 0 && f[2] == 1);
        Mat3 F{3, 3, {1, 2, 3, 4, 5, 6, 7, 8, 9}};
        float out[9] = {0};
        CHECK(ORB_SLAM::PackF12(F, out) && out[0] == 1 && out[3] == 4 && out[5] == 6 && out[8] == 9);
        Mat3 none{0, 0, {0}}, wide{3, 4, {0}};
        out[0] = -1;
        CHECK(!ORB_SLAM::PackF12(none, out) && !ORB_SLAM::PackF12(wide, out) && out[0] == -1);
    }
    std::printf("tri rows host ok\n");
    return 0;
}
