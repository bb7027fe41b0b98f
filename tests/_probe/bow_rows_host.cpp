// The host side of orbs_bow_rows_search* on the CPU against tests/_probe/hip_stub: the argument checks (orbs::check_bow_rows), the layout, staging
// and unpacking of the host form's block (orbs::RowsBlock of orbs_rows.h, here without an F12 slot), whose copies run over heap blocks of exactly
// the computed sizes, and the CSR packing of a FeatureVector (orb_slam_amd/cpp/FeatureVectorCSR.h, what LocalMapPointsBoW.cc uploads per row).
// tests/test_bow_rows_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer and runs it as a program.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "FeatureVectorCSR.h"
#include "orbs_rows.h"

using namespace orbs;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const int npairs = 3, nrows = 4, cap = 7;
    const orbs_params prm{ORBS_RULE_BOW, ORBS_TH_LOW, 0.75f, 1};
    std::vector<int32_t> pair = {0, 1, 0, 3, 2, 1}, nt = {7, 2, 0, 5}, nfv = {3, 1, 0, 2};
    std::vector<uint8_t> desc_store((size_t)nrows * cap * 32 + 16, 0xAB);
    uint8_t* desc = desc_store.data() + ((16 - ((uintptr_t)desc_store.data() & 15)) & 15);         // 16-byte aligned
    std::vector<orbx_keypoint> kps((size_t)nrows * cap);
    for (size_t i = 0; i < kps.size(); i++) kps[i].octave = (int)i;
    std::vector<uint32_t> fv_node((size_t)nrows * cap, 5), fv_feat((size_t)nrows * cap, 6);
    std::vector<int32_t> fv_off((size_t)nrows * (cap + 1), 3);
    fv_off.back() = 9;
    std::vector<uint8_t> qvalid((size_t)npairs * cap, 1), claimed((size_t)npairs * cap, 2);
    std::vector<int32_t> q2t((size_t)npairs * cap, -7), t2q(q2t), best(q2t), second(q2t), nm(npairs, -7);
    const RowPairs P{pair.data(), npairs, qvalid.data(), cap, claimed.data(), nullptr, 0, 0};
    const BowStore S{kps.data(), desc, nt.data(), fv_node.data(), fv_off.data(), fv_feat.data(), nfv.data(), nrows, cap};
    const BowOut O{q2t.data(), t2q.data(), best.data(), second.data(), nm.data()};
    {
        // the checks, host form and device form
        for (int dev = 0; dev < 2; dev++) {
            const bool d = dev != 0;
            CHECK(check_bow_rows(&prm, P, S, O, d, d) == ORBX_OK);
            CHECK(check_bow_rows(nullptr, P, S, O, d, d) == ORBX_ERR_ARG);
            orbs_params q = prm;
            q.rule = ORBS_RULE_BEST;
            CHECK(check_bow_rows(&q, P, S, O, d, d) == ORBX_ERR_ARG);
            q = prm; q.th = -1;
            CHECK(check_bow_rows(&q, P, S, O, d, d) == ORBX_ERR_ARG);
            q.th = 257;
            CHECK(check_bow_rows(&q, P, S, O, d, d) == ORBX_ERR_ARG);
            q.th = 256;
            CHECK(check_bow_rows(&q, P, S, O, d, d) == ORBX_OK);
            q = prm; q.ratio = std::nanf("");
            CHECK(check_bow_rows(&q, P, S, O, d, d) == ORBX_ERR_ARG);
            RowPairs p2 = P;
            p2.npairs = -1;
            CHECK(check_bow_rows(&prm, p2, S, O, d, d) == ORBX_ERR_ARG);
            p2 = RowPairs{nullptr, 0, nullptr, 1, nullptr, nullptr, 0, 0};                          // no pairs: nothing is looked at
            CHECK(check_bow_rows(&prm, p2, BowStore{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1}, BowOut{}, d, d) == ORBX_OK);
            p2 = P; p2.pair = nullptr;
            CHECK(check_bow_rows(&prm, p2, S, O, d, d) == ORBX_ERR_ARG);
            p2 = P; p2.qvalid = nullptr; p2.claimed = nullptr;
            CHECK(check_bow_rows(&prm, p2, S, O, d, d) == ORBX_OK);
            p2 = P; p2.npairs = 306783379;                                        // ceil(2^31 / 7): npairs * cap reaches 2^31
            CHECK(check_bow_rows(&prm, p2, S, O, d, d) == ORBX_ERR_ARG);
            BowStore s2 = S;
            s2.cap = 0;
            CHECK(check_bow_rows(&prm, P, s2, O, d, d) == ORBX_ERR_ARG);
            s2.cap = ORBF_MAX_FEATURES + 1;
            CHECK(check_bow_rows(&prm, P, s2, O, d, d) == ORBX_ERR_ARG);
            s2 = S; s2.nrows = 0;
            CHECK(check_bow_rows(&prm, P, s2, O, d, d) == ORBX_ERR_ARG);
            s2 = S; s2.nrows = 268435456;                                         // nrows * (cap + 1) reaches 2^31
            CHECK(check_bow_rows(&prm, P, s2, O, d, d) == ORBX_ERR_ARG);
            const void** members[] = {(const void**)&s2.kps, (const void**)&s2.desc, (const void**)&s2.nt, (const void**)&s2.fv_node, (const void**)&s2.fv_off,
                                      (const void**)&s2.fv_feat, (const void**)&s2.nfv};
            for (const void** mbr : members) {
                s2 = S;
                *mbr = nullptr;
                CHECK(check_bow_rows(&prm, P, s2, O, d, d) == ORBX_ERR_ARG);
            }
            BowOut o2 = O;
            o2.nmatches = nullptr;
            CHECK(check_bow_rows(&prm, P, S, o2, d, d) == ORBX_ERR_ARG);
            o2 = BowOut{nullptr, nullptr, nullptr, nullptr, nm.data()};           // the four arrays are optional
            CHECK(check_bow_rows(&prm, P, S, o2, d, d) == ORBX_OK);
        }
        // alignment: device descriptors are read in 16-byte pieces, host ones are copied into an aligned slot; device outputs are words
        BowStore s2 = S;
        s2.desc = desc + 4;
        CHECK(check_bow_rows(&prm, P, s2, O, false, false) == ORBX_OK);
        CHECK(check_bow_rows(&prm, P, s2, O, false, true) == ORBX_ERR_ARG);
        BowOut o2 = O;
        o2.t2q = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(t2q.data()) + 2);
        CHECK(check_bow_rows(&prm, P, S, o2, true, true) == ORBX_ERR_ARG);
        CHECK(check_bow_rows(&prm, P, S, o2, false, false) == ORBX_OK);
        // the host form walks the pairs; the device form reports a row out of range per pair
        std::vector<int32_t> bad = pair;
        bad[3] = nrows;
        RowPairs p2 = P;
        p2.pair = bad.data();
        CHECK(check_bow_rows(&prm, p2, S, O, false, false) == ORBX_ERR_ARG);
        CHECK(check_bow_rows(&prm, p2, S, O, true, true) == ORBX_OK);
        bad[3] = 3; bad[4] = -1;
        CHECK(check_bow_rows(&prm, p2, S, O, false, false) == ORBX_ERR_ARG);
    }
    {
        // the block with everything in it: slots at multiples of 256, one span up, one down, the records behind
        const RowsBlock B(P, S, O, true);
        CHECK(B.pair.off == 0 && B.qvalid.off == 256 && B.claimed.off == 512 && B.nt.off == 768 && B.nfv.off == 1024 && B.kps.off == 1280);
        CHECK(B.desc.off == 1280 + 1024 && B.fv_node.off == 2304 + 1024 && B.fv_off.off == 3328 + 256 && B.fv_feat.off == 3584 + 256);
        const size_t up = B.L.upload();
        CHECK(up == 3840 + 256 && B.nmatches.off == up && B.q2t.off == up + 256 && B.t2q.off == up + 512 && B.best.off == up + 768 && B.second.off == up + 1024);
        CHECK(B.L.download() == 1280 && B.rec.off == up + 1280 && B.L.total() == up + 1280 + 512 && sizeof(BowRec) == 16);
        std::vector<uint8_t> h(B.L.upload() + B.L.download()), d(B.L.total());
        const BowRows a = B.stage(h.data(), d.data(), P, S);
        CHECK((const uint8_t*)a.P.pair == d.data() && a.P.qvalid == d.data() + 256 && a.P.claimed == d.data() + 512 && a.P.npairs == npairs);
        CHECK((const uint8_t*)a.S.nt == d.data() + 768 && (const uint8_t*)a.S.nfv == d.data() + 1024 && (const uint8_t*)a.S.kps == d.data() + 1280);
        CHECK(a.S.desc == d.data() + 2304 && ((uintptr_t)(a.S.desc - d.data()) & 15) == 0 && (const uint8_t*)a.S.fv_feat == d.data() + 3840);
        CHECK(a.S.nrows == nrows && a.S.cap == cap && (uint8_t*)a.O.nmatches == d.data() + up && (uint8_t*)a.O.second == d.data() + up + 1024);
        CHECK((uint8_t*)a.rec == d.data() + up + 1280 && !B.F12.present && !a.P.F12 && a.P.qstride == cap && B.nqv == (size_t)npairs * cap);
        CHECK(reinterpret_cast<const int32_t*>(h.data())[5] == 1 && h[256 + npairs * cap - 1] == 1 && h[512 + npairs * cap - 1] == 2);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + 768)[3] == 5 && reinterpret_cast<const int32_t*>(h.data() + 1024)[3] == 2);
        CHECK(reinterpret_cast<const orbx_keypoint*>(h.data() + 1280)[nrows * cap - 1].octave == nrows * cap - 1 && h[2304 + nrows * cap * 32 - 1] == 0xAB);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + 3584)[nrows * (cap + 1) - 1] == 9 && reinterpret_cast<const uint32_t*>(h.data() + 3840)[nrows * cap - 1] == 6);
        // what comes back: a null array is passed over
        for (int i = 0; i < npairs * cap; i++) { orbx::Layout::at(h.data(), B.q2t)[i] = 100 + i; orbx::Layout::at(h.data(), B.best)[i] = 200 + i; }
        for (int p = 0; p < npairs; p++) orbx::Layout::at(h.data(), B.nmatches)[p] = 10 + p;
        B.unpack(h.data(), BowOut{q2t.data(), nullptr, best.data(), nullptr, nm.data()});
        CHECK(q2t[0] == 100 && q2t[npairs * cap - 1] == 100 + npairs * cap - 1 && best[3] == 203 && t2q[0] == -7 && second[0] == -7 && nm[2] == 12);
    }
    {
        // what the caller does not pass takes no room and resolves to null; resident rows are passed through, their counts still go up
        const RowPairs p2{pair.data(), 1, nullptr, cap, nullptr, nullptr, 0, 0};
        const BowOut o2{nullptr, t2q.data(), nullptr, nullptr, nm.data()};
        const RowsBlock B(p2, S, o2, false);
        CHECK(!B.qvalid.present && !B.claimed.present && !B.kps.present && !B.desc.present && !B.fv_node.present && !B.fv_off.present && !B.fv_feat.present);
        CHECK(B.nt.present && B.nfv.present && !B.q2t.present && B.t2q.present && !B.best.present && !B.second.present);
        CHECK(B.pair.off == 0 && B.nt.off == 256 && B.nfv.off == 512 && B.L.upload() == 768 && B.nmatches.off == 768 && B.t2q.off == 1024 && B.rec.off == 1280);
        CHECK(B.L.total() == 1536);
        std::vector<uint8_t> h(B.L.upload() + B.L.download()), d(B.L.total());
        const BowRows a = B.stage(h.data(), d.data(), p2, S);
        CHECK(!a.P.qvalid && !a.P.claimed && a.S.kps == kps.data() && a.S.desc == desc && a.S.fv_node == fv_node.data() && a.S.fv_off == fv_off.data());
        CHECK(a.S.fv_feat == fv_feat.data() && (const uint8_t*)a.S.nt == d.data() + 256 && !a.O.q2t && !a.O.best && (uint8_t*)a.O.t2q == d.data() + 1024);
    }
    {
        // a FeatureVector as CSR: nodes ascending (the map's order), features in their vector's order, indices outside the row refused
        std::map<unsigned, std::vector<unsigned> > fv;
        fv[40] = {5, 1};
        fv[7] = {0, 2, 3};
        fv[90] = {4};
        std::vector<uint32_t> node(cap), feat(cap);
        std::vector<int32_t> off(cap + 1);
        CHECK(ORB_SLAM::PackFeatureVector(fv, 6, cap, node.data(), off.data(), feat.data()) == 3);
        CHECK(node[0] == 7 && node[1] == 40 && node[2] == 90 && off[0] == 0 && off[1] == 3 && off[2] == 5 && off[3] == 6);
        CHECK(feat[0] == 0 && feat[2] == 3 && feat[3] == 5 && feat[4] == 1 && feat[5] == 4);
        CHECK(ORB_SLAM::PackFeatureVector(fv, 5, cap, node.data(), off.data(), feat.data()) == -1);      // feature 5 of a row of five
        fv[91] = {6, 7};                                                                                // eight features do not fit seven slots
        CHECK(ORB_SLAM::PackFeatureVector(fv, 8, cap, node.data(), off.data(), feat.data()) == -1);
        std::map<unsigned, std::vector<unsigned> > none;
        CHECK(ORB_SLAM::PackFeatureVector(none, 0, cap, node.data(), off.data(), feat.data()) == 0 && off[0] == 0);
        std::map<unsigned, std::vector<unsigned> > many;                                                // more nodes than slots
        for (unsigned i = 0; i < 8; i++) many[i] = std::vector<unsigned>();
        CHECK(ORB_SLAM::PackFeatureVector(many, 8, cap, node.data(), off.data(), feat.data()) == -1);
    }
    std::printf("bow rows host ok\n");
    return 0;
}
