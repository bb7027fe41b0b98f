// The host side of orbp_sim3_search on the CPU against tests/_probe/hip_stub: the argument checks that need no handle (orbp::check_sim3), the pair
// arithmetic's refusals (orbp::sim3_from_pair) and the layout, staging and unpacking of the call's pinned block (orbp::Sim3Block), whose copies run
// over heap blocks of exactly the computed sizes (tests/test_sim3_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "orbp_host.h"

using namespace orbp;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const int npairs = 2, nrows = 4, lcap = 5, nframes = 3, cap = 7;
    const orbf_bounds b{0, 640, 0, 480, 0.1f, 0.1f};
    const float R12[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, t12[3] = {1, 2, 3}, R1w[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t1w[3] = {4, 5, 6}, R2w[9] = {0, 0, 1, 1, 0, 0, 0, 1, 0},
                t2w[3] = {7, 8, 9};
    std::vector<orbp_sim3_dir> dirs(nrows);
    {
        // the pair arithmetic on numbers that are exact: sR12 = 2 R12, sR21 = R12' / 2, t21 = -sR21 t12
        CHECK(sizeof(orbp_sim3_dir) == 144 && sizeof(orbp_sim3_dir) % 16 == 0);
        CHECK(sim3_from_pair(2.0f, R12, t12, R1w, t1w, R2w, t2w, 500.f, 501.f, 320.f, 240.f, &b, 7.5f, dirs.data()) == ORBX_OK);
        const orbp_sim3_dir &d21 = dirs[0], &d12 = dirs[1];
        CHECK(d21.Raw[0] == 1 && d21.taw[2] == 6 && d12.Raw[2] == 1 && d12.taw[0] == 7);
        CHECK(d12.S[1] == -2 && d12.S[3] == 2 && d12.S[8] == 2 && d12.t[0] == 1 && d12.t[2] == 3);
        CHECK(d21.S[1] == 0.5f && d21.S[3] == -0.5f && d21.S[8] == 0.5f && d21.t[0] == -1 && d21.t[1] == 0.5f && d21.t[2] == -1.5f);
        for (const orbp_sim3_dir& d : {d21, d12})
            CHECK(d.fx == 500.f && d.fy == 501.f && d.cx == 320.f && d.cy == 240.f && d.min_x == 0 && d.max_x == 640 && d.max_y == 480 && d.th == 7.5f &&
                  d.mode == ORBP_MODE_SIM3 && d.reserved[0] == 0 && d.reserved[1] == 0);
        dirs[2] = dirs[0]; dirs[3] = dirs[1];
        // refusals leave the records alone
        std::vector<orbp_sim3_dir> keep = dirs;
        for (float s : {0.0f, -0.0f, std::numeric_limits<float>::infinity(), std::nanf("")})
            CHECK(sim3_from_pair(s, R12, t12, R1w, t1w, R2w, t2w, 1, 1, 1, 1, &b, 1, dirs.data()) == ORBX_ERR_ARG);
        CHECK(sim3_from_pair(1, nullptr, t12, R1w, t1w, R2w, t2w, 1, 1, 1, 1, &b, 1, dirs.data()) == ORBX_ERR_ARG);
        CHECK(sim3_from_pair(1, R12, t12, R1w, t1w, R2w, nullptr, 1, 1, 1, 1, &b, 1, dirs.data()) == ORBX_ERR_ARG);
        CHECK(sim3_from_pair(1, R12, t12, R1w, t1w, R2w, t2w, 1, 1, 1, 1, nullptr, 1, dirs.data()) == ORBX_ERR_ARG);
        CHECK(sim3_from_pair(1, R12, t12, R1w, t1w, R2w, t2w, 1, 1, 1, 1, &b, 1, nullptr) == ORBX_ERR_ARG);
        CHECK(std::memcmp(keep.data(), dirs.data(), sizeof(orbp_sim3_dir) * nrows) == 0);
        CHECK(sim3_from_pair(-1.0f, R12, t12, R1w, t1w, R2w, t2w, 1, 1, 1, 1, &b, 1, keep.data()) == ORBX_OK);      // a reflection is the caller's business
    }
    const std::vector<float> factors = {1.0f, 1.2f, 1.44f};
    std::vector<int32_t> list(nrows * lcap), nlist = {5, 0, 3, 9}, frame = {1, 0, 2, 1}, nt = {7, 2, 0};
    for (size_t i = 0; i < list.size(); i++) list[i] = (int32_t)i;
    const std::vector<uint8_t> skip(nrows * lcap, 1);
    std::vector<uint8_t> desc_store((size_t)nframes * cap * 32 + 16, 0xAB);
    uint8_t* desc = desc_store.data() + ((16 - ((uintptr_t)desc_store.data() & 15)) & 15);         // 16-byte aligned
    std::vector<orbx_keypoint> kps((size_t)nframes * cap);
    for (size_t i = 0; i < kps.size(); i++) kps[i].octave = (int)i;
    std::vector<int32_t> cell_off((size_t)nframes * (ORBF_GRID_CELLS + 1), 3), cell_feat((size_t)nframes * cap, 4);
    cell_off.back() = 9;
    std::vector<int32_t> best_idx(nrows * lcap, -7), best_dist(nrows * lcap, -7), match12(npairs * lcap + 1, -7), nfound(npairs, -7);
    std::vector<orbp_fused> rec(nrows * lcap);
    const Lists L{list.data(), nlist.data(), lcap, skip.data()};
    const FuseFrames K{kps.data(), desc, cell_off.data(), cell_feat.data(), nt.data(), nframes, cap, frame.data()};
    const FuseOut O{best_idx.data(), best_dist.data(), rec.data()};
    const float* f = factors.data();
    const int32_t *m12 = match12.data(), *nf = nfound.data();
    {
        // the checks, host form and device form
        for (int dev = 0; dev < 2; dev++) {
            const bool d = dev != 0;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, K, O, m12, nf, d, d) == ORBX_OK);
            CHECK(check_sim3(nullptr, 0, f, 3, Lists{nullptr, nullptr, 1, nullptr}, &b, 100, FuseFrames{nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr},
                             FuseOut{nullptr, nullptr, nullptr}, nullptr, nullptr, d, d) == ORBX_OK);                    // no pairs: nothing is looked at
            CHECK(check_sim3(dirs.data(), -1, f, 3, L, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), ORBP_MAX_VIEWS / 2 + 1, f, 3, L, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(nullptr, npairs, f, 3, L, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), npairs, nullptr, 3, L, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), npairs, f, 0, L, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), npairs, f, 1, L, &b, 100, K, O, m12, nf, d, d) == ORBX_OK);                   // one level is a pyramid
            CHECK(check_sim3(dirs.data(), npairs, f, ORBS_MAX_LEVELS + 1, L, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, nullptr, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, -1, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 256, K, O, m12, nf, d, d) == ORBX_OK);
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 257, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, K, O, nullptr, nf, d, d) == ORBX_ERR_ARG);
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, K, O, m12, nullptr, d, d) == ORBX_ERR_ARG);
            Lists l2 = L;
            l2.lcap = 0;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, l2, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            l2 = L; l2.list = nullptr;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, l2, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            l2 = L; l2.nlist = nullptr;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, l2, &b, 100, K, O, m12, nf, d, d) == ORBX_ERR_ARG);
            l2 = L; l2.skip = nullptr;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, l2, &b, 100, K, O, m12, nf, d, d) == ORBX_OK);
            FuseFrames k2 = K;
            k2.cap = 0;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.cap = ORBF_MAX_FEATURES + 1;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.nframes = 0;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.desc = nullptr;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.nt = nullptr;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, d, d) == ORBX_ERR_ARG);
            FuseOut o2 = O;
            o2.best_idx = nullptr;                                         // the directions' own outputs: required on the device, optional in the host form
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, K, o2, m12, nf, d, d) == (d ? ORBX_ERR_ARG : ORBX_OK));
            o2 = O; o2.rec = nullptr;
            CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, K, o2, m12, nf, d, d) == ORBX_OK);
        }
        // alignment: device descriptors are read in 16-byte pieces, host ones are copied into an aligned slot; the agreement's outputs are words
        FuseFrames k2 = K;
        k2.desc = desc + 4;
        CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, false, false) == ORBX_OK);
        CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, false, true) == ORBX_ERR_ARG);
        const int32_t* odd = reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(m12) + 2);
        CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, K, O, odd, nf, true, true) == ORBX_ERR_ARG);
        CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, K, O, odd, nf, false, false) == ORBX_OK);
        // the host form walks the rows: a mode that is not ORBP_MODE_SIM3, a key frame out of range; the device form reports those per row
        std::vector<orbp_sim3_dir> v2 = dirs;
        v2[3].mode = ORBP_MODE_FUSE;
        CHECK(check_sim3(v2.data(), npairs, f, 3, L, &b, 100, K, O, m12, nf, false, false) == ORBX_ERR_ARG);
        CHECK(check_sim3(v2.data(), npairs, f, 3, L, &b, 100, K, O, m12, nf, true, true) == ORBX_OK);
        std::vector<int32_t> fr2 = frame;
        fr2[2] = nframes;
        k2 = K; k2.frame = fr2.data();
        CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, false, false) == ORBX_ERR_ARG);
        k2.frame = nullptr;                                                    // row r searches key frame r, and there are three
        CHECK(check_sim3(dirs.data(), npairs, f, 3, L, &b, 100, k2, O, m12, nf, false, false) == ORBX_ERR_ARG);
    }
    {
        // the block with everything in it: slots at multiples of 256, one span up, the directions' results and the agreement's down
        const Sim3Block B(npairs, L, K, true, true);
        CHECK(B.nviews == nrows && B.npairs == npairs);
        CHECK(B.views.off == 0 && B.nlist.off == 768 && B.frame.off == 1024 && B.nt.off == 1280 && B.list.off == 1536 && B.skip.off == 1792);
        CHECK(B.kps.off == 2048 && B.desc.off == 2048 + 768 && B.cell_off.off == 2816 + 768);
        const size_t off_bytes = ((size_t)nframes * (ORBF_GRID_CELLS + 1) * 4 + 255) & ~(size_t)255;
        CHECK(B.cell_feat.off == 3584 + off_bytes && B.L.upload() == 3584 + off_bytes + 256 && B.best_idx.off == B.L.upload());
        const size_t up = B.L.upload();
        CHECK(B.best_dist.off == up + 256 && B.rec.off == up + 512 && B.match12.off == up + 1024 && B.nfound.off == up + 1280 && B.L.download() == 1536);
        CHECK(B.L.total() == up + 1536);
        std::vector<uint8_t> h(B.L.total()), d(B.L.total());
        const orbp_sim3_dir* dv;
        Lists dl;
        FuseFrames dk;
        FuseOut dout;
        B.stage(h.data(), d.data(), dirs.data(), L, K, dv, dl, dk, dout);
        CHECK((const uint8_t*)dv == d.data() && (const uint8_t*)dl.nlist == d.data() + 768 && (const uint8_t*)dk.frame == d.data() + 1024);
        CHECK((const uint8_t*)dk.nt == d.data() + 1280 && (const uint8_t*)dl.list == d.data() + 1536 && dl.skip == d.data() + 1792 && dl.lcap == lcap);
        CHECK((const uint8_t*)dk.kps_un == d.data() + 2048 && dk.desc == d.data() + 2816 && ((uintptr_t)(dk.desc - d.data()) & 15) == 0);
        CHECK(dk.nframes == nframes && dk.cap == cap && (uint8_t*)dout.best_idx == d.data() + up && (uint8_t*)dout.rec == d.data() + up + 512);
        CHECK((uint8_t*)Layout::at(d.data(), B.match12) == d.data() + up + 1024 && (uint8_t*)Layout::at(d.data(), B.nfound) == d.data() + up + 1280);
        CHECK(reinterpret_cast<const orbp_sim3_dir*>(h.data())[3].S[1] == -2 && reinterpret_cast<const int32_t*>(h.data() + 768)[3] == 9);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + 1024)[2] == 2 && reinterpret_cast<const int32_t*>(h.data() + 1280)[1] == 2);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + 1536)[nrows * lcap - 1] == nrows * lcap - 1 && h[1792 + nrows * lcap - 1] == 1);
        CHECK(reinterpret_cast<const orbx_keypoint*>(h.data() + 2048)[nframes * cap - 1].octave == nframes * cap - 1 && h[2816 + nframes * cap * 32 - 1] == 0xAB);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + B.cell_feat.off)[nframes * cap - 1] == 4);
        // what comes back: only the entries inside the (clamped) lists, a null array passed over
        for (int i = 0; i < nrows * lcap; i++) { Layout::at(h.data(), B.best_idx)[i] = 100 + i; Layout::at(h.data(), B.best_dist)[i] = 200 + i; }
        B.unpack(h.data(), L, FuseOut{best_idx.data(), nullptr, nullptr});
        CHECK(best_idx[0] == 100 && best_idx[4] == 104 && best_idx[5] == -7 && best_idx[10] == 110 && best_idx[12] == 112 && best_idx[13] == -7);
        CHECK(best_idx[15] == 115 && best_idx[19] == 119 && best_dist[0] == -7);                    // nlist 9 is clamped to lcap
    }
    {
        // what the caller does not pass takes no room and resolves to null; resident key frames are passed through
        const Lists l2{list.data(), nlist.data(), lcap, nullptr};
        const FuseFrames k2{kps.data(), desc, cell_off.data(), cell_feat.data(), nt.data(), nframes, cap, nullptr};
        const Sim3Block B(1, l2, k2, false, false);
        CHECK(!B.frame.present && !B.skip.present && !B.kps.present && !B.desc.present && !B.cell_off.present && !B.cell_feat.present && !B.rec.present);
        CHECK(B.match12.present && B.nfound.present);
        CHECK(B.views.off == 0 && B.nlist.off == 512 && B.nt.off == 768 && B.list.off == 1024 && B.L.upload() == 1280 && B.best_dist.off == 1536 &&
              B.match12.off == 1792 && B.nfound.off == 2048 && B.L.total() == 2304);
        std::vector<uint8_t> h(B.L.total()), d(B.L.total());
        const orbp_sim3_dir* dv;
        Lists dl;
        FuseFrames dk;
        FuseOut dout;
        B.stage(h.data(), d.data(), dirs.data(), l2, k2, dv, dl, dk, dout);
        CHECK(!dl.skip && !dk.frame && !dout.rec && dk.kps_un == kps.data() && dk.desc == desc && dk.cell_off == cell_off.data() && dk.cell_feat == cell_feat.data());
        CHECK((const uint8_t*)dk.nt == d.data() + 768);
        // the fuse block is the same layout without the agreement's two slots
        const FuseBlock F(2, l2, k2, false, false);
        CHECK(!F.match12.present && !F.nfound.present && F.L.total() == 1536);
    }
    std::printf("sim3 host ok\n");
    return 0;
}
