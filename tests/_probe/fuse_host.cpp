// The host side of orbp_fuse on the CPU against tests/_probe/hip_stub: the argument checks that need no handle (orbp::check_fuse) and the
// layout and staging of the call's pinned block (orbp::FuseBlock), whose copies run over heap blocks of exactly the computed sizes
// (tests/test_fuse_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbp_host.h"

using namespace orbp;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const int nviews = 3, lcap = 5, nframes = 2, cap = 7;
    std::vector<orbp_view> views(nviews);
    for (int p = 0; p < nviews; p++) { views[p] = orbp_view{}; views[p].mode = ORBP_MODE_FUSE; views[p].th = 2.5f + p; }
    const std::vector<float> factors = {1.0f, 1.2f, 1.44f};
    std::vector<int32_t> list(nviews * lcap), nlist = {5, 0, 3}, frame = {1, 0, 1}, nt = {7, 2};
    for (size_t i = 0; i < list.size(); i++) list[i] = (int32_t)i;
    const std::vector<uint8_t> skip(nviews * lcap, 1);
    std::vector<uint8_t> desc_store((size_t)nframes * cap * 32 + 16, 0xAB);
    uint8_t* desc = desc_store.data() + ((16 - ((uintptr_t)desc_store.data() & 15)) & 15);         // 16-byte aligned
    std::vector<orbx_keypoint> kps((size_t)nframes * cap);
    for (size_t i = 0; i < kps.size(); i++) kps[i].octave = (int)i;
    std::vector<int32_t> cell_off((size_t)nframes * (ORBF_GRID_CELLS + 1), 3), cell_feat((size_t)nframes * cap, 4);
    cell_off.back() = 9;
    std::vector<int32_t> best_idx(nviews * lcap), best_dist(nviews * lcap);
    std::vector<orbp_fused> rec(nviews * lcap);
    const orbf_bounds b{0, 640, 0, 480, 0.1f, 0.1f};
    const Lists L{list.data(), nlist.data(), lcap, skip.data()};
    const FuseFrames K{kps.data(), desc, cell_off.data(), cell_feat.data(), nt.data(), nframes, cap, frame.data()};
    const FuseOut O{best_idx.data(), best_dist.data(), rec.data()};
    const float* f = factors.data();
    {
        // the checks, host form and device form
        for (int dev = 0; dev < 2; dev++) {
            const bool d = dev != 0;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, K, O, d, d) == ORBX_OK);
            CHECK(check_fuse(nullptr, 0, f, 3, Lists{nullptr, nullptr, 1, nullptr}, &b, 50, FuseFrames{nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr},
                             FuseOut{}, d, d) == ORBX_OK);                                               // no views: nothing else is looked at
            CHECK(check_fuse(views.data(), -1, f, 3, L, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            CHECK(check_fuse(views.data(), ORBP_MAX_VIEWS + 1, f, 3, L, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            CHECK(check_fuse(nullptr, nviews, f, 3, L, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            CHECK(check_fuse(views.data(), nviews, nullptr, 3, L, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            CHECK(check_fuse(views.data(), nviews, f, 0, L, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            CHECK(check_fuse(views.data(), nviews, f, 1, L, &b, 50, K, O, d, d) == ORBX_OK);              // one level is a pyramid
            CHECK(check_fuse(views.data(), nviews, f, ORBS_MAX_LEVELS + 1, L, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            CHECK(check_fuse(views.data(), nviews, f, 3, L, nullptr, 50, K, O, d, d) == ORBX_ERR_ARG);
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, -1, K, O, d, d) == ORBX_ERR_ARG);
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 0, K, O, d, d) == ORBX_OK);
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 256, K, O, d, d) == ORBX_OK);
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 257, K, O, d, d) == ORBX_ERR_ARG);
            Lists l2 = L;
            l2.lcap = 0;
            CHECK(check_fuse(views.data(), nviews, f, 3, l2, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            l2 = L; l2.lcap = 1 << 30;                                                                   // nviews * lcap >= 2^31
            CHECK(check_fuse(views.data(), nviews, f, 3, l2, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            l2 = L; l2.list = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, l2, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            l2 = L; l2.nlist = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, l2, &b, 50, K, O, d, d) == ORBX_ERR_ARG);
            l2 = L; l2.skip = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, l2, &b, 50, K, O, d, d) == ORBX_OK);
            FuseFrames k2 = K;
            k2.cap = 0;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2.cap = ORBF_MAX_FEATURES + 1;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.nframes = 0;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.nframes = 1 << 18; k2.cap = ORBF_MAX_FEATURES;                                      // nframes * cap = 2^31
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.kps_un = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.desc = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.cell_off = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.cell_feat = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.nt = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == ORBX_ERR_ARG);
            k2 = K; k2.frame = nullptr;                                                                  // view p searches key frame p ...
            CHECK(check_fuse(views.data(), 2, f, 3, L, &b, 50, k2, O, d, d) == ORBX_OK);
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, d, d) == (d ? ORBX_OK : ORBX_ERR_ARG));   // ... and there are two: the device form reports it per entry
            FuseOut o2 = O;
            o2.best_idx = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, K, o2, d, d) == ORBX_ERR_ARG);
            o2 = O; o2.best_dist = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, K, o2, d, d) == ORBX_ERR_ARG);
            o2 = O; o2.rec = nullptr;
            CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, K, o2, d, d) == ORBX_OK);
        }
        // alignment: device descriptors are read in 16-byte pieces, host ones are copied into an aligned slot
        FuseFrames k2 = K;
        k2.desc = desc + 4;
        CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, false, false) == ORBX_OK);
        CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, false, true) == ORBX_ERR_ARG);
        k2 = K; k2.cell_feat = reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(cell_feat.data()) + 2);
        CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, false, true) == ORBX_ERR_ARG);
        Lists l2 = L;
        l2.list = reinterpret_cast<const int32_t*>(reinterpret_cast<const uint8_t*>(list.data()) + 1);
        CHECK(check_fuse(views.data(), nviews, f, 3, l2, &b, 50, K, O, true, true) == ORBX_ERR_ARG);
        FuseOut o2 = O;
        o2.rec = reinterpret_cast<orbp_fused*>(reinterpret_cast<uint8_t*>(rec.data()) + 2);
        CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, K, o2, true, true) == ORBX_ERR_ARG);
        // the host form walks the views: a mode that is not ORBP_MODE_FUSE, a key frame out of range
        std::vector<orbp_view> v2 = views;
        v2[1].mode = ORBP_MODE_FRAME;
        CHECK(check_fuse(v2.data(), nviews, f, 3, L, &b, 50, K, O, false, false) == ORBX_ERR_ARG);
        CHECK(check_fuse(v2.data(), nviews, f, 3, L, &b, 50, K, O, true, true) == ORBX_OK);
        std::vector<int32_t> fr2 = frame;
        fr2[2] = nframes;
        k2 = K; k2.frame = fr2.data();
        CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, false, false) == ORBX_ERR_ARG);
        fr2[2] = -1;
        CHECK(check_fuse(views.data(), nviews, f, 3, L, &b, 50, k2, O, false, false) == ORBX_ERR_ARG);
    }
    {
        // the block with everything in it: slots at multiples of 256, one span up and the results down
        const FuseBlock B(nviews, L, K, true, true);
        CHECK(sizeof(orbp_view) == 108 && sizeof(orbp_fused) == 16);
        CHECK(B.views.off == 0 && B.nlist.off == 512 && B.frame.off == 768 && B.nt.off == 1024 && B.list.off == 1280 && B.skip.off == 1536);
        CHECK(B.kps.off == 1792 && B.desc.off == 1792 + 512 && B.cell_off.off == 2304 + 512);
        const size_t off_bytes = ((size_t)nframes * (ORBF_GRID_CELLS + 1) * 4 + 255) & ~(size_t)255;
        CHECK(B.cell_feat.off == 2816 + off_bytes && B.L.upload() == 2816 + off_bytes + 256 && B.best_idx.off == B.L.upload());
        CHECK(B.best_dist.off == B.L.upload() + 256 && B.rec.off == B.L.upload() + 512 && B.L.download() == 768 && B.L.total() == B.L.upload() + 768);
        std::vector<uint8_t> h(B.L.total()), d(B.L.total());
        const orbp_view* dv;
        Lists dl;
        FuseFrames dk;
        FuseOut dout;
        B.stage(h.data(), d.data(), views.data(), L, K, dv, dl, dk, dout);
        CHECK((const uint8_t*)dv == d.data() && (const uint8_t*)dl.nlist == d.data() + 512 && (const uint8_t*)dk.frame == d.data() + 768);
        CHECK((const uint8_t*)dk.nt == d.data() + 1024 && (const uint8_t*)dl.list == d.data() + 1280 && dl.skip == d.data() + 1536 && dl.lcap == lcap);
        CHECK((const uint8_t*)dk.kps_un == d.data() + 1792 && dk.desc == d.data() + 2304 && ((uintptr_t)(dk.desc - d.data()) & 15) == 0);
        CHECK(dk.nframes == nframes && dk.cap == cap && (uint8_t*)dout.best_idx == d.data() + B.L.upload() && (uint8_t*)dout.rec == d.data() + B.L.upload() + 512);
        CHECK(reinterpret_cast<const orbp_view*>(h.data())[2].th == 4.5f && reinterpret_cast<const int32_t*>(h.data() + 512)[2] == 3);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + 768)[0] == 1 && reinterpret_cast<const int32_t*>(h.data() + 1024)[1] == 2);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + 1280)[nviews * lcap - 1] == nviews * lcap - 1 && h[1536 + nviews * lcap - 1] == 1);
        CHECK(reinterpret_cast<const orbx_keypoint*>(h.data() + 1792)[nframes * cap - 1].octave == nframes * cap - 1 && h[2304 + nframes * cap * 32 - 1] == 0xAB);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + 2816)[nframes * (ORBF_GRID_CELLS + 1) - 1] == 9);
        CHECK(reinterpret_cast<const int32_t*>(h.data() + B.cell_feat.off)[nframes * cap - 1] == 4);
    }
    {
        // what the caller does not pass takes no room and resolves to null; resident key frames are passed through
        const Lists l2{list.data(), nlist.data(), lcap, nullptr};
        const FuseFrames k2{kps.data(), desc, cell_off.data(), cell_feat.data(), nt.data(), nframes, cap, nullptr};
        const FuseBlock B(2, l2, k2, false, false);
        CHECK(!B.frame.present && !B.skip.present && !B.kps.present && !B.desc.present && !B.cell_off.present && !B.cell_feat.present && !B.rec.present);
        CHECK(B.views.off == 0 && B.nlist.off == 256 && B.nt.off == 512 && B.list.off == 768 && B.L.upload() == 1024 && B.best_dist.off == 1280 && B.L.total() == 1536);
        std::vector<uint8_t> h(B.L.total()), d(B.L.total());
        const orbp_view* dv;
        Lists dl;
        FuseFrames dk;
        FuseOut dout;
        B.stage(h.data(), d.data(), views.data(), l2, k2, dv, dl, dk, dout);
        CHECK(!dl.skip && !dk.frame && !dout.rec && dk.kps_un == kps.data() && dk.desc == desc && dk.cell_off == cell_off.data() && dk.cell_feat == cell_feat.data());
        CHECK((const uint8_t*)dk.nt == d.data() + 512);
    }
    std::printf("fuse host ok\n");
    return 0;
}
