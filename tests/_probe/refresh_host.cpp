// The host side of orbp_refresh on the CPU against tests/_probe/hip_stub: the argument checks that need no handle (orbp::check_refresh) and the
// layout and staging of the call's pinned block (orbp::RefreshBlock), whose copies run over heap blocks of exactly the computed sizes
// (tests/test_refresh_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbp_host.h"

using namespace orbp;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    const int n = 5, nkf = 3, cap = 7;
    const std::vector<float> pos(n * 3, 1.5f), ow(nkf * 3, 2.5f), factors = {1.0f, 1.2f, 1.44f};
    const std::vector<int32_t> obs_off = {0, 2, 2, 5, 6, 9};
    std::vector<int32_t> obs(9 * 2), ref(n, 0);
    for (size_t i = 0; i < obs.size(); i++) obs[i] = (int32_t)i;
    const std::vector<uint8_t> skip(n, 1), bad(nkf, 0), desc((size_t)nkf * cap * 32, 0xAB);
    std::vector<orbx_keypoint> kps((size_t)nkf * cap);
    for (size_t i = 0; i < kps.size(); i++) kps[i].octave = (int)i;
    const RefreshLists L{pos.data(), obs_off.data(), obs.data(), ref.data(), skip.data()};
    const KeyFrames K{ow.data(), bad.data(), kps.data(), desc.data(), nkf, cap};
    const int both = ORBP_REFRESH_NORMAL_DEPTH | ORBP_REFRESH_DESCRIPTOR;
    {
        // the checks: host lists (obs_off is walked) and device lists (presence and alignment only)
        CHECK(check_refresh(n, L, K, factors.data(), 3, both, false, false) == ORBX_OK);
        CHECK(check_refresh(0, RefreshLists{}, K, factors.data(), 3, both, false, false) == ORBX_OK);
        CHECK(check_refresh(-1, L, K, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
        CHECK(check_refresh(n, L, K, nullptr, 3, both, false, false) == ORBX_ERR_ARG);
        CHECK(check_refresh(n, L, K, factors.data(), 1, both, false, false) == ORBX_ERR_ARG);          // GetScaleFactor() reads level 1
        CHECK(check_refresh(n, L, K, factors.data(), 2, both, false, false) == ORBX_OK);
        CHECK(check_refresh(n, L, K, factors.data(), ORBS_MAX_LEVELS + 1, both, false, false) == ORBX_ERR_ARG);
        CHECK(check_refresh(n, L, K, factors.data(), 3, 0, false, false) == ORBX_ERR_ARG);
        CHECK(check_refresh(n, L, K, factors.data(), 3, 4, false, false) == ORBX_ERR_ARG);
        KeyFrames k2 = K;
        k2.nkf = 0;
        CHECK(check_refresh(n, L, k2, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
        k2.nkf = 1 << 16; k2.cap = 1 << 15;                                                            // nkf * cap = 2^31
        CHECK(check_refresh(n, L, k2, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
        k2 = K; k2.ow = nullptr;
        CHECK(check_refresh(n, L, k2, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
        CHECK(check_refresh(n, L, k2, factors.data(), 3, ORBP_REFRESH_DESCRIPTOR, false, false) == ORBX_OK);      // the centres are not read
        k2 = K; k2.desc = nullptr;
        CHECK(check_refresh(n, L, k2, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
        CHECK(check_refresh(n, L, k2, factors.data(), 3, ORBP_REFRESH_NORMAL_DEPTH, false, false) == ORBX_OK);
        k2 = K; k2.desc = desc.data() + 4;
        CHECK(check_refresh(n, L, k2, factors.data(), 3, both, false, false) == ORBX_OK);               // a host array is copied into an aligned slot
        CHECK(check_refresh(n, L, k2, factors.data(), 3, both, false, true) == ORBX_ERR_ARG);           // a device array is read in 16-byte pieces
        RefreshLists l2 = L;
        l2.ref = nullptr;
        CHECK(check_refresh(n, l2, K, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
        CHECK(check_refresh(n, l2, K, factors.data(), 3, ORBP_REFRESH_DESCRIPTOR, false, false) == ORBX_OK);
        l2 = L; l2.obs = nullptr;
        CHECK(check_refresh(n, l2, K, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
        l2 = L; l2.obs = obs.data() + 1;
        CHECK(check_refresh(n, l2, K, factors.data(), 3, both, true, false) == ORBX_ERR_ARG);           // device pairs: one 8-byte load each
        std::vector<int32_t> down = obs_off;
        down[3] = 1;
        l2 = L; l2.obs_off = down.data();
        CHECK(check_refresh(n, l2, K, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
        CHECK(check_refresh(n, l2, K, factors.data(), 3, both, true, false) == ORBX_OK);                // device lists are not walked
        down = obs_off; down[0] = -1;
        CHECK(check_refresh(n, l2, K, factors.data(), 3, both, false, false) == ORBX_ERR_ARG);
    }
    {
        // the block with everything in it: slots at multiples of 256, one span up and the records down
        const RefreshBlock B(n, obs_off[n], L, K, true);
        CHECK(B.pos.off == 0 && B.obs_off.off == 256 && B.obs.off == 512 && B.ref.off == 768 && B.skip.off == 1024 && B.kf_ow.off == 1280 && B.kf_bad.off == 1536);
        CHECK(B.kf_kps.off == 1792 && B.kf_desc.off == 1792 + 768 && B.L.upload() == 2560 + 768 && B.out.off == B.L.upload());
        CHECK(B.L.download() == 256 && B.L.total() == B.L.upload() + 256);
        std::vector<uint8_t> h(B.L.total()), d(B.L.total());
        RefreshLists dl;
        KeyFrames dk;
        B.stage(h.data(), d.data(), L, K, dl, dk);
        CHECK((const uint8_t*)dl.pos == d.data() && (const uint8_t*)dl.obs == d.data() + 512 && (const uint8_t*)dk.desc == d.data() + 2560);
        CHECK(dk.nkf == nkf && dk.cap == cap && ((uintptr_t)((const uint8_t*)dk.desc - d.data()) & 15) == 0);
        const int32_t* ho = reinterpret_cast<const int32_t*>(h.data() + 512);
        CHECK(ho[0] == 0 && ho[17] == 17 && h[1024] == 1 && h[2560 + nkf * cap * 32 - 1] == 0xAB);
        CHECK(reinterpret_cast<const orbx_keypoint*>(h.data() + 1792)[nkf * cap - 1].octave == nkf * cap - 1);
    }
    {
        // what the caller does not pass takes no room and resolves to null; resident key frames are passed through
        const RefreshLists l2{nullptr, obs_off.data(), obs.data(), nullptr, nullptr};
        const KeyFrames k2{nullptr, nullptr, kps.data(), desc.data(), nkf, cap};
        const RefreshBlock B(n, obs_off[n], l2, k2, false);
        CHECK(!B.pos.present && !B.ref.present && !B.skip.present && !B.kf_ow.present && !B.kf_bad.present && !B.kf_kps.present && !B.kf_desc.present);
        CHECK(B.obs_off.off == 0 && B.obs.off == 256 && B.L.upload() == 512 && B.out.off == 512 && B.L.total() == 768);
        std::vector<uint8_t> h(B.L.total()), d(B.L.total());
        RefreshLists dl;
        KeyFrames dk;
        B.stage(h.data(), d.data(), l2, k2, dl, dk);
        CHECK(!dl.pos && !dl.ref && !dl.skip && !dk.ow && !dk.bad && dk.kps == kps.data() && dk.desc == desc.data());
        // points without a single observation: the pair array still has room for one element, and nothing is copied into it
        const std::vector<int32_t> zero(n + 1, 0);
        const RefreshLists l3{nullptr, zero.data(), obs.data(), nullptr, nullptr};
        const RefreshBlock E(n, 0, l3, k2, false);
        CHECK(E.L.total() == 768);
        std::vector<uint8_t> he(E.L.total()), de(E.L.total());
        E.stage(he.data(), de.data(), l3, k2, dl, dk);
        CHECK(dl.obs != nullptr);
    }
    std::printf("refresh host ok\n");
    return 0;
}
