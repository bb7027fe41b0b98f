// The host side of orbp_loop_* on the CPU against tests/_probe/hip_stub: orbp_view_from_sim3's arithmetic on a few fixed inputs, the argument
// checks that need no handle (orbp::check_loop_project, check_loop_search, check_loop_one), the layout of the one-view call's block
// (orbp::LoopBlock over orbp::OneView, whose stage() and unpack() run here) and its path through orbx::Staged: the upload and download spans
// are exact, with sentinels around them, and a block that must grow waits for the chain first (tests/test_loop_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer).
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "orbp_host.h"

using namespace orbp;
using orbx::Block;
using orbx::Call;
using orbx::Chain;
using orbx::Staged;
using orbx::Stream;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {
// what orbx::Call and orbx::Staged want of a handle
struct Handle {
    int device = 0;
    std::mutex mu;
    std::string err;
    Stream own;
    Chain chain;
    Block block;
};

bool all(const uint8_t* p, size_t n, uint8_t v) {
    for (size_t i = 0; i < n; i++)
        if (p[i] != v) return false;
    return true;
}

// One orbp_loop_search over `m`'s block as orbp_project.hip writes it, the body standing in for the kernels: it checks what went up and answers
// into the download span.  Every byte no copy may touch holds a sentinel.  at_fill: the HIP calls up to the first write into the pinned block.
int one_view_call(Handle& m, int nt, int nlist, int qcap, bool with_skip, bool with_claimed, bool frame_host, bool with_t2slot, bool with_rec, std::string& at_fill,
                  std::string& log) {
    const int cap = nt > 1 ? nt : 1, lcap = nlist > 1 ? nlist : 1;
    orbp_view view{};
    view.mode = ORBP_MODE_LOOP;
    view.th = 10.0f;
    std::vector<int32_t> list(lcap, 7), cell_off(ORBF_GRID_CELLS + 1, 5), cell_feat(cap, 6);
    std::vector<uint8_t> skip(lcap, 1), claimed(cap, 2), desc((size_t)cap * 32, 0xCD);
    std::vector<orbx_keypoint> kps(cap);
    for (int i = 0; i < cap; i++) kps[i].octave = i;
    hip_stub_log.clear();
    hip_stub_up = hip_stub_down = {};
    Call<Handle> c(&m, nullptr);
    const LoopBlock B(cap, lcap, qcap, {with_skip, with_claimed, frame_host, with_t2slot, with_rec});
    const size_t up = B.L.upload(), down = B.L.download(), total = B.L.total();
    Staged<Handle> s(c, m.block, B.L);
    CHECK(s.fit() == ORBX_OK);
    at_fill = hip_stub_log;
    const size_t hsize = m.block.h.size(), dsize = m.block.d.size();
    CHECK(hsize >= up + down && dsize >= total);
    std::memset(s.h, 0x11, up);                                       // padding between the slots goes up as it is
    std::memset(s.h + up, 0xA5, hsize - up);
    std::memset(s.d, 0x33, dsize);
    std::vector<int32_t> t2pos(cap, -5), t2slot(cap, -5);
    std::vector<orbp_fused> rec(lcap);
    std::memset(rec.data(), 0x77, rec.size() * sizeof(orbp_fused));
    int nmatches = -5, nvisible = -5;
    const Frame frame{kps.data(), desc.data(), cell_off.data(), cell_feat.data(), nullptr, cap, with_claimed ? claimed.data() : nullptr};
    const OneViewCall io{&view, list.data(), nlist, with_skip ? skip.data() : nullptr, frame, nt, t2pos.data(), with_t2slot ? t2slot.data() : nullptr, &nmatches, &nvisible};
    Lists dl;
    Frame fr;
    B.stage(s.h, s.d, io, dl, fr);
    const int32_t* d_counts = Layout::at(s.d, B.counts);
    const uint8_t* d_claimed = fr.claimed;
    bool body_ok = false;
    const int rc = s.run([&] {
        const uint8_t* d = s.d;
        body_ok = hip_stub_log.back() == 'u' && all(s.d + up, dsize - up, 0x33);                              // nothing behind the upload span was touched
        body_ok = body_ok && reinterpret_cast<const orbp_view*>(d)->th == 10.0f && d_counts[0] == nt && d_counts[1] == nlist && dl.nlist[0] == nlist;
        body_ok = body_ok && (nlist == 0 || dl.list[nlist - 1] == 7) && (!with_skip ? dl.skip == nullptr : (nlist == 0 || dl.skip[nlist - 1] == 1));
        body_ok = body_ok && (!with_claimed ? d_claimed == nullptr : (d_claimed >= d && d_claimed < d + up && (nt == 0 || d_claimed[nt - 1] == 2)));
        if (frame_host) {
            body_ok = body_ok && (const uint8_t*)fr.kps_un >= d && (const uint8_t*)fr.cell_feat < d + up && ((uintptr_t)(fr.desc - d) & 15) == 0;
            body_ok = body_ok && fr.cell_off[ORBF_GRID_CELLS] == 5 && (nt == 0 || (fr.kps_un[nt - 1].octave == nt - 1 && fr.desc[(size_t)nt * 32 - 1] == 0xCD && fr.cell_feat[nt - 1] == 6));
        } else {
            body_ok = body_ok && fr.kps_un == kps.data() && fr.desc == desc.data() && fr.cell_off == cell_off.data() && fr.cell_feat == cell_feat.data();
        }
        body_ok = body_ok && fr.nt == d_counts && fr.cap == cap;
        // the device-only tail lies behind the download span and inside the block
        const Queries q = B.dev.q.at(s.d);
        body_ok = body_ok && (uint8_t*)q.qxyr >= s.d + up + down && (uint8_t*)Layout::at(s.d, B.dev.tile_count) + (size_t)loop_tiles(lcap) * 4 <= s.d + total;
        body_ok = body_ok && (with_rec ? !B.dev.rec.present && B.rec.present : B.dev.rec.present && !B.rec.present) && !B.dev.g_kps.present && q.qangle == nullptr;
        std::memset(s.d + up, 0x22, down);
        return (int)ORBX_OK;
    });
    log = hip_stub_log;
    CHECK(rc == ORBX_OK && body_ok);
    CHECK(hip_stub_up.dst == s.d && hip_stub_up.src == s.h && hip_stub_up.bytes == up);
    CHECK(hip_stub_down.dst == s.h + up && hip_stub_down.src == s.d + up && hip_stub_down.bytes == down);
    CHECK(all(s.h + up, down, 0x22) && all(s.h + up + down, hsize - up - down, 0xA5) && all(s.d + up + down, dsize - up - down, 0x33));
    // unpack: the result words 0x22222222 mean an overflow, which still reports the visible count and copies nothing else
    CHECK(B.unpack(s.h, io, with_rec ? rec.data() : nullptr) == ORBX_ERR_CAPACITY && nvisible == 0x22222222 && nmatches == -5 && t2pos[0] == -5);
    Layout::at(s.h, B.result)[1] = 0;
    CHECK(B.unpack(s.h, io, with_rec ? rec.data() : nullptr) == ORBX_OK && nmatches == 0x22222222);
    const bool rec_copied = rec[0].status == 0x22222222 && rec[nlist > 0 ? nlist - 1 : 0].level == 0x22222222;
    CHECK(nt > 0 ? t2pos[nt - 1] == 0x22222222 : t2pos[0] == -5);
    CHECK(nt > 0 && with_t2slot ? t2slot[nt - 1] == 0x22222222 : t2slot[0] == -5);
    CHECK(with_rec && nlist > 0 ? rec_copied : rec[0].status == 0x77777777);
    return 0;
}

// the sizes of the block before the one-view forms shared a layout, per flag combination this probe goes through: before -> now
int same_sizes(int cap, int lcap, int qcap, const LoopBlock::Flags& f, size_t up, size_t down, size_t total) {
    const LoopBlock B(cap, lcap, qcap, f);
    std::printf("loop block: upload %zu -> %zu, download %zu -> %zu, total %zu -> %zu\n", up, B.L.upload(), down, B.L.download(), total, B.L.total());
    CHECK(B.L.upload() <= up && B.L.download() <= down && B.L.total() <= total);
    return 0;
}
}  // namespace

int main() {
    {
        // orbp_view_from_sim3: exact cases, and what it refuses; the other fields stay
        orbp_view v{};
        v.fx = 3.0f; v.th = 10.0f; v.mode = ORBP_MODE_LOOP;
        const float S[12] = {0, -2, 0, 4, 2, 0, 0, 6, 0, 0, 2, -8};                                            // 2 * [Rz(90) | (2, 3, -4)]
        CHECK(view_from_sim3(S, &v) == ORBX_OK);
        const float R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
        for (int i = 0; i < 9; i++) CHECK(v.Rcw[i] == R[i]);
        CHECK(v.tcw[0] == 2.0f && v.tcw[1] == 3.0f && v.tcw[2] == -4.0f && v.Ow[0] == -3.0f && v.Ow[1] == 2.0f && v.Ow[2] == 4.0f);
        CHECK(v.fx == 3.0f && v.th == 10.0f && v.mode == ORBP_MODE_LOOP);
        const orbp_view before = v;
        float Z[12] = {0, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3};
        CHECK(view_from_sim3(Z, &v) == ORBX_ERR_ARG && std::memcmp(&v, &before, sizeof(v)) == 0);              // scw == 0
        Z[0] = std::numeric_limits<float>::quiet_NaN();
        CHECK(view_from_sim3(Z, &v) == ORBX_ERR_ARG);
        Z[0] = std::numeric_limits<float>::infinity();
        CHECK(view_from_sim3(Z, &v) == ORBX_ERR_ARG);
        Z[0] = 3e38f; Z[1] = 3e38f;                                                                            // the double sum is finite, its root is not a float
        CHECK(view_from_sim3(Z, &v) == ORBX_ERR_ARG && std::memcmp(&v, &before, sizeof(v)) == 0);
        CHECK(view_from_sim3(nullptr, &v) == ORBX_ERR_ARG && view_from_sim3(S, nullptr) == ORBX_ERR_ARG);
    }
    const int nviews = 3, lcap = 600, nframes = 2, cap = 7, qcap = 16;
    std::vector<orbp_view> views(nviews);
    const std::vector<float> factors = {1.0f, 1.2f, 1.44f};
    const float* f = factors.data();
    std::vector<int32_t> list(nviews * lcap), nlist(nviews), frame(nviews), nt(nframes), ints(4096);
    std::vector<uint8_t> skip(nviews * lcap), claimed(nviews * cap);
    std::vector<uint8_t> desc_store((size_t)nframes * cap * 32 + 16), qdesc_store((size_t)nviews * qcap * 32 + 16);
    uint8_t* desc = desc_store.data() + ((16 - ((uintptr_t)desc_store.data() & 15)) & 15);
    uint8_t* qdesc = qdesc_store.data() + ((16 - ((uintptr_t)qdesc_store.data() & 15)) & 15);
    std::vector<orbx_keypoint> kps((size_t)nframes * cap);
    std::vector<int32_t> cell_off((size_t)nframes * (ORBF_GRID_CELLS + 1)), cell_feat((size_t)nframes * cap);
    std::vector<orbp_fused> rec(nviews * lcap);
    std::vector<float> qxyr(nviews * qcap * 3);
    const orbf_bounds b{0, 640, 0, 480, 0.1f, 0.1f};
    const Lists L{list.data(), nlist.data(), lcap, skip.data()};
    auto off1 = [](auto* p) { return reinterpret_cast<decltype(p)>(reinterpret_cast<uintptr_t>(p) + 1); };       // a misaligned address (never read)
    {
        // orbp_loop_project_batch_device
        const Queries Q{qxyr.data(), ints.data(), qdesc, ints.data()};
        int32_t *nq = ints.data(), *ov = ints.data();
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, rec.data(), Q, nq, ov, qcap) == ORBX_OK);
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, Q, nq, ov, qcap) == ORBX_OK);          // no records
        CHECK(check_loop_project(nullptr, 0, f, 3, Lists{nullptr, nullptr, 1, nullptr}, nullptr, Queries{}, nullptr, nullptr, 1) == ORBX_OK);   // no views
        CHECK(check_loop_project(views.data(), -1, f, 3, L, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(views.data(), ORBP_MAX_VIEWS + 1, f, 3, L, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(nullptr, nviews, f, 3, L, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(views.data(), nviews, nullptr, 3, L, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(views.data(), nviews, f, 0, L, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(views.data(), nviews, f, 1, L, nullptr, Q, nq, ov, qcap) == ORBX_OK);
        CHECK(check_loop_project(views.data(), nviews, f, ORBS_MAX_LEVELS + 1, L, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, Q, nq, ov, 0) == ORBX_ERR_ARG);
        Lists l2 = L;
        l2.lcap = 0;
        CHECK(check_loop_project(views.data(), nviews, f, 3, l2, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        l2 = L; l2.lcap = 1 << 30;
        CHECK(check_loop_project(views.data(), nviews, f, 3, l2, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        l2 = L; l2.list = nullptr;
        CHECK(check_loop_project(views.data(), nviews, f, 3, l2, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        l2 = L; l2.nlist = nullptr;
        CHECK(check_loop_project(views.data(), nviews, f, 3, l2, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        l2 = L; l2.skip = nullptr;
        CHECK(check_loop_project(views.data(), nviews, f, 3, l2, nullptr, Q, nq, ov, qcap) == ORBX_OK);
        l2 = L; l2.list = off1(list.data());
        CHECK(check_loop_project(views.data(), nviews, f, 3, l2, nullptr, Q, nq, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, off1(rec.data()), Q, nq, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, Q, nullptr, ov, qcap) == ORBX_ERR_ARG);
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, Q, nq, nullptr, qcap) == ORBX_ERR_ARG);
        Queries q2 = Q;
        q2.qxyr = nullptr;
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, q2, nq, ov, qcap) == ORBX_ERR_ARG);
        q2 = Q; q2.qlev = nullptr;
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, q2, nq, ov, qcap) == ORBX_ERR_ARG);
        q2 = Q; q2.qpos = nullptr;
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, q2, nq, ov, qcap) == ORBX_ERR_ARG);
        q2 = Q; q2.qdesc = nullptr;
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, q2, nq, ov, qcap) == ORBX_ERR_ARG);
        q2 = Q; q2.qdesc = qdesc + 8;                                                                          // the descriptors are written in 16-byte pieces
        CHECK(check_loop_project(views.data(), nviews, f, 3, L, nullptr, q2, nq, ov, qcap) == ORBX_ERR_ARG);
    }
    {
        // orbp_loop_search_batch_device
        const FuseFrames K{kps.data(), desc, cell_off.data(), cell_feat.data(), nt.data(), nframes, cap, frame.data()};
        const LoopOut O{rec.data(), ints.data(), ints.data(), ints.data(), ints.data(), ints.data()};
        auto chk = [&](const Lists& l, const FuseFrames& k, const LoopOut& o, int nv = 3, int nl = 3, int dist = 50, int qc = 16, const orbf_bounds* bb = nullptr) {
            return check_loop_search(views.data(), nv, f, nl, l, bb ? bb : &b, dist, k, qc, o);
        };
        CHECK(chk(L, K, O) == ORBX_OK);
        CHECK(check_loop_search(nullptr, 0, f, 3, Lists{nullptr, nullptr, 1, nullptr}, &b, 50, FuseFrames{nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr}, 1,
                                LoopOut{}) == ORBX_OK);
        CHECK(check_loop_search(nullptr, nviews, f, 3, L, &b, 50, K, qcap, O) == ORBX_ERR_ARG);
        CHECK(check_loop_search(views.data(), nviews, nullptr, 3, L, &b, 50, K, qcap, O) == ORBX_ERR_ARG);
        CHECK(check_loop_search(views.data(), nviews, f, 3, L, nullptr, 50, K, qcap, O) == ORBX_ERR_ARG);
        CHECK(chk(L, K, O, -1) == ORBX_ERR_ARG && chk(L, K, O, ORBP_MAX_VIEWS + 1) == ORBX_ERR_ARG);
        CHECK(chk(L, K, O, nviews, 0) == ORBX_ERR_ARG && chk(L, K, O, nviews, 1) == ORBX_OK && chk(L, K, O, nviews, ORBS_MAX_LEVELS + 1) == ORBX_ERR_ARG);
        CHECK(chk(L, K, O, nviews, 3, -1) == ORBX_ERR_ARG && chk(L, K, O, nviews, 3, 0) == ORBX_OK && chk(L, K, O, nviews, 3, 256) == ORBX_OK &&
              chk(L, K, O, nviews, 3, 257) == ORBX_ERR_ARG);
        CHECK(chk(L, K, O, nviews, 3, 50, 0) == ORBX_ERR_ARG && chk(L, K, O, nviews, 3, 50, ORBF_MAX_FEATURES) == ORBX_OK &&
              chk(L, K, O, nviews, 3, 50, ORBF_MAX_FEATURES + 1) == ORBX_ERR_ARG);
        Lists l2 = L;
        l2.lcap = 0;
        CHECK(chk(l2, K, O) == ORBX_ERR_ARG);
        l2 = L; l2.lcap = 1 << 30;
        CHECK(chk(l2, K, O) == ORBX_ERR_ARG);
        l2 = L; l2.list = nullptr;
        CHECK(chk(l2, K, O) == ORBX_ERR_ARG);
        l2 = L; l2.nlist = nullptr;
        CHECK(chk(l2, K, O) == ORBX_ERR_ARG);
        l2 = L; l2.skip = nullptr;
        CHECK(chk(l2, K, O) == ORBX_OK);
        l2 = L; l2.nlist = off1(nlist.data());
        CHECK(chk(l2, K, O) == ORBX_ERR_ARG);
        FuseFrames k2 = K;
        k2.cap = 0;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2.cap = ORBF_MAX_FEATURES + 1;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.nframes = 0;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.nframes = 1 << 18; k2.cap = ORBF_MAX_FEATURES;                                               // nframes * cap = 2^31
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.kps_un = nullptr;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.desc = nullptr;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.desc = desc + 4;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.cell_off = nullptr;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.cell_feat = nullptr;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.cell_feat = off1(cell_feat.data());
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.nt = nullptr;
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        k2 = K; k2.frame = nullptr;                                                                            // view p searches row p; a row out of range is reported per view
        CHECK(chk(L, k2, O) == ORBX_OK);
        k2 = K; k2.frame = off1(frame.data());
        CHECK(chk(L, k2, O) == ORBX_ERR_ARG);
        LoopOut o2 = O;
        o2.rec = nullptr;
        CHECK(chk(L, K, o2) == ORBX_OK);
        o2 = O; o2.t2slot = nullptr;
        CHECK(chk(L, K, o2) == ORBX_OK);
        o2 = O; o2.t2pos = nullptr;
        CHECK(chk(L, K, o2) == ORBX_ERR_ARG);
        o2 = O; o2.nmatches = nullptr;
        CHECK(chk(L, K, o2) == ORBX_ERR_ARG);
        o2 = O; o2.nq = nullptr;
        CHECK(chk(L, K, o2) == ORBX_ERR_ARG);
        o2 = O; o2.overflow = nullptr;
        CHECK(chk(L, K, o2) == ORBX_ERR_ARG);
        o2 = O; o2.rec = off1(rec.data());
        CHECK(chk(L, K, o2) == ORBX_ERR_ARG);
        o2 = O; o2.t2slot = off1(ints.data());
        CHECK(chk(L, K, o2) == ORBX_ERR_ARG);
    }
    {
        // orbp_loop_search
        orbp_view v{};
        v.mode = ORBP_MODE_LOOP;
        const Frame F{kps.data(), desc, cell_off.data(), cell_feat.data(), nullptr, cap, nullptr};
        int nm = 0;
        int32_t* t2pos = ints.data();
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_OK);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, F, cap, true, qcap, t2pos, &nm) == ORBX_OK);
        CHECK(check_loop_one(&v, f, 3, nullptr, 0, &b, 50, Frame{nullptr, nullptr, cell_off.data(), nullptr, nullptr, 1, nullptr}, 0, false, qcap, nullptr, &nm) == ORBX_OK);
        CHECK(check_loop_one(nullptr, f, 3, list.data(), lcap, &b, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, nullptr, 3, list.data(), lcap, &b, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 0, list.data(), lcap, &b, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, ORBS_MAX_LEVELS + 1, list.data(), lcap, &b, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, nullptr, lcap, &b, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), -1, &b, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, nullptr, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, -1, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 257, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, F, -1, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, F, ORBF_MAX_FEATURES + 1, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, F, cap, false, 0, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, F, cap, false, ORBF_MAX_FEATURES + 1, t2pos, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, F, cap, false, qcap, nullptr, &nm) == ORBX_ERR_ARG);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, F, cap, false, qcap, t2pos, nullptr) == ORBX_ERR_ARG);
        for (int mode : {ORBP_MODE_FRAME, ORBP_MODE_LAST_FRAME, ORBP_MODE_KEYFRAME, ORBP_MODE_FUSE, 5, -1}) {
            orbp_view w = v;
            w.mode = mode;
            CHECK(check_loop_one(&w, f, 3, list.data(), lcap, &b, 50, F, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        }
        Frame f2 = F;
        f2.kps_un = nullptr;
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, f2, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        f2 = F; f2.desc = nullptr;
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, f2, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        f2 = F; f2.cell_off = nullptr;
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, f2, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        f2 = F; f2.cell_feat = nullptr;
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, f2, cap, false, qcap, t2pos, &nm) == ORBX_ERR_ARG);
        f2 = F; f2.desc = desc + 4;                                                                            // a host array is copied into an aligned slot, a resident row is read in place
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, f2, cap, false, qcap, t2pos, &nm) == ORBX_OK);
        CHECK(check_loop_one(&v, f, 3, list.data(), lcap, &b, 50, f2, cap, true, qcap, t2pos, &nm) == ORBX_ERR_ARG);
    }
    {
        // the block with everything in it: slots at multiples of 256, one span up, the results down, the rest behind them
        const LoopBlock B(7, 600, 16, {true, true, true, true, true});
        CHECK(sizeof(orbp_view) == 108 && sizeof(orbp_fused) == 16 && sizeof(orbx_keypoint) == 28 && loop_tiles(600) == 3 && loop_tiles(256) == 1 && loop_tiles(257) == 2);
        CHECK(B.view.off == 0 && B.counts.off == 256 && B.list.off == 512 && B.skip.off == 512 + 2560);
        CHECK(B.frame.kps.off == 3072 + 768 && B.frame.desc.off == 4096 && B.frame.cell_off.off == 4352);
        const size_t off_bytes = ((size_t)(ORBF_GRID_CELLS + 1) * 4 + 255) & ~(size_t)255;
        CHECK(B.frame.cell_feat.off == 4352 + off_bytes && B.frame.claimed.off == 4608 + off_bytes && B.L.upload() == 4608 + off_bytes + 256);
        const size_t up = B.L.upload();
        CHECK(B.result.off == up && B.t2pos.off == up + 256 && B.t2slot.off == up + 512 && B.rec.off == up + 768 && B.L.download() == 768 + 9728);
        const size_t tail = up + B.L.download();
        CHECK(B.dev.q.qxyr.off == tail && !B.dev.q.qangle.present && B.dev.tile_count.off > B.dev.q.t2q.off && !B.dev.rec.present && !B.dev.g_kps.present);
        CHECK(B.L.total() == B.dev.tile_count.off + 256);
        // what the caller does not pass takes no room; records nobody asked for move behind the download span
        const LoopBlock C(7, 600, 16, {false, false, false, false, false});
        CHECK(!C.skip.present && !C.frame.claimed.present && !C.frame.kps.present && !C.frame.desc.present && !C.frame.cell_off.present && !C.frame.cell_feat.present);
        CHECK(C.L.upload() == 512 + 2560 && !C.t2slot.present && !C.rec.present && C.L.download() == 512 && C.dev.rec.present && C.dev.rec.off >= C.L.upload() + 512);
        CHECK(C.L.total() == C.dev.rec.off + 9728);
        // the flags of a resident key frame are a host array all the same: they go up without the frame
        const LoopBlock D(7, 600, 16, {false, true, false, false, false});
        CHECK(D.frame.claimed.present && !D.frame.kps.present && D.frame.claimed.off == 512 + 2560 && D.L.upload() == 3072 + 256);
        CHECK(same_sizes(7, 600, 16, {true, true, true, true, true}, 17408, 10496, 30208) == 0 && same_sizes(7, 600, 16, {false, false, false, false, false}, 3072, 512, 15616) == 0);
        CHECK(same_sizes(300, 600, 640, {true, true, true, true, true}, 36352, 12544, 89088) == 0 && same_sizes(1, 1, 1, {false, false, false, false, false}, 768, 512, 3584) == 0);
        CHECK(same_sizes(1, 1, 1, {false, true, true, true, true}, 14336, 1024, 17408) == 0 && same_sizes(2000, 8000, 8000, {true, true, true, true, true}, 183552, 144640, 816896) == 0);
        CHECK(same_sizes(2000, 8000, 8192, {true, true, false, false, false}, 42752, 8448, 679424) == 0);
        // the batch forms' scratch: the projection alone has no query arrays of its own; gathered rows only when asked for
        Layout P;
        LoopSlots S;
        S.reserve(P, 3, 600, 1, 16, false, true, false);
        CHECK(!S.q.qxyr.present && S.tile_count.off == 0 && S.rec.off == 256 && P.total() == 256 + (((size_t)3 * 600 * 16 + 255) & ~(size_t)255) && !S.g_kps.present);
        Layout G;
        LoopSlots T;
        T.reserve(G, 3, 600, 7, 16, true, false, true);
        CHECK(T.q.qxyr.present && !T.rec.present && T.g_kps.present && T.g_desc.off % 256 == 0 && T.g_nt.present && G.total() == T.g_nt.off + 256);
    }
    {
        // the one-view call through the handle's block: exact spans, sentinels around them, and the chain waited for before a grow
        Handle m;
        CHECK(m.own.ensure() == hipSuccess && m.chain.ev.ensure() == hipSuccess);
        std::string at_fill, log;
        CHECK(one_view_call(m, 300, 600, 640, true, true, true, true, true, at_fill, log) == 0);
        CHECK(at_fill == "mm" && log == "mmudry");                    // the first call: nothing on the handle to wait for
        const size_t h0 = m.block.h.size(), d0 = m.block.d.size();
        CHECK(one_view_call(m, 300, 600, 640, true, true, true, true, true, at_fill, log) == 0);
        CHECK(at_fill.empty() && log == "sudry" && m.block.h.size() == h0 && m.block.d.size() == d0);           // the steady state
        CHECK(one_view_call(m, 1, 1, 1, false, false, false, false, false, at_fill, log) == 0 && at_fill.empty() && m.block.d.size() == d0);
        CHECK(one_view_call(m, 0, 0, 1, false, true, true, true, true, at_fill, log) == 0 && at_fill.empty());    // an empty key frame and an empty list
        CHECK(one_view_call(m, 2000, 8000, 8000, true, true, true, true, true, at_fill, log) == 0);
        CHECK(at_fill.substr(0, 1) == "w" && at_fill.find('m') != std::string::npos && m.block.h.size() > h0 && m.block.d.size() > d0);   // waits, then frees and allocates
        const size_t d1 = m.block.d.size();
        CHECK(one_view_call(m, 2000, 8000, 8192, true, true, false, false, false, at_fill, log) == 0 && m.block.d.size() >= d1);
        CHECK(one_view_call(m, 300, 600, 640, true, true, true, true, true, at_fill, log) == 0 && at_fill.empty() && log == "sudry");
    }
    CHECK(hip_stub_live == 0);
    std::printf("loop host ok\n");
    return 0;
}
