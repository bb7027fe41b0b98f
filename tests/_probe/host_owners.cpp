// orb_slam_amd/csrc/orbx_host.h and orbp_host.h on the CPU against tests/_probe/hip_stub: the staging layout, the layouts of the blocks
// a map-point table keeps, the device scope and the event chain, and what the owners hold after a failed allocation
// (tests/test_host_owners.py builds this under AddressSanitizer, which also reports leaks and double frees).
#include <cstdio>

#include "orbp_host.h"
#include "orbx_host.h"

using namespace orbx;

// upload span, download span and total of orbp_track's / orbp_track_source's block against the sizes of the hand-laid block it replaces
static bool spans(const orbp::TrackBlock& B, size_t up, size_t down, size_t total) {
    const Layout::Slot<int32_t> i32[] = {B.counts, B.list, B.result, B.t2pos, B.t2slot, B.frame.cell_off, B.frame.cell_feat, B.q.qlev, B.q.t2q};
    for (const auto& s : i32)
        if (s.off % 256) return false;
    return B.view.off == 0 && B.counts.off == 256 && B.result.off == up && B.frame.kps.off % 256 == 0 && B.rec.off % 256 == 0 &&
           B.q.qxyr.off == up + down && B.q.qangle.off % 256 == 0 && B.L.upload() == up && B.L.download() == down && B.L.total() == total;
}

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    {
        // layout: every array at a multiple of 256 bytes, at least one element reserved, inputs uploaded by alloc(), outputs read by get()
        const uint8_t q[100] = {1, 2, 3};
        const double w[3] = {0.5, 1.5, 2.5};
        Staging s;
        const auto a = s.in(q, 100);
        const auto b = s.out<int32_t>(0);
        const auto c = s.in(w, 3);
        const auto d = s.out<int32_t>(65);
        CHECK(a.off == 0 && b.off == 256 && c.off == 512 && d.off == 768);
        CHECK(s.alloc() == hipSuccess && s.buf.size() == 1280);
        CHECK(s[a][2] == 3 && s[c][2] == 2.5 && (uint8_t*)s[d] == s.buf.as() + 768);
        double back[3] = {};
        CHECK(s.get(back, c, 3) == hipSuccess && back[1] == 1.5);
        DevBuf kept = std::move(s.buf);              // a longer-lived owner takes the block
        CHECK(kept.size() == 1280 && s.buf.size() == 0 && !s.buf);
    }
    CHECK(hip_stub_live == 0);
    {
        // a failed grow leaves an empty buffer of size 0, never the old size over a freed or null pointer
        DevBuf d;
        CHECK(d.ensure(100) == hipSuccess && d.size() == 100 && d);
        void* p = d;
        CHECK(d.ensure(60) == hipSuccess && (void*)d == p);
        hip_stub_fail = 1;
        CHECK(d.ensure(200) != hipSuccess && d.size() == 0 && !d);
        CHECK(d.ensure(60) == hipSuccess && d.size() == 60);
        // pinned + mapped: a failed mapping frees the allocation
        PinnedBuf h;
        hip_stub_fail = 2;
        CHECK(h.ensure(64, hipHostMallocMapped) != hipSuccess && h.size() == 0 && !h && !h.mapped());
        CHECK(hip_stub_live == 1);
        CHECK(h.ensure(64, hipHostMallocMapped) == hipSuccess && h.mapped() == h.as());
        // streams and events are created once; a failed creation holds nothing and is retried
        Stream st;
        Event ev[3];
        hip_stub_fail = 1;
        CHECK(st.ensure() != hipSuccess && !st);
        CHECK(st.ensure() == hipSuccess && st);
        hipStream_t s0 = st;
        CHECK(st.ensure() == hipSuccess && (hipStream_t)st == s0);
        hip_stub_fail = 2;
        bool ok = true;
        for (Event& e : ev) ok = ok && e.ensure() == hipSuccess;
        CHECK(!ok && ev[0] && !ev[1] && !ev[2]);
        CHECK(hip_stub_live == 4);
    }
    CHECK(hip_stub_live == 0);                          // every owner released what it held, once
    {
        // Layout: slots at multiples of 256 bytes, an absent slot takes no room and resolves to null, the two spans
        Layout L;
        const auto a = L.add<float>(3);
        const auto b = L.add<double>(100, false);
        const auto c = L.add<uint8_t>(257);
        const auto e = L.add<int32_t>(0);
        L.end_upload();
        const auto r = L.add<int32_t>(3);
        L.end_download();
        const auto w = L.add<uint8_t>(1000);
        CHECK(a.off == 0 && b.off == 256 && !b.present && c.off == 256 && e.off == 768 && r.off == 1024 && w.off == 1280);
        CHECK(L.upload() == 1024 && L.download() == 256 && L.total() == 2304);
        uint8_t base[1];
        CHECK(Layout::at(base, b) == nullptr && (uint8_t*)Layout::at(base, a) == base);
        // the query scratch of the batch calls: (nviews, cap, qcap), without and with the angles
        Layout s0, s1;
        orbp::QuerySlots q0, q1;
        q0.reserve(s0, 1, 1000, 512, false);
        q1.reserve(s1, 8, 1000, 700, true);
        CHECK(s0.total() == 35072 && !q0.qangle.present && q0.at(base).qangle == nullptr);
        CHECK(s1.total() == 391168 && q1.qangle.present && q1.qangle.off == 391168 - 22528);
        // orbp_track(nt, nlist, qcap): flags {source, list, skip, src_kps, src_desc, frame, claimed, t2slot, rec}
        CHECK(spans(orbp::TrackBlock(1000, 600, 512, {false, true, false, false, false, true, false, true, false}), 79872, 4352, 119296));
        CHECK(spans(orbp::TrackBlock(1000, 600, 512, {false, false, true, false, false, true, true, true, true}), 79104, 16384, 130560));
        CHECK(spans(orbp::TrackBlock(300, 257, 100, {false, true, true, false, false, false, true, true, true}), 2304, 6912, 17408));
        CHECK(spans(orbp::TrackBlock(1, 1, 64, {false, true, false, false, false, true, false, true, false}), 14080, 512, 18944));
        // orbp_track_source: a last-frame source from the host, a key-frame source from the host, both frames on the device, an empty list
        CHECK(spans(orbp::TrackBlock(1000, 700, 512, {true, true, true, true, true, true, true, true, false}), 124160, 8448, 169728));
        CHECK(spans(orbp::TrackBlock(300, 257, 100, {true, true, false, true, false, false, false, false, false}), 9216, 1536, 19456));
        CHECK(spans(orbp::TrackBlock(300, 257, 100, {true, true, false, false, false, false, false, true, false}), 1792, 2816, 13312));
        CHECK(spans(orbp::TrackBlock(5, 1, 64, {true, true, false, false, false, true, false, false, false}), 14080, 512, 19200));
        const orbp::TrackBlock dev(300, 257, 100, {false, true, true, false, false, false, true, true, true});
        CHECK(!dev.frame.kps.present && !dev.frame.claimed.present && !dev.t2pos.present && dev.rec.present);
        // a frame on the device is passed through with the count's device address; a host frame is copied and named inside the block
        const orbp::Frame f{nullptr, nullptr, nullptr, nullptr, nullptr, 300, base};
        const int32_t nt = 0;
        const orbp::Frame g = dev.frame.stage(nullptr, nullptr, f, 0, &nt);
        CHECK(g.claimed == base && g.nt == &nt && g.cap == 300);
    }
    {
        // a pinned block and its device twin: a failed grow of either leaves both empty
        Block b;
        CHECK(!b.fits(1, 1) && b.ensure(100, 300) == hipSuccess && b.fits(100, 300) && !b.fits(101, 300) && !b.fits(100, 301));
        hip_stub_fail = 2;                              // the pinned half grows, the device half fails
        CHECK(b.ensure(200, 600) != hipSuccess && b.h.size() == 0 && b.d.size() == 0 && !b.h && !b.d && !b.fits(1, 1));
        CHECK(hip_stub_live == 0);
        CHECK(b.ensure(200, 600) == hipSuccess && b.fits(200, 600));
    }
    {
        // DeviceScope restores the previous device, also when the wanted one cannot be selected
        hip_stub_device = 1;
        {
            DeviceScope ds(0);
            CHECK(ds.ok && hip_stub_device == 0);
        }
        CHECK(hip_stub_device == 1);
        {
            DeviceScope ds(7);
            CHECK(!ds.ok);
        }
        CHECK(hip_stub_device == 1);
        // Chain: begin and wait before any end are no-ops; a link left early records the chain
        Chain c;
        CHECK(c.ev.ensure() == hipSuccess);
        CHECK(c.begin(nullptr) == hipSuccess && c.wait() == hipSuccess && hip_stub_waits == 0 && !c.chained);
        {
            Chain::Link link(c, nullptr);
        }
        CHECK(c.chained && c.begin(nullptr) == hipSuccess && hip_stub_waits == 1 && c.wait() == hipSuccess && hip_stub_waits == 2);
        Chain c2;
        CHECK(c2.ev.ensure() == hipSuccess);
        {
            Chain::Link link(c2, nullptr);
            CHECK(link.end() == hipSuccess && c2.chained);
        }
    }
    CHECK(hip_stub_live == 0);
    std::printf("host owners ok\n");
    return 0;
}
