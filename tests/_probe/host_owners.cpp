// orb_slam_amd/csrc/orbx_host.h and orbp_host.h on the CPU against tests/_probe/hip_stub: the staging layout, the layouts of the block
// a map-point table keeps, the device scope and the event chain, what the owners hold after a failed allocation, and the scope of a call
// on a handle (orbx::Call) with the path of a synchronous host form through the handle's block (orbx::Staged), in the order of their HIP calls
// (tests/test_host_owners.py builds this under AddressSanitizer, which also reports leaks and double frees).
#include <cstdio>
#include <mutex>
#include <string>

#include "orbp_host.h"
#include "orbx_host.h"

using namespace orbx;

// upload span, download span and total of orbp_track's / orbp_track_source's block (orbp::OneView plus the source slots and the queries)
// against the sizes of the block before the one-view forms shared a layout, which are those of the hand-laid block before that; one line
// of the table per flag combination: before -> now
static bool spans(const orbp::TrackBlock& B, size_t up, size_t down, size_t total) {
    std::printf("track block: upload %zu -> %zu, download %zu -> %zu, total %zu -> %zu\n", up, B.L.upload(), down, B.L.download(), total, B.L.total());
    const Layout::Slot<int32_t> i32[] = {B.counts, B.list, B.result, B.t2pos, B.t2slot, B.frame.cell_off, B.frame.cell_feat, B.q.qlev, B.q.t2q};
    for (const auto& s : i32)
        if (s.off % 256) return false;
    return B.view.off == 0 && B.counts.off == 256 && B.result.off == up && B.frame.kps.off % 256 == 0 && B.rec.off % 256 == 0 &&
           B.q.qxyr.off == up + down && B.q.qangle.off % 256 == 0 && B.L.upload() == up && B.L.download() == down && B.L.total() == total;
}

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
}  // namespace

static bool all(const uint8_t* p, size_t n, uint8_t v) {
    for (size_t i = 0; i < n; i++)
        if (p[i] != v) return false;
    return true;
}

// One synchronous host form over `m`'s block as orbp_project.hip writes them: fit, fill the upload span, run a body that stands in for the
// kernels (it answers 0x22 into the download span and returns body_rc).  Around it every byte of both halves that no copy may touch holds a
// sentinel.  Returns 1 on a failed check; rc: the call's status; at_fill: the HIP calls up to the first write into the pinned block.
static int staged_call(Handle& m, const Layout& L, int body_rc, int& rc, std::string& at_fill) {
    const size_t up = L.upload(), down = L.download(), total = L.total();
    hip_stub_log.clear();
    hip_stub_up = hip_stub_down = {};
    at_fill = "-";
    Call<Handle> c(&m, nullptr);
    CHECK(c.st == (hipStream_t)m.own && hip_stub_device == m.device);
    Staged<Handle> s(c, m.block, L);
    if ((rc = s.fit()) != ORBX_OK) return 0;
    at_fill = hip_stub_log;
    CHECK(s.h == m.block.h.as() && s.d == m.block.d.as() && m.block.fits(up + down, total) && !m.block.busy);
    const size_t hsize = m.block.h.size(), dsize = m.block.d.size();
    std::memset(s.h, 0x11, up);
    std::memset(s.h + up, 0xA5, hsize - up);                          // the download span and the pinned bytes beyond it
    std::memset(s.d, 0x33, dsize);                                    // the device-only tail among them
    bool body_ok = false;
    rc = s.run([&] {
        body_ok = hip_stub_log.back() == 'u' && all(s.d, up, 0x11) && all(s.d + up, dsize - up, 0x33);      // the upload is [0, up) and is in front
        std::memset(s.d + up, 0x22, down);
        return body_rc;
    });
    CHECK(body_ok && hip_stub_up.dst == s.d && hip_stub_up.src == s.h && hip_stub_up.bytes == up);
    CHECK(all(s.h, up, 0x11) && all(s.h + up + down, hsize - up - down, 0xA5) && all(s.d + up + down, dsize - up - down, 0x33));
    if (rc != ORBX_OK) return 0;
    if (down) CHECK(hip_stub_down.dst == s.h + up && hip_stub_down.src == s.d + up && hip_stub_down.bytes == down && all(s.h + up, down, 0x22));
    else CHECK(hip_stub_down.bytes == 0 && hip_stub_log.find('d') == std::string::npos);
    return 0;
}

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
    {
        // Call: the handle's device for the scope, the chain recorded once on every way out after begin(), the mutex free afterwards
        Handle m;
        CHECK(m.own.ensure() == hipSuccess && m.chain.ev.ensure() == hipSuccess);
        hipStream_t other = nullptr;
        CHECK(hipStreamCreateWithFlags(&other, hipStreamNonBlocking) == hipSuccess);
        hip_stub_device = 1;
        hip_stub_log.clear();
        {
            Call<Handle> c(&m, other);                                 // the caller's stream; left without begin(): nothing recorded
            CHECK(c.ok() && c.st == other && hip_stub_device == 0);
        }
        CHECK(hip_stub_device == 1 && hip_stub_log.empty() && !m.chain.chained && m.mu.try_lock());
        m.mu.unlock();
        {
            Call<Handle> c(&m, nullptr);                               // left early after begin()
            CHECK(c.begin() == ORBX_OK && hip_stub_log.empty());       // nothing to wait for yet
        }
        CHECK(hip_stub_log == "r" && m.chain.chained && hip_stub_device == 1 && m.mu.try_lock());
        m.mu.unlock();
        {
            Call<Handle> c(&m, nullptr);
            CHECK(c.begin() == ORBX_OK && c.end() == ORBX_OK && hip_stub_log == "rsr");
        }
        CHECK(hip_stub_log == "rsr");                                   // end() recorded it: leaving does not record again
        CHECK(hip_stub_device == 1);
        // a device that cannot be selected: reported by begin() and by fit(), nothing enqueued, recorded or allocated
        m.device = 7;
        hip_stub_log.clear();
        {
            Call<Handle> c(&m, nullptr);
            Layout L;
            L.add<uint8_t>(100);
            L.end_upload();
            Staged<Handle> s(c, m.block, L);
            CHECK(!c.ok() && c.begin() == ORBX_ERR_DEVICE && s.fit() == ORBX_ERR_DEVICE && s.run([] { return (int)ORBX_OK; }) == ORBX_ERR_DEVICE);
        }
        CHECK(hip_stub_log.empty() && hip_stub_device == 1 && !m.block.h && !m.block.d && m.mu.try_lock());
        m.mu.unlock();
        CHECK(hipStreamDestroy(other) == hipSuccess);
    }
    CHECK(hip_stub_live == 0);
    {
        // Staged: one block for every form of a handle
        Handle m;
        CHECK(m.own.ensure() == hipSuccess && m.chain.ev.ensure() == hipSuccess);
        const int live0 = hip_stub_live;
        int rc = 0;
        std::string at_fill;
        Layout L;                                                       // 512 up, 256 down, 1024 behind them on the device only
        L.add<uint8_t>(300); L.end_upload(); L.add<int32_t>(3); L.end_download(); L.add<uint8_t>(1000);
        CHECK(L.upload() == 512 && L.download() == 256 && L.total() == 1792);
        // the first call grows the empty block (nothing to wait for: no work on the handle yet), both halves to 4096
        CHECK(staged_call(m, L, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK);
        CHECK(at_fill == "mm" && hip_stub_log == "mmudry" && m.block.h.size() == 4096 && m.block.d.size() == 4096 && hip_stub_live == live0 + 2);
        // the steady state: nothing allocated, no wait on the host; the stream waits for the chain
        const void *h0 = m.block.h, *d0 = m.block.d;
        CHECK(staged_call(m, L, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK);
        CHECK(at_fill.empty() && hip_stub_log == "sudry" && (void*)m.block.h == h0 && (void*)m.block.d == d0 && !m.block.busy);
        // an empty download span issues no copy (orbp_put)
        Layout U;
        U.add<float>(257); U.end_upload();
        CHECK(U.download() == 0 && staged_call(m, U, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK && at_fill.empty() && hip_stub_log == "sury");
        // a device-only tail grows the device half alone, a larger upload both: the host waits for the chain before anything is freed, and
        // the pinned half is sized to the two spans, the device half to the whole layout
        Layout T;
        T.add<uint8_t>(300); T.end_upload(); T.add<int32_t>(3); T.end_download(); T.add<uint8_t>(10000);
        CHECK(staged_call(m, T, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK && at_fill == "wfm" && m.block.h.size() == 4096 && m.block.d.size() == 16384);
        Layout G;
        G.add<uint8_t>(5000); G.end_upload(); G.add<int32_t>(3); G.end_download(); G.add<uint8_t>(20000);
        CHECK(staged_call(m, G, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK && at_fill == "wfmfm" && m.block.h.size() == 8192 && m.block.d.size() == 32768);
        CHECK(hip_stub_live == live0 + 2);
        // a small call after the large ones runs in the block as it is
        CHECK(staged_call(m, L, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK && at_fill.empty() && m.block.h.size() == 8192 && m.block.d.size() == 32768);
        // a failed grow (the pinned half grows, the device half fails) leaves both halves empty; the next call grows again
        Layout H;
        H.add<uint8_t>(9000); H.end_upload(); H.add<int32_t>(3); H.end_download(); H.add<uint8_t>(40000);
        hip_stub_fail = 2;
        m.err.clear();
        CHECK(staged_call(m, H, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_ERR_DEVICE && !m.err.empty() && at_fill == "-");
        CHECK(!m.block.h && !m.block.d && m.block.h.size() == 0 && m.block.d.size() == 0 && hip_stub_live == live0 && hip_stub_log == "wfmff");     // waited, then: pinned freed and made, device freed, its allocation fails, pinned freed
        CHECK(staged_call(m, H, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK && at_fill == "wmm" && m.block.h.size() == 16384 && m.block.d.size() == 65536);
        // a body that fails after the upload: the chain is recorded once, nothing comes down, nothing is waited for; the next call waits
        // for the chain on the host before its first write into the pinned block, the call after that does not
        CHECK(staged_call(m, L, ORBX_ERR_ARG, rc, at_fill) == 0 && rc == ORBX_ERR_ARG && at_fill.empty() && hip_stub_log == "sur" && m.block.busy);
        CHECK(staged_call(m, L, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK && at_fill == "w" && hip_stub_log == "wsudry" && !m.block.busy);
        CHECK(staged_call(m, L, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK && at_fill.empty() && hip_stub_log == "sudry");
        // ... and so does a call that has to grow after a failed one: one wait serves both
        CHECK(staged_call(m, L, ORBX_ERR_CAPACITY, rc, at_fill) == 0 && rc == ORBX_ERR_CAPACITY && m.block.busy);
        Layout I;
        I.add<uint8_t>(20000); I.end_upload();
        CHECK(staged_call(m, I, ORBX_OK, rc, at_fill) == 0 && rc == ORBX_OK && at_fill == "wfm" && m.block.h.size() == 32768 && m.block.d.size() == 65536);
    }
    CHECK(hip_stub_live == 0);
    std::printf("host owners ok\n");
    return 0;
}
