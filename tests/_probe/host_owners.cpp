// orb_slam_amd/csrc/orbx_host.h on the CPU against tests/_probe/hip_stub: the staging layout, and what the owners hold after a failed
// allocation (tests/test_host_owners.py builds this under AddressSanitizer, which also reports leaks and double frees).
#include <cstdio>

#include "orbx_host.h"

using namespace orbx;

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
    std::printf("host owners ok\n");
    return 0;
}
