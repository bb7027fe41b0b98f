// The host side of orbp_cull* on the CPU against tests/_probe/hip_stub: the argument checks that need no handle (orbp::check_cull), the layout of
// the host form's block (orbp::CullBlock) and its path through orbx::Staged: the upload and download spans are exact, with sentinels around them,
// columns the caller keeps on the device are passed through, and unpack copies ncand words of each output and no more (tests/test_cull_host.py
// builds this under AddressSanitizer + UndefinedBehaviorSanitizer).
#include <cstdio>
#include <cstdlib>
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

// One orbp_cull over `m`'s block as orbp_project.hip writes it, the body standing in for the kernels: it checks what went up and answers into
// the download span.
int cull_call(Handle& m, int ncand, int nkf, int cap, bool kf_host, std::string& log) {
    std::vector<int32_t> cand(ncand, 3), kf_slot((size_t)nkf * cap, 5), kf_nt(nkf, cap), nmps(ncand + 1, -5), nred(ncand + 1, -6), cull(ncand + 1, -7);
    std::vector<uint8_t> kf_oct((size_t)nkf * cap + 1, 7);
    const CullList C{cand.data(), ncand};
    const CullColumns K{{kf_slot.data(), kf_nt.data(), nkf, cap}, kf_oct.data() + 1, 8};              // the octaves at an odd address
    const CullOut O{nmps.data(), nred.data(), cull.data()};
    CHECK(check_cull(C, K, O, false, !kf_host) == ORBX_OK);
    hip_stub_log.clear();
    hip_stub_up = hip_stub_down = {};
    Call<Handle> c(&m, nullptr);
    const CullBlock B(C, K, kf_host);
    const size_t up = B.L.upload(), down = B.L.download(), total = B.L.total();
    CHECK(total == up + down && down >= (size_t)ncand * 12);          // nothing device-only: the scratch is the handle's
    CHECK(B.kf_slot.present == kf_host && B.kf_oct.present == kf_host && B.kf_nt.present == kf_host && B.cand.present);
    Staged<Handle> s(c, m.block, B.L);
    CHECK(s.fit() == ORBX_OK);
    const size_t hsize = m.block.h.size(), dsize = m.block.d.size();
    CHECK(hsize >= up + down && dsize >= total);
    std::memset(s.h, 0x11, up);
    std::memset(s.h + up, 0xA5, hsize - up);
    std::memset(s.d, 0x33, dsize);
    CullList dc;
    CullColumns dk;
    CullOut dout;
    B.stage(s.h, s.d, C, K, dc, dk, dout);
    bool body_ok = false;
    const int rc = s.run([&] {
        const uint8_t* d = s.d;
        auto inside = [&](const void* p) { return (const uint8_t*)p >= d && (const uint8_t*)p < d + up; };
        body_ok = hip_stub_log.back() == 'u' && all(s.d + up, dsize - up, 0x33);
        body_ok = body_ok && inside(dc.cand) && dc.ncand == ncand && dc.cand[ncand - 1] == 3;
        if (kf_host) body_ok = body_ok && inside(dk.K.slot) && inside(dk.oct) && inside(dk.K.nt) && dk.K.slot[(size_t)nkf * cap - 1] == 5 && dk.oct[(size_t)nkf * cap - 1] == 7 && dk.K.nt[nkf - 1] == cap;
        else body_ok = body_ok && dk.K.slot == kf_slot.data() && dk.oct == kf_oct.data() + 1 && dk.K.nt == kf_nt.data();
        body_ok = body_ok && dk.K.nkf == nkf && dk.K.cap == cap && dk.nlevels == 8;
        body_ok = body_ok && (uint8_t*)dout.nmps == s.d + up && (uint8_t*)(dout.cull + ncand) <= s.d + up + down;
        for (int i = 0; i < ncand; i++) { dout.nmps[i] = 100 + i; dout.nred[i] = 50 + i; dout.cull[i] = i & 1; }
        return (int)ORBX_OK;
    });
    log = hip_stub_log;
    CHECK(rc == ORBX_OK && body_ok);
    CHECK(hip_stub_up.dst == s.d && hip_stub_up.src == s.h && hip_stub_up.bytes == up);
    CHECK(hip_stub_down.dst == s.h + up && hip_stub_down.src == s.d + up && hip_stub_down.bytes == down);
    CHECK(all(s.h + up + down, hsize - up - down, 0xA5) && all(s.d + up + down, dsize - up - down, 0x33));
    B.unpack(s.h, O);
    for (int i = 0; i < ncand; i++) CHECK(nmps[i] == 100 + i && nred[i] == 50 + i && cull[i] == (i & 1));
    CHECK(nmps[ncand] == -5 && nred[ncand] == -6 && cull[ncand] == -7);
    return 0;
}
}  // namespace

int main() {
    const int ncand = 30, nkf = 5, cap = 300;
    std::vector<int32_t> ints(8192);
    std::vector<uint8_t> bytes(4096);
    int32_t* a = ints.data();
    const uint8_t* o = bytes.data();
    auto off1 = [](auto* p) { return reinterpret_cast<decltype(p)>(reinterpret_cast<uintptr_t>(p) + 1); };       // a misaligned address (never read)
    {
        const CullList C{a, ncand};
        const CullColumns K{{a, a, nkf, cap}, o, 8};
        const CullOut O{a, a, a};
        auto cols = [&](const int32_t* s, const uint8_t* oc, const int32_t* n, int rows, int stride, int levels = 8) { return CullColumns{{s, n, rows, stride}, oc, levels}; };
        for (bool dev : {true, false}) {
            CHECK(check_cull(C, K, O, dev, dev) == ORBX_OK);
            CHECK(check_cull(CullList{nullptr, 0}, cols(nullptr, nullptr, nullptr, nkf, cap), CullOut{nullptr, nullptr, nullptr}, dev, dev) == ORBX_OK);      // no candidate
            CHECK(check_cull(C, cols(nullptr, nullptr, nullptr, 0, cap), CullOut{nullptr, nullptr, nullptr}, dev, dev) == ORBX_OK);                          // no row
            CHECK(check_cull(CullList{a, -1}, K, O, dev, dev) == ORBX_ERR_ARG && check_cull(CullList{a, ORBP_CULL_MAX_CANDIDATES + 1}, K, O, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(CullList{a, ORBP_CULL_MAX_CANDIDATES}, K, O, dev, dev) == ORBX_OK);
            CHECK(check_cull(C, cols(a, o, a, -1, cap), O, dev, dev) == ORBX_ERR_ARG && check_cull(C, cols(a, o, a, ORBP_LOCAL_MAX_ROWS + 1, 8), O, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(C, cols(a, o, a, ORBP_LOCAL_MAX_ROWS, 8), O, dev, dev) == ORBX_OK);
            CHECK(check_cull(C, cols(a, o, a, nkf, 0), O, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(C, cols(a, o, a, 1 << 15, 1 << 16), O, dev, dev) == ORBX_ERR_ARG);                                                                  // nkf * cap = 2^31
            CHECK(check_cull(C, cols(a, o, a, (1 << 15) - 1, 1 << 16), O, dev, dev) == ORBX_OK);
            CHECK(check_cull(C, cols(a, o, a, nkf, cap, 0), O, dev, dev) == ORBX_ERR_ARG && check_cull(C, cols(a, o, a, nkf, cap, ORBS_MAX_LEVELS + 1), O, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(C, cols(a, o, a, nkf, cap, 1), O, dev, dev) == ORBX_OK && check_cull(C, cols(a, o, a, nkf, cap, ORBS_MAX_LEVELS), O, dev, dev) == ORBX_OK);
            CHECK(check_cull(CullList{nullptr, ncand}, K, O, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(C, cols(nullptr, o, a, nkf, cap), O, dev, dev) == ORBX_ERR_ARG && check_cull(C, cols(a, nullptr, a, nkf, cap), O, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(C, cols(a, o, nullptr, nkf, cap), O, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(C, K, CullOut{nullptr, a, a}, dev, dev) == ORBX_ERR_ARG && check_cull(C, K, CullOut{a, nullptr, a}, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(C, K, CullOut{a, a, nullptr}, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_cull(C, cols(a, o + 1, a, nkf, cap), O, dev, dev) == ORBX_OK);                                                                         // bytes need no alignment
        }
        CHECK(check_cull(CullList{off1(a), ncand}, K, O, true, true) == ORBX_ERR_ARG && check_cull(CullList{off1(a), ncand}, K, O, false, true) == ORBX_OK);
        CHECK(check_cull(C, K, CullOut{off1(a), a, a}, true, true) == ORBX_ERR_ARG && check_cull(C, K, CullOut{a, off1(a), a}, true, true) == ORBX_ERR_ARG);
        CHECK(check_cull(C, K, CullOut{a, a, off1(a)}, true, true) == ORBX_ERR_ARG);
        CHECK(check_cull(C, cols(off1(a), o, a, nkf, cap), O, false, true) == ORBX_ERR_ARG);                                                                  // resident columns beside host candidates
        CHECK(check_cull(C, cols(a, o, off1(a), nkf, cap), O, true, true) == ORBX_ERR_ARG);
    }
    {
        // the layout: slots at multiples of 256, one span up, one down, nothing behind them
        const CullList C{a, ncand};
        const CullColumns K{{a, a, nkf, cap}, o, 8};
        const CullBlock B(C, K, true);
        CHECK(B.cand.off == 0 && B.kf_slot.off == 256 && B.kf_oct.off == 256 + 6144 && B.kf_nt.off == 6400 + 1536 && B.L.upload() == 7936 + 256);
        CHECK(B.nmps.off == 8192 && B.nred.off == 8448 && B.cull.off == 8704 && B.L.download() == 768 && B.L.total() == 8960 && B.nfeat == 1500);
        const CullBlock R(C, K, false);                                                                                                                      // resident columns: the candidates alone go up
        CHECK(!R.kf_slot.present && !R.kf_oct.present && !R.kf_nt.present && R.L.upload() == 256 && R.nmps.off == 256 && R.L.total() == 1024);
    }
    {
        // the calls through the handle's block: exact spans, sentinels, the steady state allocates and waits for nothing
        Handle m;
        CHECK(m.own.ensure() == hipSuccess && m.chain.ev.ensure() == hipSuccess);
        std::string log;
        CHECK(cull_call(m, 30, 5, 300, true, log) == 0 && log == "mmudry");
        const size_t h0 = m.block.h.size(), d0 = m.block.d.size();
        CHECK(cull_call(m, 30, 5, 300, true, log) == 0 && log == "sudry" && m.block.h.size() == h0 && m.block.d.size() == d0);
        CHECK(cull_call(m, 30, 5, 300, false, log) == 0 && log == "sudry");
        CHECK(cull_call(m, 1, 1, 1, true, log) == 0 && log == "sudry");
        CHECK(cull_call(m, ORBP_CULL_MAX_CANDIDATES, 200, 1000, true, log) == 0);
        CHECK(log.substr(0, 1) == "w" && m.block.h.size() > h0);                                                                                              // waits for the chain, then grows
        CHECK(cull_call(m, 80, 2000, 1000, false, log) == 0 && log == "sudry");
    }
    CHECK(hip_stub_live == 0);
    std::printf("cull host ok\n");
    return 0;
}
