// The host side of orbp_local_* and orbp_rows_purge_device on the CPU against tests/_probe/hip_stub: the argument checks that need no handle
// (orbp::check_local_votes, check_local_points, check_rows_purge), the layouts of the two host forms' blocks (orbp::LocalVotesBlock,
// orbp::LocalPointsBlock) and their path through orbx::Staged: the upload and download spans are exact, with sentinels around them, what the caller
// keeps on the device is passed through, and unpack copies of every problem the entries it has and no more (tests/test_local_map_host.py builds
// this under AddressSanitizer + UndefinedBehaviorSanitizer).
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

// One orbp_local_points over `m`'s block as orbp_project.hip writes it, the body standing in for the kernels: it checks what went up and answers
// into the download span (problem p lists counts[p] entries, which may exceed lcap).
int points_call(Handle& m, int np, int qcap, int rcap, int nkf, int cap, int lcap, bool with_query, bool kf_host, const std::vector<int>& counts, std::string& log) {
    std::vector<int32_t> query((size_t)np * qcap, 11), nquery(np, qcap), rows((size_t)np * rcap, 3), nrows(np, rcap), kf_slot((size_t)nkf * cap, 5), kf_nt(nkf > 0 ? nkf : 1, cap);
    const Query Q{with_query ? query.data() : nullptr, with_query ? nquery.data() : nullptr, qcap};
    const RowLists R{rows.data(), nrows.data(), rcap};
    const Columns K{kf_slot.data(), kf_nt.data(), nkf, cap};
    std::vector<int32_t> list((size_t)np * lcap, -5), nlist(np, -5), overflow(np, -5);
    std::vector<uint8_t> skip((size_t)np * lcap, 9);
    const LocalOut O{list.data(), nlist.data(), skip.data(), overflow.data(), lcap};
    CHECK(check_local_points(Q, np, R, K, O, false, !kf_host) == ORBX_OK);
    hip_stub_log.clear();
    hip_stub_up = hip_stub_down = {};
    Call<Handle> c(&m, nullptr);
    const LocalPointsBlock B(np, Q, R, K, lcap, kf_host);
    const size_t up = B.L.upload(), down = B.L.download(), total = B.L.total();
    CHECK(total == up + down);                                        // nothing device-only: the scratch is the handle's
    Staged<Handle> s(c, m.block, B.L);
    CHECK(s.fit() == ORBX_OK);
    const size_t hsize = m.block.h.size(), dsize = m.block.d.size();
    CHECK(hsize >= up + down && dsize >= total);
    std::memset(s.h, 0x11, up);
    std::memset(s.h + up, 0xA5, hsize - up);
    std::memset(s.d, 0x33, dsize);
    Query dq;
    RowLists dr;
    Columns dk;
    LocalOut dout;
    B.stage(s.h, s.d, Q, R, K, dq, dr, dk, dout);
    bool body_ok = false;
    const int rc = s.run([&] {
        const uint8_t* d = s.d;
        auto inside = [&](const void* p) { return (const uint8_t*)p >= d && (const uint8_t*)p < d + up; };
        body_ok = hip_stub_log.back() == 'u' && all(s.d + up, dsize - up, 0x33);
        body_ok = body_ok && (with_query ? inside(dq.q) && inside(dq.nq) && dq.q[(size_t)np * qcap - 1] == 11 && dq.nq[np - 1] == qcap : !dq.q && !dq.nq) && dq.qcap == qcap;
        body_ok = body_ok && inside(dr.rows) && inside(dr.nrows) && dr.rows[(size_t)np * rcap - 1] == 3 && dr.nrows[np - 1] == rcap && dr.rcap == rcap;
        if (kf_host && nkf > 0) body_ok = body_ok && inside(dk.slot) && inside(dk.nt) && dk.slot[(size_t)nkf * cap - 1] == 5 && dk.nt[nkf - 1] == cap;
        else if (!kf_host) body_ok = body_ok && dk.slot == kf_slot.data() && dk.nt == kf_nt.data();
        body_ok = body_ok && dk.nkf == nkf && dk.cap == cap && dout.lcap == lcap;
        body_ok = body_ok && (uint8_t*)dout.nlist == s.d + up && (uint8_t*)dout.skip + (size_t)np * lcap <= s.d + up + down;
        for (int p = 0; p < np; p++) {
            dout.nlist[p] = counts[p];
            dout.overflow[p] = counts[p] > lcap;
            for (int i = 0; i < lcap; i++) { dout.list[(size_t)p * lcap + i] = 100 * p + i; dout.skip[(size_t)p * lcap + i] = (uint8_t)(i & 1); }
        }
        return (int)ORBX_OK;
    });
    log = hip_stub_log;
    CHECK(rc == ORBX_OK && body_ok);
    CHECK(hip_stub_up.dst == s.d && hip_stub_up.src == s.h && hip_stub_up.bytes == up);
    CHECK(hip_stub_down.dst == s.h + up && hip_stub_down.src == s.d + up && hip_stub_down.bytes == down);
    CHECK(all(s.h + up + down, hsize - up - down, 0xA5) && all(s.d + up + down, dsize - up - down, 0x33));
    B.unpack(s.h, O);
    for (int p = 0; p < np; p++) {
        const int k = counts[p] < 0 ? 0 : (counts[p] > lcap ? lcap : counts[p]);
        CHECK(nlist[p] == counts[p] && overflow[p] == (counts[p] > lcap));
        for (int i = 0; i < lcap; i++) {
            CHECK(list[(size_t)p * lcap + i] == (i < k ? 100 * p + i : -5));
            CHECK(skip[(size_t)p * lcap + i] == (i < k ? (i & 1) : 9));
        }
    }
    // a caller who wants no overflow flags gets the rest
    std::vector<int32_t> nl2(np, -5);
    B.unpack(s.h, LocalOut{list.data(), nl2.data(), skip.data(), nullptr, lcap});
    CHECK(nl2[np - 1] == counts[np - 1]);
    return 0;
}

int votes_call(Handle& m, int np, int qcap, int nkf, int cap, bool kf_host, std::string& log) {
    std::vector<int32_t> query((size_t)np * qcap, 11), nquery(np, qcap), kf_slot((size_t)nkf * cap, 5), kf_nt(nkf, cap), votes((size_t)np * nkf + 1, -5);
    const Query Q{query.data(), nquery.data(), qcap};
    const Columns K{kf_slot.data(), kf_nt.data(), nkf, cap};
    CHECK(check_local_votes(Q, np, K, votes.data(), false, !kf_host) == ORBX_OK);
    hip_stub_log.clear();
    Call<Handle> c(&m, nullptr);
    const LocalVotesBlock B(np, Q, K, kf_host);
    const size_t up = B.L.upload(), down = B.L.download();
    CHECK(B.L.total() == up + down && B.nvotes == (size_t)np * nkf && down >= B.nvotes * 4 && B.in.kf_slot.present == kf_host);
    Staged<Handle> s(c, m.block, B.L);
    CHECK(s.fit() == ORBX_OK);
    Query dq;
    Columns dk;
    B.in.stage(s.h, s.d, Q, K, dq, dk);
    bool body_ok = false;
    const int rc = s.run([&] {
        body_ok = dq.q[(size_t)np * qcap - 1] == 11 && dq.nq[np - 1] == qcap && (kf_host ? dk.slot != kf_slot.data() && dk.slot[(size_t)nkf * cap - 1] == 5 && dk.nt[nkf - 1] == cap
                                                                                          : dk.slot == kf_slot.data() && dk.nt == kf_nt.data());
        int32_t* v = Layout::at(s.d, B.votes);
        body_ok = body_ok && (uint8_t*)v == s.d + up;
        for (size_t i = 0; i < B.nvotes; i++) v[i] = (int32_t)i;
        return (int)ORBX_OK;
    });
    log = hip_stub_log;
    CHECK(rc == ORBX_OK && body_ok && hip_stub_up.bytes == up && hip_stub_down.bytes == down);
    std::memcpy(votes.data(), Layout::at(s.h, B.votes), B.nvotes * 4);
    CHECK(votes[B.nvotes - 1] == (int32_t)B.nvotes - 1 && votes[B.nvotes] == -5);
    return 0;
}
}  // namespace

int main() {
    const int np = 3, qcap = 50, rcap = 7, nkf = 5, cap = 300, lcap = 40;
    std::vector<int32_t> ints(8192);
    std::vector<uint8_t> bytes(4096);
    int32_t* a = ints.data();
    auto off1 = [](auto* p) { return reinterpret_cast<decltype(p)>(reinterpret_cast<uintptr_t>(p) + 1); };       // a misaligned address (never read)
    {
        // orbp_local_votes*: on the device (alignment matters) and on the host
        const Query Q{a, a, qcap};
        const Columns K{a, a, nkf, cap};
        for (bool dev : {true, false}) {
            CHECK(check_local_votes(Q, np, K, a, dev, dev) == ORBX_OK);
            CHECK(check_local_votes(Query{nullptr, nullptr, 1}, 0, Columns{nullptr, nullptr, 0, 1}, nullptr, dev, dev) == ORBX_OK);       // no problem
            CHECK(check_local_votes(Q, np, Columns{nullptr, nullptr, 0, cap}, nullptr, dev, dev) == ORBX_OK);                             // no row
            CHECK(check_local_votes(Q, -1, K, a, dev, dev) == ORBX_ERR_ARG && check_local_votes(Q, ORBP_LOCAL_MAX_PROBLEMS + 1, K, a, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_local_votes(Q, ORBP_LOCAL_MAX_PROBLEMS, K, a, dev, dev) == ORBX_OK);
            CHECK(check_local_votes(Query{a, a, 0}, np, K, a, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_local_votes(Q, np, Columns{a, a, -1, cap}, a, dev, dev) == ORBX_ERR_ARG && check_local_votes(Q, np, Columns{a, a, nkf, 0}, a, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_local_votes(Q, np, Columns{a, a, 1 << 16, 1 << 15}, a, dev, dev) == ORBX_ERR_ARG);                                 // nkf * cap = 2^31
            CHECK(check_local_votes(Q, np, Columns{a, a, (1 << 16) - 1, 1 << 15}, a, dev, dev) == ORBX_OK);
            CHECK(check_local_votes(Query{nullptr, a, qcap}, np, K, a, dev, dev) == ORBX_ERR_ARG && check_local_votes(Query{a, nullptr, qcap}, np, K, a, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_local_votes(Q, np, Columns{nullptr, a, nkf, cap}, a, dev, dev) == ORBX_ERR_ARG && check_local_votes(Q, np, Columns{a, nullptr, nkf, cap}, a, dev, dev) == ORBX_ERR_ARG);
            CHECK(check_local_votes(Q, np, K, nullptr, dev, dev) == ORBX_ERR_ARG);
        }
        CHECK(check_local_votes(Query{off1(a), a, qcap}, np, K, a, true, true) == ORBX_ERR_ARG && check_local_votes(Q, np, K, off1(a), true, true) == ORBX_ERR_ARG);
        CHECK(check_local_votes(Q, np, Columns{off1(a), a, nkf, cap}, a, false, true) == ORBX_ERR_ARG);                                   // resident columns beside host queries
        CHECK(check_local_votes(Q, np, Columns{a, off1(a), nkf, cap}, a, true, true) == ORBX_ERR_ARG);
    }
    {
        // orbp_local_points*
        const Query Q{a, a, qcap};
        const RowLists R{a, a, rcap};
        const Columns K{a, a, nkf, cap};
        const LocalOut O{a, a, bytes.data(), a, lcap};
        auto chk = [&](const Query& q, int n, const RowLists& r, const Columns& k, const LocalOut& o, bool dev = true) { return check_local_points(q, n, r, k, o, dev, dev); };
        for (bool dev : {true, false}) {
            CHECK(chk(Q, np, R, K, O, dev) == ORBX_OK);
            CHECK(chk(Query{nullptr, nullptr, 1}, np, R, K, O, dev) == ORBX_OK);                                                          // no query: no flag
            CHECK(chk(Query{a, nullptr, qcap}, np, R, K, O, dev) == ORBX_ERR_ARG);
            CHECK(chk(Query{nullptr, nullptr, 1}, 0, RowLists{nullptr, nullptr, 1}, Columns{nullptr, nullptr, 0, 1}, LocalOut{nullptr, nullptr, nullptr, nullptr, 1}, dev) == ORBX_OK);
            CHECK(chk(Q, np, R, Columns{nullptr, nullptr, 0, cap}, O, dev) == ORBX_OK);                                                  // no row to name: every list is empty
            CHECK(chk(Q, -1, R, K, O, dev) == ORBX_ERR_ARG && chk(Q, ORBP_LOCAL_MAX_PROBLEMS + 1, R, K, O, dev) == ORBX_ERR_ARG);
            CHECK(chk(Query{a, a, 0}, np, R, K, O, dev) == ORBX_ERR_ARG);
            CHECK(chk(Q, np, RowLists{a, a, 0}, K, O, dev) == ORBX_ERR_ARG && chk(Q, np, RowLists{a, a, ORBP_LOCAL_MAX_ROWS + 1}, K, O, dev) == ORBX_ERR_ARG);
            CHECK(chk(Q, np, RowLists{a, a, ORBP_LOCAL_MAX_ROWS}, Columns{a, a, nkf, 16}, O, dev) == ORBX_OK);
            CHECK(chk(Q, np, RowLists{a, a, 1 << 15}, Columns{a, a, 4, 1 << 16}, O, dev) == ORBX_ERR_ARG);                               // rcap * cap = 2^31
            CHECK(chk(Q, np, R, Columns{a, a, -1, cap}, O, dev) == ORBX_ERR_ARG && chk(Q, np, R, Columns{a, a, nkf, 0}, O, dev) == ORBX_ERR_ARG);
            CHECK(chk(Q, np, R, Columns{a, a, 1 << 16, 1 << 15}, O, dev) == ORBX_ERR_ARG);
            CHECK(chk(Q, np, R, K, LocalOut{a, a, bytes.data(), a, 0}, dev) == ORBX_ERR_ARG);
            CHECK(chk(Q, 2, R, K, LocalOut{a, a, bytes.data(), a, 1 << 30}, dev) == ORBX_ERR_ARG && chk(Q, 1, R, K, LocalOut{a, a, bytes.data(), a, 1 << 30}, dev) == ORBX_OK);
            CHECK(chk(Q, np, RowLists{nullptr, a, rcap}, K, O, dev) == ORBX_ERR_ARG && chk(Q, np, RowLists{a, nullptr, rcap}, K, O, dev) == ORBX_ERR_ARG);
            CHECK(chk(Q, np, R, Columns{nullptr, a, nkf, cap}, O, dev) == ORBX_ERR_ARG && chk(Q, np, R, Columns{a, nullptr, nkf, cap}, O, dev) == ORBX_ERR_ARG);
            CHECK(chk(Q, np, R, K, LocalOut{nullptr, a, bytes.data(), a, lcap}, dev) == ORBX_ERR_ARG && chk(Q, np, R, K, LocalOut{a, nullptr, bytes.data(), a, lcap}, dev) == ORBX_ERR_ARG);
            CHECK(chk(Q, np, R, K, LocalOut{a, a, nullptr, a, lcap}, dev) == ORBX_ERR_ARG);
        }
        CHECK(chk(Q, np, R, K, LocalOut{a, a, bytes.data(), nullptr, lcap}, true) == ORBX_ERR_ARG);                                       // the flags are required on the device,
        CHECK(chk(Q, np, R, K, LocalOut{a, a, bytes.data(), nullptr, lcap}, false) == ORBX_OK);                                           // optional on the host
        CHECK(chk(Q, np, R, K, LocalOut{a, a, bytes.data() + 1, a, lcap}, true) == ORBX_OK);                                              // bytes need no alignment
        CHECK(chk(Query{off1(a), a, qcap}, np, R, K, O) == ORBX_ERR_ARG && chk(Q, np, RowLists{off1(a), a, rcap}, K, O) == ORBX_ERR_ARG);
        CHECK(chk(Q, np, RowLists{a, off1(a), rcap}, K, O) == ORBX_ERR_ARG && chk(Q, np, R, Columns{off1(a), a, nkf, cap}, O) == ORBX_ERR_ARG);
        CHECK(chk(Q, np, R, K, LocalOut{off1(a), a, bytes.data(), a, lcap}) == ORBX_ERR_ARG && chk(Q, np, R, K, LocalOut{a, off1(a), bytes.data(), a, lcap}) == ORBX_ERR_ARG);
        CHECK(chk(Q, np, R, K, LocalOut{a, a, bytes.data(), off1(a), lcap}) == ORBX_ERR_ARG);
    }
    {
        // orbp_rows_purge_device
        CHECK(check_rows_purge(a, 4, a, nkf, cap) == ORBX_OK && check_rows_purge(nullptr, 0, nullptr, nkf, cap) == ORBX_OK && check_rows_purge(a, 4, nullptr, 0, cap) == ORBX_OK);
        CHECK(check_rows_purge(a, -1, a, nkf, cap) == ORBX_ERR_ARG && check_rows_purge(nullptr, 4, a, nkf, cap) == ORBX_ERR_ARG && check_rows_purge(a, 4, nullptr, nkf, cap) == ORBX_ERR_ARG);
        CHECK(check_rows_purge(a, 4, off1(a), nkf, cap) == ORBX_ERR_ARG && check_rows_purge(a, 4, a, -1, cap) == ORBX_ERR_ARG && check_rows_purge(a, 4, a, nkf, 0) == ORBX_ERR_ARG);
        CHECK(check_rows_purge(a, 4, a, 1 << 16, 1 << 15) == ORBX_ERR_ARG);
    }
    {
        // the layouts: slots at multiples of 256, one span up, one down, nothing behind them
        CHECK(local_tiles(1) == 1 && local_tiles(256) == 1 && local_tiles(257) == 2 && local_tiles(300) == 2 && local_tile_words(5, 7, 300) == 70);
        const Query Q{a, a, qcap};
        const RowLists R{a, a, rcap};
        const Columns K{a, a, nkf, cap};
        const LocalPointsBlock B(np, Q, R, K, lcap, true);
        CHECK(B.in.query.off == 0 && B.in.nquery.off == 768 && B.in.kf_slot.off == 1024 && B.in.kf_nt.off == 1024 + 6144 && B.rows.off == 7424 && B.nrows.off == 7680 && B.L.upload() == 7936);
        CHECK(B.nlist.off == 7936 && B.overflow.off == 8192 && B.list.off == 8448 && B.skip.off == 8448 + 512 && B.L.download() == 1024 + 256 && B.L.total() == 7936 + 1280);
        const LocalPointsBlock C(np, Query{nullptr, nullptr, 1}, R, K, lcap, false);                                                       // resident columns, no query: the rows alone go up
        CHECK(!C.in.query.present && !C.in.nquery.present && !C.in.kf_slot.present && !C.in.kf_nt.present && C.rows.off == 0 && C.L.upload() == 512);
        const LocalVotesBlock V(np, Q, K, false);
        CHECK(V.in.query.present && !V.in.kf_slot.present && V.L.upload() == 1024 && V.votes.off == 1024 && V.L.download() == 256 && V.nvotes == 15);
    }
    {
        // the calls through the handle's block: exact spans, sentinels, the steady state allocates and waits for nothing
        Handle m;
        CHECK(m.own.ensure() == hipSuccess && m.chain.ev.ensure() == hipSuccess);
        std::string log;
        CHECK(points_call(m, 3, 50, 7, 5, 300, 40, true, true, {0, 17, 40}, log) == 0 && log == "mmudry");
        const size_t h0 = m.block.h.size(), d0 = m.block.d.size();
        CHECK(points_call(m, 3, 50, 7, 5, 300, 40, true, true, {41, 1000, -3}, log) == 0 && log == "sudry" && m.block.h.size() == h0 && m.block.d.size() == d0);   // overflow, a count below 0
        CHECK(points_call(m, 3, 50, 7, 5, 300, 40, false, false, {40, 39, 1}, log) == 0 && log == "sudry");
        CHECK(points_call(m, 1, 1, 1, 0, 1, 1, false, true, {0}, log) == 0 && log == "sudry");                                                             // no row at all
        CHECK(points_call(m, ORBP_LOCAL_MAX_PROBLEMS, 1000, 80, 200, 1000, 8000, true, true, std::vector<int>(ORBP_LOCAL_MAX_PROBLEMS, 7999), log) == 0);
        CHECK(log.substr(0, 1) == "w" && m.block.h.size() > h0);                                                                                          // waits for the chain, then grows
        CHECK(votes_call(m, 3, 50, 5, 300, true, log) == 0 && log == "sudry");
        CHECK(votes_call(m, 30, 1000, 200, 1000, false, log) == 0 && log == "sudry");
        CHECK(votes_call(m, 1, 1, 1, 1, true, log) == 0);
    }
    CHECK(hip_stub_live == 0);
    std::printf("local map host ok\n");
    return 0;
}
