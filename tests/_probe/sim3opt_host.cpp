// The host side of the Sim3 refinement (include/orbg.h) on the CPU against tests/_probe/hip_stub: the argument checks in front of the launch
// (orbg_host.h), the packing of a candidate's arrays into its pair table, the one-shot staging the host forms use (orbx::Staging) with the layout of
// orbg_sim3_batch, and the shared arithmetic (orbg_math.h) through the host route (tools/sim3opt_host_route.cpp, compiled into this program): n
// from 0 to the limit, the lane and word edges, the four branches of Sim3(update), a NaN coordinate, a point with z = 0, a point behind the cameras,
// every pair removed, and a batch against the single calls.  tests/test_sim3opt_host.py builds this under AddressSanitizer +
// UndefinedBehaviorSanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_host.h"
#include "../../tools/sim3opt_host_route.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {

uint32_t lcg_state = 9876u;
double uniform() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (lcg_state >> 8) / 16777216.0;
}

struct Scene {
    std::vector<float> P1, P2, o1, o2;
    orbg_problem q;
    float S12[13];
};

// camera 2 rotated about y, shifted and scaled against camera 1: P1 = s*R*P2 + t; every fifth pair displaced on side 1 or side 2 in turn; the
// start is the identity with scale 1
Scene make_scene(int n, double displaced = 40.0) {
    Scene sc;
    sc.q = orbg_problem{517.3f, 516.5f, 318.6f, 255.3f, 535.4f, 539.2f, 320.1f, 247.6f, 10.0f, n};
    const float I[13] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(sc.S12, I, sizeof(I));
    const double c = std::cos(0.04), sn = std::sin(0.04), t[3] = {0.05, -0.04, 0.06}, s = 1.05;
    for (int i = 0; i < n; i++) {
        const float X = (float)(uniform() * 4 - 2), Y = (float)(uniform() * 3 - 1.5), Z = (float)(3 + uniform() * 5);       // P2
        const double x = s * (c * X + sn * Z) + t[0], y = s * Y + t[1], z = s * (-sn * X + c * Z) + t[2];                  // P1
        double u1 = 517.3 * x / z + 318.6 + 0.3 * (uniform() - 0.5), v1 = 516.5 * y / z + 255.3 + 0.3 * (uniform() - 0.5);
        double u2 = 535.4 * X / Z + 320.1 + 0.3 * (uniform() - 0.5), v2 = 539.2 * Y / Z + 247.6 + 0.3 * (uniform() - 0.5);
        if (i % 10 == 4) { u1 += displaced; v1 -= displaced; }
        if (i % 10 == 9) { u2 -= displaced; v2 += displaced; }
        const float sigma2 = (float)std::pow(1.44, i % 3);
        sc.P1.insert(sc.P1.end(), {(float)x, (float)y, (float)z});
        sc.P2.insert(sc.P2.end(), {X, Y, Z});
        sc.o1.insert(sc.o1.end(), {(float)u1, (float)v1, 1.0f / sigma2});
        sc.o2.insert(sc.o2.end(), {(float)u2, (float)v2, sigma2});
    }
    return sc;
}

int popcount(const std::vector<uint64_t>& w) {
    int c = 0;
    for (uint64_t x : w) c += __builtin_popcountll(x);
    return c;
}

bool finite_result(const orbg_result& r) {
    bool ok = std::isfinite(r.s);
    for (float v : r.S12) ok = ok && std::isfinite(v);
    for (double v : r.q) ok = ok && std::isfinite(v);
    for (double v : r.t) ok = ok && std::isfinite(v);
    return ok;
}

int run(const Scene& s, orbg_result& r, std::vector<uint64_t>& fl, std::vector<orbo_step>& tr) {
    fl.assign(ORBO_WORDS(s.q.n) + 1, 0xdeadbeefdeadbeefull);          // one word past the end must stay as it is
    tr.assign(ORBG_MAX_ITERS, orbo_step{});
    const int rc = orbg_sim3(&s.q, s.P1.data(), s.P2.data(), s.o1.data(), s.o2.data(), s.S12, &r, fl.data(), tr.data(), 0);
    if (fl.back() != 0xdeadbeefdeadbeefull) return -100;
    fl.pop_back();
    return rc;
}

}  // namespace

int main() {
    // ---- argument checks ----
    const orbg_problem good = {500, 500, 320, 240, 510, 510, 318, 242, 10, 60};
    CHECK(orbg::check_problem(good) == ORBX_OK);
    for (int k = 0; k < 2; k++) {
        orbg_problem b = good;
        b.n = k == 0 ? -1 : ORBG_MAX_PAIRS + 1;
        CHECK(orbg::check_problem(b) == ORBX_ERR_ARG);
        orbg::Problems PR;
        CHECK(orbg::check_batch(&b, 1, ORBG_MAX_PAIRS, PR) == ORBX_ERR_ARG);
    }
    {
        orbg::Problems PR;
        CHECK(orbg::check_batch(&good, 1, 60, PR) == ORBX_OK && PR.p[0].n == 60);
        CHECK(orbg::check_batch(&good, 1, 59, PR) == ORBX_ERR_ARG);                    // a cap below the problem's n
        CHECK(orbg::check_batch(&good, 0, 60, PR) == ORBX_ERR_ARG);
        CHECK(orbg::check_batch(&good, ORBG_MAX_PROBLEMS + 1, 60, PR) == ORBX_ERR_ARG);
        CHECK(orbg::check_batch(nullptr, 1, 60, PR) == ORBX_ERR_ARG);
        CHECK(orbg::check_batch(&good, 1, 0, PR) == ORBX_ERR_ARG);
        CHECK(orbg::check_batch(&good, 1, ORBG_MAX_PAIRS + 1, PR) == ORBX_ERR_ARG);
        orbg_problem empty = good;
        empty.n = 0;
        CHECK(orbg::check_batch(&empty, 1, 1, PR) == ORBX_OK);
        float f = 0;
        uint64_t w = 0;
        CHECK(orbg::check_candidate(empty, nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
        CHECK(orbg::check_candidate(good, &f, &f, nullptr, &f, &w) == ORBX_ERR_ARG);
        orbg_result r;
        CHECK(orbg_sim3(nullptr, &f, &f, &f, &f, &f, &r, &w, nullptr, 0) == ORBX_ERR_ARG);
        CHECK(orbg_sim3(&good, &f, &f, &f, &f, nullptr, &r, &w, nullptr, 0) == ORBX_ERR_ARG);
        CHECK(orbg_sim3(&good, &f, &f, &f, &f, &f, nullptr, &w, nullptr, 0) == ORBX_ERR_ARG);
        CHECK(orbg_sim3(&good, &f, &f, &f, &f, &f, &r, nullptr, nullptr, 0) == ORBX_ERR_ARG);
    }
    // ---- the pair table and the staging layout of orbg_sim3_batch ----
    {
        const Scene s = make_scene(70);
        const int cap = 130;
        std::vector<float> table((size_t)ORBG_PAIR_ROWS * cap, -1.0f);
        orbg::pack_pairs(70, cap, s.P1.data(), s.P2.data(), s.o1.data(), s.o2.data(), table.data());
        CHECK(table[0 * cap + 69] == s.P1[69 * 3] && table[5 * cap + 69] == s.P2[69 * 3 + 2] && table[8 * cap + 69] == s.o1[69 * 3 + 2]);
        CHECK(table[11 * cap + 69] == s.o2[69 * 3 + 2] && table[11 * cap + 70] == -1.0f && table[0 * cap + 70] == -1.0f);
        orbx::Staging st;
        const auto ip = st.in(table.data(), table.size());
        const auto is = st.in(s.S12, 13);
        const auto orr = st.out<orbg_result>(1);
        const auto of = st.out<uint64_t>(ORBO_WORDS(cap));
        const auto ot = st.out<orbo_step>(0);
        CHECK(st.alloc() == hipSuccess);
        CHECK(st[ip] && st[is] && st[orr] && st[of] && st[ot]);
        std::vector<float> back(table.size());
        CHECK(st.get(back.data(), ip, back.size()) == hipSuccess && back == table);
    }
    // ---- Sim3(update): the four branches, each against exp(sigma) and a rotation by theta ----
    for (int k = 0; k < 4; k++) {
        const double th = (k & 1) ? 0.3 : 1e-7, sg = (k & 2) ? 0.2 : 1e-8;
        const double x[7] = {0.0, th, 0.0, 0.1, -0.2, 0.3, sg};
        orbg::Sim3 S, Si, P;
        orbg::sim3_exp(x, S);
        CHECK(S.s == std::exp(sg) && std::fabs(S.q[1] - std::sin(th / 2)) < 1e-6 && std::fabs(S.t[1] + 0.2 * (k & 2 ? (S.s - 1) / sg : 1.0)) < 1e-6);
        orbg::sim3_inverse(S, Si);
        orbg::sim3_mul(S, Si, P);
        CHECK(std::fabs(P.s - 1) < 1e-12 && std::fabs(P.t[0]) < 1e-12 && std::fabs(P.t[2]) < 1e-12 && std::fabs(std::fabs(P.q[3]) - 1) < 1e-6);
    }
    // ---- the arithmetic through the host route ----
    orbg_result r;
    std::vector<uint64_t> fl;
    std::vector<orbo_step> tr;
    for (int n : {0, 1, 9, 10, 11, 63, 64, 65, 127, 128, 129, 300, ORBG_MAX_PAIRS}) {
        const Scene s = make_scene(n);
        CHECK(run(s, r, fl, tr) == ORBX_OK);
        CHECK(finite_result(r) && r.ncorr == n && r.nbad <= popcount(fl));
        CHECK(r.S12[12] == 0.0f && r.S12[13] == 0.0f && r.S12[14] == 0.0f && r.S12[15] == 1.0f);
        const int planted = (n + 5) / 10 + n / 10;
        if (n - planted < 10) CHECK(r.ret0 == 1 && r.nin == 0 && r.iters[1] == 0 && r.s == 1.0 && r.q[3] == 1.0 && r.t[0] == 0.0 && tr[5].status == 2);
        if (n >= 20) {
            CHECK(r.ret0 == 0 && r.nbad == planted && r.nin == n - popcount(fl) && popcount(fl) == planted);
            CHECK(std::fabs(r.s - 1.05) < 0.01 && std::fabs(r.t[0] - 0.05) < 0.02 && std::fabs(r.t[1] + 0.04) < 0.02 && std::fabs(r.t[2] - 0.06) < 0.03);
            for (int i = 0; i < n; i++) CHECK(((fl[i / 64] >> (i % 64)) & 1) == (uint64_t)(i % 5 == 4));                       // the displaced pairs
            CHECK(r.iters[0] >= 1 && r.iters[0] <= 5 && r.iters[1] >= 1 && r.iters[1] <= 10);
        }
        if (n == 0) CHECK(r.q[3] == 1.0 && r.s == 1.0 && r.nbad == 0 && r.ret0 == 1 && tr[0].status == 2 && tr[14].status == 2);
        if (n % 64) CHECK((fl.back() >> (n % 64)) == 0);                                                                       // zero bits past n
    }
    {   // a NaN pair and a pair with z = 0 on both sides: a NaN chi2 fails both comparisons, the pair stays and counts as an inlier; every
        // trial is rejected on a NaN rho and the estimate stays
        for (int k = 0; k < 2; k++) {
            Scene s = make_scene(40);
            for (int c = 0; c < 3; c++) s.P1[7 * 3 + c] = s.P2[7 * 3 + c] = k == 0 ? NAN : 0.0f;         // z = 0 at t = 0: 0/0 on both sides
            CHECK(run(s, r, fl, tr) == ORBX_OK);
            CHECK(r.q[3] == 1.0 && r.t[0] == 0.0 && r.s == 1.0);
            CHECK(((fl[0] >> 7) & 1) == 0 && r.iters[0] == 5 && tr[0].trials == 1 && tr[0].status == 0);
        }
    }
    {   // a point behind both cameras is a pair like any other
        Scene s = make_scene(40);
        s.P1[11 * 3 + 2] = -3.0f;
        s.P2[11 * 3 + 2] = -3.0f;
        CHECK(run(s, r, fl, tr) == ORBX_OK);
        CHECK(finite_result(r) && std::fabs(r.s - 1.05) < 0.02);
    }
    {   // every pair removed by the first check: ret0 with every flag set
        Scene s = make_scene(20);
        for (int i = 0; i < 20; i++) { s.o1[i * 3] += (float)(150 + 100 * uniform()) * (i % 2 ? 1 : -1); s.o1[i * 3 + 1] -= (float)(150 + 100 * uniform()) * (i % 3 ? 1 : -1); }
        CHECK(run(s, r, fl, tr) == ORBX_OK);
        CHECK(finite_result(r) && r.ret0 == 1 && r.nbad == 20 && popcount(fl) == 20 && r.iters[1] == 0 && r.s == 1.0);
    }
    {   // a batch against the single calls
        const int ns[5] = {10, 65, 0, 130, 9};
        std::vector<Scene> ss;
        for (int n : ns) ss.push_back(make_scene(n));
        std::vector<orbg_problem> q;
        std::vector<const float*> a1, a2, b1, b2;
        std::vector<float> S;
        std::vector<std::vector<uint64_t>> words(5);
        std::vector<uint64_t*> wp;
        for (int p = 0; p < 5; p++) {
            q.push_back(ss[p].q);
            a1.push_back(ns[p] ? ss[p].P1.data() : nullptr);
            a2.push_back(ns[p] ? ss[p].P2.data() : nullptr);
            b1.push_back(ns[p] ? ss[p].o1.data() : nullptr);
            b2.push_back(ns[p] ? ss[p].o2.data() : nullptr);
            S.insert(S.end(), ss[p].S12, ss[p].S12 + 13);
            words[p].assign(ORBO_WORDS(ns[p]), 0);
            wp.push_back(ns[p] ? words[p].data() : nullptr);
        }
        std::vector<orbg_result> res(5);
        CHECK(orbg_sim3_batch(q.data(), 5, a1.data(), a2.data(), b1.data(), b2.data(), S.data(), res.data(), wp.data(), nullptr, 0) == ORBX_OK);
        for (int p = 0; p < 5; p++) {
            CHECK(run(ss[p], r, fl, tr) == ORBX_OK);
            CHECK(std::memcmp(&r, &res[p], sizeof(r)) == 0 && fl == words[p]);
        }
        a1[1] = nullptr;
        CHECK(orbg_sim3_batch(q.data(), 5, a1.data(), a2.data(), b1.data(), b2.data(), S.data(), res.data(), wp.data(), nullptr, 0) == ORBX_ERR_ARG);
    }
    std::printf("sim3opt host ok\n");
    return 0;
}
