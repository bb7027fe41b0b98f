// The host side of the Sim3 RANSAC (include/orbh.h) on the CPU against tests/_probe/hip_stub: the argument checks in front of the launches
// (orbh_host.h), the packing of a solver's arrays into its point table, the one-shot staging the host forms use (orbx::Staging) with the layouts of
// orbh_iterate_batch, and the shared arithmetic (orbh_math.h over orb_jacobi.h) through the host route (tools/sim3solver_host_route.cpp, compiled
// into this program): N from 3 to the limit, sets with a repeated index and an index outside, NaN coordinates, a point with z = 0, equal triples and
// three calls of iterate over one state.  tests/test_sim3solver_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_host.h"
#include "../../tools/sim3solver_host_route.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {

uint32_t lcg_state = 12345u;
double uniform() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (lcg_state >> 8) / 16777216.0;
}

struct Scene {
    std::vector<float> x1, x2, u1, u2, m1, m2;
    orbh_problem q;
};

// X1 = s R X2 + t with a rotation about y, every fourth correspondence an outlier
Scene make_scene(int N, int iters, int min_inliers, double scale) {
    Scene s;
    s.q = orbh_problem{500.0f, 510.0f, 320.0f, 240.0f, 505.0f, 515.0f, 322.0f, 238.0f, N, iters, min_inliers, iters};
    const double c = std::cos(0.2), sn = std::sin(0.2), t[3] = {0.1, -0.2, 0.3};
    for (int i = 0; i < N; i++) {
        double X = uniform() * 4 - 2, Y = uniform() * 3 - 1.5, Z = 3 + uniform() * 5;
        const double a = scale * (c * X + sn * Z) + t[0], b = scale * Y + t[1], d = scale * (-sn * X + c * Z) + t[2];
        if (i % 4 == 3) { X = uniform() * 4 - 2; Y = uniform() * 3 - 1.5; }
        const float p1[3] = {(float)a, (float)b, (float)d}, p2[3] = {(float)X, (float)Y, (float)Z};
        s.x1.insert(s.x1.end(), p1, p1 + 3);
        s.x2.insert(s.x2.end(), p2, p2 + 3);
        s.u1.insert(s.u1.end(), {500.0f * (p1[0] / p1[2]) + 320.0f, 510.0f * (p1[1] / p1[2]) + 240.0f});
        s.u2.insert(s.u2.end(), {505.0f * (p2[0] / p2[2]) + 322.0f, 515.0f * (p2[1] / p2[2]) + 238.0f});
        s.m1.push_back(orbh::max_error(1.0f));
        s.m2.push_back(orbh::max_error(1.44f));
    }
    return s;
}

std::vector<int32_t> make_sets(int N, int iters) {
    std::vector<int32_t> sets((size_t)iters * 3);
    for (int32_t& x : sets) x = (int32_t)(uniform() * N) % N;
    return sets;
}

bool finite_block(const orbh_hyp& h) {
    bool ok = std::isfinite(h.s);
    for (float v : h.T12) ok = ok && std::isfinite(v);
    for (float v : h.T21) ok = ok && std::isfinite(v);
    return ok;
}

}  // namespace

int main() {
    // ---- argument checks ----
    const orbh_problem good = {500, 500, 320, 240, 500, 500, 320, 240, 60, 35, 20, 35};
    CHECK(orbh::check_problem(good) == ORBX_OK);
    for (int k = 0; k < 6; k++) {
        orbh_problem b = good;
        if (k == 0) b.n = 2;
        if (k == 1) b.n = ORBH_MAX_POINTS + 1;
        if (k == 2) b.iters = 0;
        if (k == 3) b.iters = ORBH_MAX_ITERS + 1;
        if (k == 4) b.min_inliers = -1;
        if (k == 5) b.max_its = 0;
        CHECK(orbh::check_problem(b) == ORBX_ERR_ARG);
        orbh::Problems PR;
        int iters = 0;
        CHECK(orbh::check_batch(&b, 1, ORBH_MAX_POINTS, ORBH_MAX_ITERS, PR, iters) == ORBX_ERR_ARG);
    }
    {
        orbh::Problems PR;
        int iters = 0;
        orbh_problem two[2] = {good, good};
        two[1].iters = 5;
        CHECK(orbh::check_batch(two, 2, 60, 35, PR, iters) == ORBX_OK && iters == 35 && PR.p[1].iters == 5);
        CHECK(orbh::check_batch(two, 2, 59, 35, PR, iters) == ORBX_ERR_ARG);
        CHECK(orbh::check_batch(two, 2, 60, 34, PR, iters) == ORBX_ERR_ARG);
        CHECK(orbh::check_batch(two, 0, 60, 35, PR, iters) == ORBX_ERR_ARG);
        CHECK(orbh::check_batch(two, ORBH_MAX_PROBLEMS + 1, 60, 35, PR, iters) == ORBX_ERR_ARG);
        CHECK(orbh::check_batch(nullptr, 1, 60, 35, PR, iters) == ORBX_ERR_ARG);
        orbh_state st;
        std::memset(&st, 0, sizeof(st));
        CHECK(orbh::check_state(st) == ORBX_OK);
        st.iterations = -1;
        CHECK(orbh::check_state(st) == ORBX_ERR_ARG);
    }
    static_assert(sizeof(orbh_problem) == 48 && sizeof(orbh_hyp) == 216 && sizeof(orbh_state) == 124 && sizeof(orbh_result) == 80, "the records of capi.py");

    // ---- SetRansacParameters and the max errors ----
    {
        int32_t mx = 0;
        CHECK(orbh_ransac_parameters(20, 0.99, 20, 300, &mx) == ORBX_OK && mx == 1);
        CHECK(orbh_ransac_parameters(100, 0.99, 20, 300, &mx) == ORBX_OK && mx == 300);
        CHECK(orbh_ransac_parameters(30, 0.99, 20, 300, &mx) == ORBX_OK && mx == 14);
        CHECK(orbh_ransac_parameters(10, 0.99, 20, 300, &mx) == ORBX_OK && mx == 1);       // epsilon > 1: the logarithm of a negative number
        CHECK(orbh_ransac_parameters(0, 0.99, 20, 300, &mx) == ORBX_OK && mx == 1);
        CHECK(orbh_ransac_parameters(-1, 0.99, 20, 300, &mx) == ORBX_ERR_ARG && orbh_ransac_parameters(5, 0.99, 20, 300, nullptr) == ORBX_ERR_ARG);
        const float s2[4] = {1.0f, 1.44f, 2.0736f, NAN};
        float me[4];
        CHECK(orbh_max_errors(4, s2, me) == ORBX_OK && me[0] == 9.0f && me[1] == 13.0f && me[2] == 19.0f && me[3] == 0.0f);
        CHECK(orbh_max_errors(1, nullptr, me) == ORBX_ERR_ARG);
    }

    // ---- the point table and the staging of orbh_iterate_batch: every slot inside the block, the inputs where they were put ----
    {
        const int N = 70, cap = 100, I = 35, W = ORBH_WORDS(cap);
        Scene s = make_scene(N, I, 20, 1.0);
        std::vector<float> table((size_t)ORBH_POINT_ROWS * cap, -1.0f);
        orbh::pack_points(N, cap, s.x1.data(), s.x2.data(), s.u1.data(), s.u2.data(), s.m1.data(), s.m2.data(), table.data());
        CHECK(table[0 * cap + 69] == s.x1[69 * 3] && table[5 * cap + 3] == s.x2[3 * 3 + 2] && table[9 * cap + 7] == s.u2[7 * 2 + 1]);
        CHECK(table[11 * cap + 69] == s.m2[69] && table[11 * cap + 70] == -1.0f && table[0 * cap + 70] == -1.0f);
        std::vector<int32_t> sets((size_t)I * 3, 7);
        orbx::Staging st;
        const auto ip = st.in(table.data(), table.size());
        const auto is = st.in(sets.data(), sets.size());
        const auto oh = st.out<orbh_hyp>(I);
        const auto of = st.out<uint64_t>((size_t)I * W);
        const auto orr = st.out<orbh_result>(1);
        CHECK(st.alloc() == hipSuccess);
        CHECK(st[ip][table.size() - 1] == -1.0f && st[is][I * 3 - 1] == 7);
        CHECK(((uintptr_t)st[oh] & 7) == 0 && ((uintptr_t)st[of] & 7) == 0 && ((uintptr_t)st[orr] & 3) == 0);
        std::memset(&st[oh][I - 1], 0, sizeof(orbh_hyp));
        st[of][(size_t)I * W - 1] = 9;
        uint64_t back = 0;
        CHECK(st.get(&back, of, 1) == hipSuccess);
    }

    // ---- the arithmetic through the host route ----
    for (int N : {3, 4, 20, 63, 64, 65, 257, ORBH_MAX_POINTS}) {
        const int I = 35, W = ORBH_WORDS(N);
        Scene s = make_scene(N, I, N < 40 ? 3 : N / 3, N % 2 ? 0.4 : 2.7);
        std::vector<int32_t> sets = make_sets(N, I);
        sets[1 * 3 + 2] = sets[1 * 3 + 1];                     // a repeated index
        sets[2 * 3 + 0] = N;                                   // an index outside
        sets[3 * 3 + 2] = -1;
        if (N == 257) {
            s.x1[5 * 3 + 1] = NAN;                             // NaN coordinates
            s.u2[9 * 2] = NAN;
            sets[0] = 5; sets[1] = 1; sets[2] = 2;
            s.x2[11 * 3 + 2] = 0.0f;                           // a point with z = 0
            s.u2[11 * 2] = INFINITY;
        }
        if (N == 65) {
            for (int k = 0; k < 9; k++) s.x2[k] = s.x1[k];     // equal triples
            sets[0] = 0; sets[1] = 1; sets[2] = 2;
        }
        std::vector<orbh_hyp> hyp(I);
        std::vector<uint64_t> fl((size_t)I * W, ~0ull);
        CHECK(orbh_hypotheses(&s.q, s.x1.data(), s.x2.data(), s.u1.data(), s.u2.data(), s.m1.data(), s.m2.data(), sets.data(), hyp.data(), fl.data(), 0) == ORBX_OK);
        int best = 0;
        for (int it = 0; it < I; it++) {
            int pop = 0;
            for (int w = 0; w < W; w++) pop += __builtin_popcountll(fl[(size_t)it * W + w]);
            CHECK(pop == hyp[it].count && hyp[it].count >= 0 && hyp[it].count <= N);
            if (N % 64) CHECK((fl[(size_t)it * W + W - 1] >> (N % 64)) == 0);            // zero bits past N
            if (it == 2 || it == 3) CHECK(std::isnan(hyp[it].s) && std::isnan(hyp[it].q[0]) && hyp[it].count == 0);
            else if (it > 3 && N > 3) best = hyp[it].count > best ? hyp[it].count : best;
        }
        if (N == 257) {
            CHECK(hyp[0].count == 0 && std::isnan(hyp[0].T12[0]));                       // a NaN correspondence in the set
            for (int it = 4; it < I; it++) CHECK(!((fl[(size_t)it * W] >> 5) & 1) && !((fl[(size_t)it * W] >> 9) & 1) && !((fl[(size_t)it * W] >> 11) & 1));
        }
        if (N == 65) CHECK(hyp[0].count == 0 && std::isnan(hyp[0].R[0]) && hyp[0].q[0] == 1.0 && hyp[0].q[1] == 0.0);
        if (N >= 63) {
            CHECK(best > N / 2);                               // three quarters are inliers: some hypothesis finds most of them
            CHECK(finite_block(hyp[4]));
        }

        // three calls of iterate over one state, the second and third continuing
        orbh_state state;
        std::memset(&state, 0, sizeof(state));
        std::vector<uint64_t> bf(W, 0), rf(W, 0);
        orbh_problem q = s.q;
        q.max_its = 12;
        q.iters = 5;
        int walked = 0;
        for (int call = 0; call < 3; call++) {
            orbh_result res;
            CHECK(orbh_iterate(&q, s.x1.data(), s.x2.data(), s.u1.data(), s.u2.data(), s.m1.data(), s.m2.data(), sets.data() + call * 15, &state, bf.data(),
                               &res, rf.data(), nullptr, nullptr, 0) == ORBX_OK);
            walked += res.found ? res.stop + 1 : res.stop;
            CHECK(state.iterations == walked && walked <= 12);
            CHECK(res.found == 0 || res.ninliers > q.min_inliers);
            CHECK(res.no_more == (!res.found && state.iterations >= 12));
            int pop = 0;
            for (int w = 0; w < W; w++) pop += __builtin_popcountll(rf[w]);
            CHECK(pop == res.ninliers);
        }
        // N below mRansacMinInliers: bNoMore at once, nothing walked
        q.min_inliers = N + 1;
        const int before = state.iterations;
        orbh_result res;
        CHECK(orbh_iterate(&q, s.x1.data(), s.x2.data(), s.u1.data(), s.u2.data(), s.m1.data(), s.m2.data(), sets.data(), &state, bf.data(), &res, rf.data(),
                           hyp.data(), fl.data(), 0) == ORBX_OK);
        CHECK(res.no_more == 1 && res.found == 0 && res.stop == 0 && state.iterations == before);
    }

    // ---- the batch form checks every solver before it computes any ----
    {
        Scene s = make_scene(30, 5, 10, 1.0);
        std::vector<int32_t> sets = make_sets(30, 5);
        orbh_problem qs[2] = {s.q, s.q};
        qs[1].n = 2;
        orbh_state states[2];
        std::memset(states, 0, sizeof(states));
        uint64_t bf[2] = {0, 0}, rf[2] = {0, 0};
        uint64_t *pbf[2] = {&bf[0], &bf[1]}, *prf[2] = {&rf[0], &rf[1]};
        const float *x1[2] = {s.x1.data(), s.x1.data()}, *x2[2] = {s.x2.data(), s.x2.data()}, *u1[2] = {s.u1.data(), s.u1.data()};
        const float *u2[2] = {s.u2.data(), s.u2.data()}, *m1[2] = {s.m1.data(), s.m1.data()}, *m2[2] = {s.m2.data(), s.m2.data()};
        const int32_t* st[2] = {sets.data(), sets.data()};
        orbh_result res[2];
        CHECK(orbh_iterate_batch(qs, 2, x1, x2, u1, u2, m1, m2, st, states, pbf, res, prf, nullptr, nullptr, 0) == ORBX_ERR_ARG);
        CHECK(states[0].iterations == 0);
        qs[1].n = 30;
        CHECK(orbh_iterate_batch(qs, 2, x1, x2, u1, u2, m1, m2, st, states, pbf, res, prf, nullptr, nullptr, 0) == ORBX_OK);
        CHECK(states[0].iterations == states[1].iterations && states[0].iterations > 0 && bf[0] == bf[1]);
    }
    std::printf("sim3solver host ok\n");
    return 0;
}
