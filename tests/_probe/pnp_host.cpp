// The host side of the EPnP RANSAC (include/orbe.h) on the CPU against tests/_probe/hip_stub: the argument checks in front of the launches
// (orbe_host.h), the one-shot staging the host forms use (orbx::Staging) with the layouts of orbe_iterate, and the shared arithmetic (orbe_math.h
// over orb_jacobi.h) through the host route (tools/pnp_host_route.cpp, compiled into this program): a scene with outliers, sets with repeated and
// outside indices, NaN coordinates, the largest N, planted flag arrays of every size class and three calls of iterate over one state.
// tests/test_pnp_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_host.h"
#include "../../tools/pnp_host_route.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {

uint32_t lcg_state = 12345u;
double uniform() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (lcg_state >> 8) / 16777216.0;
}

struct Scene {
    std::vector<float> p3d, p2d, maxerr;
    orbe_problem q;
};

// points in front of a camera at a small rotation, every fourth correspondence an outlier
Scene make_scene(int N, int iters, int min_inliers) {
    Scene s;
    s.q = orbe_problem{500.0f, 510.0f, 320.0f, 240.0f, N, iters, min_inliers, iters};
    const double c = std::cos(0.2), sn = std::sin(0.2), t[3] = {0.1, -0.2, 0.3};
    for (int i = 0; i < N; i++) {
        const double X = uniform() * 4 - 2, Y = uniform() * 3 - 1.5, Z = 3 + uniform() * 5;
        const double xc = c * X + sn * Z + t[0], yc = Y + t[1], zc = -sn * X + c * Z + t[2];
        double u = 320 + 500 * xc / zc, v = 240 + 510 * yc / zc;
        if (i % 4 == 3) { u = uniform() * 640; v = uniform() * 480; }
        s.p3d.insert(s.p3d.end(), {(float)X, (float)Y, (float)Z});
        s.p2d.insert(s.p2d.end(), {(float)(u + uniform() - 0.5), (float)(v + uniform() - 0.5)});
        s.maxerr.push_back(5.991f);
    }
    return s;
}

std::vector<int32_t> make_sets(int N, int iters) {
    std::vector<int32_t> sets((size_t)iters * 4);
    for (int32_t& x : sets) x = (int32_t)(uniform() * N) % N;
    return sets;
}

}  // namespace

int main() {
    // ---- argument checks ----
    orbe_problem good = {500, 500, 320, 240, 60, 35, 10, 35};
    CHECK(orbe::check_problem(good) == ORBX_OK);
    for (int k = 0; k < 6; k++) {
        orbe_problem b = good;
        if (k == 0) b.n = 3;
        if (k == 1) b.n = ORBE_MAX_POINTS + 1;
        if (k == 2) b.iters = 0;
        if (k == 3) b.iters = ORBE_MAX_ITERS + 1;
        if (k == 4) b.min_inliers = 3;
        if (k == 5) b.max_its = 0;
        CHECK(orbe::check_problem(b) == ORBX_ERR_ARG);
    }
    orbe::Problems PR;
    int iters = -1;
    orbe_problem two[2] = {good, good};
    two[1].iters = 7;
    CHECK(orbe::check_batch(two, 2, 60, 35, PR, iters) == ORBX_OK && iters == 35 && PR.p[1].iters == 7);
    CHECK(orbe::check_batch(two, 2, 59, 35, PR, iters) == ORBX_ERR_ARG);
    CHECK(orbe::check_batch(two, 2, 60, 34, PR, iters) == ORBX_ERR_ARG);
    CHECK(orbe::check_batch(two, 0, 60, 35, PR, iters) == ORBX_ERR_ARG);
    CHECK(orbe::check_batch(two, ORBE_MAX_PROBLEMS + 1, 60, 35, PR, iters) == ORBX_ERR_ARG);
    CHECK(orbe::check_batch(nullptr, 1, 60, 35, PR, iters) == ORBX_ERR_ARG);
    CHECK(orbe::check_batch(two, 2, ORBE_MAX_POINTS + 1, 35, PR, iters) == ORBX_ERR_ARG);
    CHECK(orbe::check_batch(two, 2, 60, ORBE_MAX_ITERS + 1, PR, iters) == ORBX_ERR_ARG);
    int dummy = 0;
    CHECK(orbe::all_set({&dummy, &dummy}) && !orbe::all_set({&dummy, nullptr}));
    orbe_state st0 = {};
    CHECK(orbe::check_state(st0) == ORBX_OK);
    st0.best_inliers = -1;
    CHECK(orbe::check_state(st0) == ORBX_ERR_ARG);
    {
        int32_t mi = 0, mx = 0;
        float eps = 0, me[3], s2[3] = {1.0f, 1.44f, 2.0736f};
        CHECK(orbe_ransac_parameters(0, 0.99, 10, 300, 4, 0.5f, 5.991f, s2, &mi, &mx, &eps, me) == ORBX_ERR_ARG);
        CHECK(orbe_ransac_parameters(3, 0.99, 10, 300, 4, 0.5f, 5.991f, nullptr, &mi, &mx, &eps, me) == ORBX_ERR_ARG);
        CHECK(orbe_ransac_parameters(3, 0.99, 10, 300, 4, 0.5f, 5.991f, s2, &mi, &mx, &eps, me) == ORBX_OK);
        CHECK(mi == 10 && mx == 1 && me[1] == 1.44f * 5.991f);                     // N < minInliers: epsilon > 1, log of a negative number, one iteration
        CHECK(orbe_ransac_parameters(3, 1.0, 1, 300, 1, 1e-30f, 5.991f, s2, &mi, &mx, &eps, me) == ORBX_OK && mx >= 1 && mx <= 300);
    }

    // ---- the staging of orbe_iterate: every slot inside the block, the inputs where they were put ----
    {
        const size_t N = 100, I = 35;
        std::vector<float> a(N * 3, 1.5f);
        std::vector<int32_t> sets(I * 4, 7);
        orbx::Staging s;
        const auto a3 = s.in(a.data(), N * 3);
        const auto st = s.in(sets.data(), I * 4);
        const auto oR = s.out<double>(I * 9);
        const auto of = s.out<uint8_t>(I * N);
        const auto orr = s.out<orbe_result>(1);
        CHECK(s.alloc() == hipSuccess);
        CHECK(s[a3][N * 3 - 1] == 1.5f && s[st][I * 4 - 1] == 7);
        CHECK(((uintptr_t)s[oR] & 7) == 0 && ((uintptr_t)s[orr] & 3) == 0);
        s[oR][I * 9 - 1] = 2.0;
        s[of][I * N - 1] = 9;
        double back = 0;
        CHECK(s.get(&back, oR, 1) == hipSuccess);
    }

    // ---- the arithmetic through the host route ----
    for (int N : {4, 10, 65, 300, ORBE_MAX_POINTS}) {
        const int I = N == ORBE_MAX_POINTS ? 3 : 35;
        Scene s = make_scene(N, I, N < 20 ? 4 : N / 3);
        std::vector<int32_t> sets = make_sets(N, I);
        sets[1 * 4 + 2] = sets[1 * 4 + 1];                     // a repeated index
        if (I > 4) {
            sets[2 * 4 + 0] = N;                               // an index outside
            sets[3 * 4 + 3] = -1;
        }
        if (N == 300) {
            s.p3d[5 * 3 + 1] = NAN;
            s.p2d[9 * 2] = NAN;
            sets[4 * 4] = 5;
            sets[5 * 4] = 9;
        }
        const int C = I > 6 ? I : 6;                           // the planted arrays below take six slots
        std::vector<double> R(C * 9), t(C * 3), err(C * 3), vecs(C * 48), rR(C * 9, -7.0), rt(C * 3, -7.0);
        std::vector<int32_t> branch(C), count(C), rcount(C, -7), rok(C, -7);
        std::vector<uint8_t> flags((size_t)C * N), rflags((size_t)C * N, 7);
        CHECK(orbe_hypotheses(&s.q, s.p3d.data(), s.p2d.data(), s.maxerr.data(), sets.data(), R.data(), t.data(), err.data(), branch.data(), vecs.data(),
                              count.data(), flags.data(), 0) == ORBX_OK);
        CHECK(orbe_hypotheses(&s.q, s.p3d.data(), nullptr, s.maxerr.data(), sets.data(), R.data(), t.data(), err.data(), branch.data(), vecs.data(),
                              count.data(), flags.data(), 0) == ORBX_ERR_ARG);
        if (I > 4) CHECK(std::isnan(R[2 * 9]) && count[2] == 0 && branch[2] == 0 && std::isnan(R[3 * 9 + 8]) && count[3] == 0);
        for (int it = 0; it < I; it++) CHECK(count[it] >= 0 && count[it] <= N && branch[it] >= 0 && branch[it] <= 3);
        CHECK(orbe_refine(&s.q, s.p3d.data(), s.p2d.data(), s.maxerr.data(), count.data(), flags.data(), 0, rR.data(), rt.data(), rcount.data(), rflags.data(),
                          rok.data(), 0) == ORBX_OK);
        int records = 0;
        for (int it = 0; it < I; it++) {
            const bool rec = orbe::is_record(count.data(), it, s.q.min_inliers, 0);
            records += rec;
            CHECK(rec ? (rcount[it] >= 0 && rok[it] == (rcount[it] > s.q.min_inliers)) : (rcount[it] == -7 && rok[it] == -7 && rR[it * 9] == -7.0));
        }
        std::printf("N %d: %d records\n", N, records);
        // three calls over one state
        orbe_state state = {};
        std::vector<uint8_t> bf(N), rf(N), out(N);
        orbe_result res;
        for (int call = 0; call < 3; call++) {
            CHECK(orbe_iterate(&s.q, s.p3d.data(), s.p2d.data(), s.maxerr.data(), sets.data(), &state, bf.data(), rf.data(), &res, out.data(), 0) == ORBX_OK);
            CHECK(res.kind >= ORBE_KIND_NONE && res.kind <= ORBE_KIND_REFINED && res.stop >= 0 && res.stop <= I && res.ninliers >= 0 && res.ninliers <= N);
            CHECK(state.iterations == (call + 1) * I || res.kind == ORBE_KIND_REFINED);
        }
        // planted flag arrays: fewer than four, five, around the 64 partial sums, all
        const int counts[6] = {3, 5, 63, 64, 65, N};
        orbe_problem q6 = s.q;
        q6.iters = 6;
        std::vector<uint8_t> fin((size_t)6 * N, 0);
        for (int k = 0; k < 6; k++)
            for (int i = 0, have = 0; i < N && have < counts[k]; i++)
                if (i % 4 != 3 || counts[k] == N) { fin[(size_t)k * N + i] = 1; have++; }
        CHECK(orbe_refit(&q6, s.p3d.data(), s.p2d.data(), s.maxerr.data(), fin.data(), rR.data(), rt.data(), vecs.data(), rcount.data(), rflags.data(), rok.data(),
                         0) == ORBX_OK);
        CHECK(std::isnan(rR[0]) && rcount[0] == 0 && rok[0] == 0);
    }
    std::printf("pnp host ok\n");
    return 0;
}
