// The host side of the bundle adjustment (include/orbb.h) on the CPU: the argument checks (orbb_host.h), the layout of the work buffer, the state
// helpers and the shared arithmetic (orbb_math.h) through the host route (tools/localba_host_route.cpp, compiled into this program): scenes from one
// free pose to seventeen, a point with one edge, a point without edges, a pose without edges, no edges at all, no iterations, a NaN coordinate, a
// point on a camera's plane z = 0, every edge inactive, and the two-phase run.  tests/test_localba_host.py builds this under AddressSanitizer +
// UndefinedBehaviorSanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../tools/localba_host_route.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {

uint32_t lcg_state = 9876u;
double uniform() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (lcg_state >> 8) / 16777216.0;
}

struct Scene {
    orbb_problem q;
    std::vector<float> cam, uv, w, Tcw, world;
    std::vector<int32_t> first, pose;
    std::vector<double> qt, xyz, chi2;
    std::vector<uint64_t> active, flags;
};

// cameras side by side looking down z, points 3 to 7 m away; point j is seen by the poses p with (j + p) % skip != 0
Scene make_scene(int nfree, int nfixed, int npoints, int skip, double noise = 0.5) {
    Scene s;
    const int np = nfree + nfixed;
    s.first.push_back(0);
    for (int p = 0; p < np; p++) {
        s.cam.insert(s.cam.end(), {517.3f, 516.5f, 318.6f, 255.3f});
        const float off = p < nfree ? 0.03f : 0.0f;
        const float T[12] = {1, 0, 0, -0.3f * p + off, 0, 1, 0, off, 0, 0, 1, -off};
        s.Tcw.insert(s.Tcw.end(), T, T + 12);
    }
    for (int j = 0; j < npoints; j++) {
        const double X = uniform() * 3 - 1.5, Y = uniform() * 2 - 1, Z = 3 + uniform() * 4;
        s.world.insert(s.world.end(), {(float)(X + 0.02), (float)(Y - 0.02), (float)(Z + 0.03)});
        for (int p = 0; p < np; p++) {
            if (skip && (j + p) % skip == 0) continue;
            const double x = X - 0.3 * p, u = 517.3 * x / Z + 318.6 + noise * (uniform() - 0.5), v = 516.5 * Y / Z + 255.3 + noise * (uniform() - 0.5);
            s.pose.push_back(p);
            s.uv.insert(s.uv.end(), {(float)u, (float)v});
            s.w.push_back(1.0f / (float)std::pow(1.44, (j + p) % 8));
        }
        s.first.push_back((int32_t)s.pose.size());
    }
    s.q = orbb_problem{nfree, nfixed, npoints, (int32_t)s.pose.size()};
    s.qt.assign((size_t)np * 7, 0.0);
    s.xyz.assign((size_t)npoints * 3 + 1, 0.0);
    s.chi2.assign(s.pose.size() + 1, -7.0);                               // one past the end must stay as it is
    s.active.assign(ORBB_WORDS(s.q.nedges) + 1, ~(uint64_t)0);
    s.flags.assign(ORBB_WORDS(s.q.nedges) + 1, 0xdeadbeefdeadbeefull);
    return s;
}

int start(Scene& s) { return orbb_state_from_float(&s.q, s.Tcw.data(), s.world.data(), s.qt.data(), s.xyz.data()); }

int run(Scene& s, int iters, orbb_result& r, std::vector<orbo_step>* trace = nullptr, std::vector<double>* dump = nullptr) {
    if (trace) trace->assign(ORBB_MAX_ITERS, orbo_step{});
    if (dump) dump->assign(ORBB_DUMP_DOUBLES(s.q.nfree, s.q.npoints), -1.0);
    const int rc = orbb_optimize(&s.q, s.cam.data(), s.first.data(), s.pose.data(), s.uv.data(), s.w.data(), (float)std::sqrt(5.991), s.qt.data(), s.xyz.data(),
                                 s.active.data(), s.chi2.data(), iters, &r, s.flags.data(), trace ? trace->data() : nullptr, dump ? dump->data() : nullptr, 0);
    if (s.flags.back() != 0xdeadbeefdeadbeefull || s.chi2.back() != -7.0) return -100;
    return rc;
}

bool finite_state(const Scene& s) {
    bool ok = true;
    for (double v : s.qt) ok = ok && std::isfinite(v);
    for (double v : s.xyz) ok = ok && std::isfinite(v);
    return ok;
}

int flagged(const Scene& s) {
    int c = 0;
    for (int e = 0; e < s.q.nedges; e++) c += (int)((s.flags[e >> 6] >> (e & 63)) & 1);
    return c;
}

}  // namespace

int main() {
    orbb_result r;
    // shapes: one free pose up to seventeen, with and without fixed poses behind them
    const int shapes[][4] = {{1, 1, 8, 0}, {2, 1, 12, 0}, {5, 3, 70, 3}, {17, 2, 40, 4}, {3, 2, 130, 2}};
    for (const auto& sh : shapes) {
        Scene s = make_scene(sh[0], sh[1], sh[2], sh[3]);
        CHECK(start(s) == ORBX_OK);
        CHECK(orbb_work_bytes(&s.q) > 0 && orbb_work_bytes(&s.q) % 256 == 0);
        std::vector<orbo_step> tr;
        std::vector<double> dump;
        CHECK(run(s, 5, r, &tr, &dump) == ORBX_OK);
        CHECK(r.iters >= 1 && r.iters <= 5 && r.chi_last <= r.chi_first && std::isfinite(r.chi_last) && r.lambda > 0 && finite_state(s));
        for (double v : dump) CHECK(std::isfinite(v) && v != -1.0);
        for (int i = r.iters; i < ORBB_MAX_ITERS; i++) CHECK(tr[i].status == 2);
        // the second phase on the same state, flagged edges out
        for (size_t w = 0; w + 1 < s.active.size(); w++) s.active[w] &= ~s.flags[w];
        const double before = r.chi_last;
        CHECK(run(s, 10, r) == ORBX_OK);
        CHECK(r.chi_first <= before * (1 + 1e-9) && r.chi_last <= r.chi_first && finite_state(s));
        // the float outputs
        std::vector<float> T((size_t)(sh[0] + sh[1]) * 16), X((size_t)sh[2] * 3);
        CHECK(orbb_state_to_float(&s.q, s.qt.data(), s.xyz.data(), T.data(), X.data()) == ORBX_OK);
        CHECK(T[15] == 1.0f && T[12] == 0.0f);
    }
    {   // a point with one edge, a point without edges and a free pose without edges
        Scene s = make_scene(3, 2, 20, 0);
        std::vector<int32_t> first{0}, pose;
        std::vector<float> uv, w;
        for (int j = 0; j < 20; j++) {
            for (int e = s.first[j]; e < s.first[j + 1]; e++) {
                const int p = s.pose[e];
                if (p == 2 || (j == 4 && p != 0) || j == 9) continue;
                pose.push_back(p);
                uv.insert(uv.end(), {s.uv[e * 2], s.uv[e * 2 + 1]});
                w.push_back(s.w[e]);
            }
            first.push_back((int32_t)pose.size());
        }
        s.first = first; s.pose = pose; s.uv = uv; s.w = w;
        s.q.nedges = (int32_t)pose.size();
        s.chi2.assign(pose.size() + 1, -7.0);
        s.active.assign(ORBB_WORDS(s.q.nedges) + 1, ~(uint64_t)0);
        s.flags.assign(ORBB_WORDS(s.q.nedges) + 1, 0xdeadbeefdeadbeefull);
        CHECK(start(s) == ORBX_OK);
        const std::vector<double> q0 = s.qt, x0 = s.xyz;
        CHECK(run(s, 5, r) == ORBX_OK);
        CHECK(r.iters >= 1 && finite_state(s) && r.chi_last < r.chi_first);
        CHECK(std::memcmp(&s.qt[2 * 7], &q0[2 * 7], 7 * sizeof(double)) == 0);          // the pose without edges
        CHECK(std::memcmp(&s.xyz[9 * 3], &x0[9 * 3], 3 * sizeof(double)) == 0);         // the point without edges
        CHECK(std::memcmp(&s.xyz[4 * 3], &x0[4 * 3], 3 * sizeof(double)) != 0);         // the one-edge point moves
    }
    {   // no edges at all; no iterations; every edge inactive
        Scene s = make_scene(2, 1, 6, 1);
        CHECK(s.q.nedges == 0 && start(s) == ORBX_OK);
        const std::vector<double> q0 = s.qt;
        CHECK(run(s, 5, r) == ORBX_OK && r.status == ORBB_RUN_NOTHING && r.iters == 0 && s.qt == q0);
        Scene t = make_scene(2, 1, 10, 0);
        CHECK(start(t) == ORBX_OK);
        const std::vector<double> t0 = t.qt;
        CHECK(run(t, 0, r) == ORBX_OK && r.status == ORBB_RUN_NOTHING && t.qt == t0 && t.chi2[0] >= 0 && r.chi_first > 0);
        std::fill(t.active.begin(), t.active.end(), 0);
        std::fill(t.chi2.begin(), t.chi2.end() - 1, 3.0);
        CHECK(run(t, 5, r) == ORBX_OK && r.status == ORBB_RUN_NOTHING && t.qt == t0 && t.chi2[0] == 3.0 && flagged(t) == 0);
    }
    {   // a NaN coordinate: the sums are NaN, every solve fails, the state stays; a point on a camera's plane z = 0
        Scene s = make_scene(2, 1, 10, 0);
        CHECK(start(s) == ORBX_OK);
        s.xyz[3] = std::nan("");
        const std::vector<double> q0 = s.qt;
        CHECK(run(s, 3, r) == ORBX_OK);
        CHECK(r.iters == 3 && r.status == ORBB_RUN_OK && std::memcmp(s.qt.data(), q0.data(), q0.size() * sizeof(double)) == 0);    // one rejected trial each
        Scene z = make_scene(2, 1, 10, 0);
        CHECK(start(z) == ORBX_OK);
        z.xyz[2] = 0.0;                                                   // the fixed pose has t.z = 0
        CHECK(run(z, 3, r) == ORBX_OK);
    }
    {   // the argument checks
        Scene s = make_scene(2, 1, 10, 0);
        CHECK(start(s) == ORBX_OK);
        orbb_problem bad = s.q;
        bad.nfree = 0;
        CHECK(orbb_work_bytes(&bad) == 0 && orbb_state_from_float(&bad, s.Tcw.data(), s.world.data(), s.qt.data(), s.xyz.data()) == ORBX_ERR_ARG);
        bad = s.q;
        bad.nfree = ORBB_MAX_FREE + 1;
        CHECK(orbb_work_bytes(&bad) == 0);
        s.pose[2] = 3;
        CHECK(run(s, 5, r) == ORBX_ERR_ARG);
        s.pose[2] = s.pose[1];
        CHECK(run(s, 5, r) == ORBX_ERR_ARG);
    }
    std::printf("localba host ok\n");
    return 0;
}
