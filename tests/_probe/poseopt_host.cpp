// The host side of the pose optimisation (include/orbo.h) on the CPU against tests/_probe/hip_stub: the argument checks in front of the launch
// (orbo_host.h), the packing of a frame's arrays into its edge table, the one-shot staging the host forms use (orbx::Staging) with the layout of
// orbo_pose_batch, and the shared arithmetic (orbo_math.h) through the host route (tools/poseopt_host_route.cpp, compiled into this program): n from
// 0 to the limit, the lane and word edges, a NaN coordinate, a point with z = 0, a point behind the camera, every edge an outlier, and a batch
// against the single calls.  tests/test_poseopt_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx_host.h"
#include "../../tools/poseopt_host_route.cpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {

uint32_t lcg_state = 4321u;
double uniform() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (lcg_state >> 8) / 16777216.0;
}

struct Scene {
    std::vector<float> xyz, uv, w;
    orbo_problem q;
    float Tcw[12];
};

// a camera rotated about y and shifted; every fifth observation displaced; the start is the identity
Scene make_scene(int n, double displaced = 30.0) {
    Scene s;
    s.q = orbo_problem{517.3f, 516.5f, 318.6f, 255.3f, n};
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(s.Tcw, I, sizeof(I));
    const double c = std::cos(0.04), sn = std::sin(0.04), t[3] = {0.05, -0.04, 0.06};
    for (int i = 0; i < n; i++) {
        const float X = (float)(uniform() * 4 - 2), Y = (float)(uniform() * 3 - 1.5), Z = (float)(3 + uniform() * 5);
        const double x = c * X + sn * Z + t[0], y = Y + t[1], z = -sn * X + c * Z + t[2];
        double u = 517.3 * x / z + 318.6 + (uniform() - 0.5), v = 516.5 * y / z + 255.3 + (uniform() - 0.5);
        if (i % 5 == 4) { u += displaced; v -= displaced; }
        const float sigma2 = (float)std::pow(1.44, i % 8);
        s.xyz.insert(s.xyz.end(), {X, Y, Z});
        s.uv.insert(s.uv.end(), {(float)u, (float)v});
        s.w.push_back(1.0f / sigma2);
    }
    return s;
}

int popcount(const std::vector<uint64_t>& w) {
    int c = 0;
    for (uint64_t x : w) c += __builtin_popcountll(x);
    return c;
}

bool finite_result(const orbo_result& r) {
    bool ok = true;
    for (float v : r.Tcw) ok = ok && std::isfinite(v);
    for (double v : r.q) ok = ok && std::isfinite(v);
    for (double v : r.t) ok = ok && std::isfinite(v);
    return ok;
}

int run(const Scene& s, orbo_result& r, std::vector<uint64_t>& fl, std::vector<orbo_step>& tr) {
    fl.assign(ORBO_WORDS(s.q.n) + 1, 0xdeadbeefdeadbeefull);          // one word past the end must stay as it is
    tr.assign(ORBO_MAX_ITERS, orbo_step{});
    const int rc = orbo_pose(&s.q, s.xyz.data(), s.uv.data(), s.w.data(), s.Tcw, &r, fl.data(), tr.data(), 0);
    if (fl.back() != 0xdeadbeefdeadbeefull) return -100;
    fl.pop_back();
    return rc;
}

}  // namespace

int main() {
    // ---- argument checks ----
    const orbo_problem good = {500, 500, 320, 240, 60};
    CHECK(orbo::check_problem(good) == ORBX_OK);
    for (int k = 0; k < 2; k++) {
        orbo_problem b = good;
        b.n = k == 0 ? -1 : ORBO_MAX_EDGES + 1;
        CHECK(orbo::check_problem(b) == ORBX_ERR_ARG);
        orbo::Problems PR;
        CHECK(orbo::check_batch(&b, 1, ORBO_MAX_EDGES, PR) == ORBX_ERR_ARG);
    }
    {
        orbo::Problems PR;
        CHECK(orbo::check_batch(&good, 1, 60, PR) == ORBX_OK && PR.p[0].n == 60);
        CHECK(orbo::check_batch(&good, 1, 59, PR) == ORBX_ERR_ARG);                    // a cap below the problem's n
        CHECK(orbo::check_batch(&good, 0, 60, PR) == ORBX_ERR_ARG);
        CHECK(orbo::check_batch(&good, ORBO_MAX_PROBLEMS + 1, 60, PR) == ORBX_ERR_ARG);
        CHECK(orbo::check_batch(nullptr, 1, 60, PR) == ORBX_ERR_ARG);
        CHECK(orbo::check_batch(&good, 1, 0, PR) == ORBX_ERR_ARG);
        CHECK(orbo::check_batch(&good, 1, ORBO_MAX_EDGES + 1, PR) == ORBX_ERR_ARG);
        const orbo_problem empty = {500, 500, 320, 240, 0};
        CHECK(orbo::check_batch(&empty, 1, 1, PR) == ORBX_OK);
        float f = 0;
        uint64_t w = 0;
        CHECK(orbo::check_frame(empty, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
        CHECK(orbo::check_frame(good, &f, &f, nullptr, &w) == ORBX_ERR_ARG);
        orbo_result r;
        CHECK(orbo_pose(nullptr, &f, &f, &f, &f, &r, &w, nullptr, 0) == ORBX_ERR_ARG);
        CHECK(orbo_pose(&good, &f, &f, &f, nullptr, &r, &w, nullptr, 0) == ORBX_ERR_ARG);
        CHECK(orbo_pose(&good, &f, &f, &f, &f, nullptr, &w, nullptr, 0) == ORBX_ERR_ARG);
        CHECK(orbo_pose(&good, &f, &f, &f, &f, &r, nullptr, nullptr, 0) == ORBX_ERR_ARG);
    }
    // ---- the edge table and the staging layout of orbo_pose_batch ----
    {
        const Scene s = make_scene(70);
        const int cap = 130;
        std::vector<float> table((size_t)ORBO_EDGE_ROWS * cap, -1.0f);
        orbo::pack_edges(70, cap, s.xyz.data(), s.uv.data(), s.w.data(), table.data());
        CHECK(table[0 * cap + 69] == s.xyz[69 * 3] && table[2 * cap + 69] == s.xyz[69 * 3 + 2] && table[4 * cap + 69] == s.uv[69 * 2 + 1]);
        CHECK(table[5 * cap + 69] == s.w[69] && table[5 * cap + 70] == -1.0f && table[0 * cap + 70] == -1.0f);
        orbx::Staging st;
        const auto ie = st.in(table.data(), table.size());
        const auto it = st.in(s.Tcw, 12);
        const auto orr = st.out<orbo_result>(1);
        const auto of = st.out<uint64_t>(ORBO_WORDS(cap));
        const auto ot = st.out<orbo_step>(0);
        CHECK(st.alloc() == hipSuccess);
        CHECK(st[ie] && st[it] && st[orr] && st[of] && st[ot]);
        std::vector<float> back(table.size());
        CHECK(st.get(back.data(), ie, back.size()) == hipSuccess && back == table);
    }
    // ---- the arithmetic through the host route ----
    orbo_result r;
    std::vector<uint64_t> fl;
    std::vector<orbo_step> tr;
    for (int n : {0, 1, 8, 9, 10, 63, 64, 65, 127, 128, 129, 300, ORBO_MAX_EDGES}) {
        const Scene s = make_scene(n);
        CHECK(run(s, r, fl, tr) == ORBX_OK);
        CHECK(finite_result(r) && r.ninitial == n && r.noutlier == popcount(fl) && r.nbad == r.noutlier);
        CHECK(r.rounds == (n < 10 ? 1 : 4));
        CHECK(r.Tcw[12] == 0.0f && r.Tcw[13] == 0.0f && r.Tcw[14] == 0.0f && r.Tcw[15] == 1.0f);
        if (n >= 10) {
            CHECK(std::fabs(r.t[0] - 0.05) < 0.02 && std::fabs(r.t[1] + 0.04) < 0.02 && std::fabs(r.t[2] - 0.06) < 0.03);     // the planted pose
            for (int i = 0; i < n; i++) CHECK(((fl[i / 64] >> (i % 64)) & 1) == (uint64_t)(i % 5 == 4));                       // the displaced edges
            CHECK(r.iters[0] >= 1 && r.iters[0] <= 10 && r.iters[3] <= 5);
        }
        if (n == 0) CHECK(r.q[3] == 1.0 && r.t[0] == 0.0 && r.nbad == 0 && tr[0].status == 2 && tr[31].status == 2);
        if (n % 64) CHECK((fl.back() >> (n % 64)) == 0);                                                                       // zero bits past n
    }
    {   // a NaN coordinate and a point with z = 0: such an edge keeps its flag (clear), every trial is rejected on a NaN rho, and the estimate stays
        for (int k = 0; k < 2; k++) {
            Scene s = make_scene(40);
            if (k == 0) s.xyz[7 * 3 + 1] = NAN;
            else { s.xyz[7 * 3] = 0.0f; s.xyz[7 * 3 + 1] = 0.0f; s.xyz[7 * 3 + 2] = 0.0f; }
            CHECK(run(s, r, fl, tr) == ORBX_OK);
            CHECK(r.q[3] == 1.0 && r.t[0] == 0.0 && r.t[2] == 0.0);
            CHECK(((fl[0] >> 7) & 1) == 0 && r.iters[0] == 10 && tr[0].trials == 1 && tr[0].status == 0 && tr[9].status == 0);
        }
    }
    {   // a point behind the camera is an edge like any other
        Scene s = make_scene(40);
        s.xyz[11 * 3 + 2] = -3.0f;
        CHECK(run(s, r, fl, tr) == ORBX_OK);
        CHECK(finite_result(r) && ((fl[0] >> 11) & 1) == 1 && std::fabs(r.t[0] - 0.05) < 0.03);
    }
    {   // every edge an outlier after round 1: the later rounds iterate nothing
        Scene s = make_scene(20);
        for (int i = 0; i < 20; i++) { s.uv[i * 2] += (float)(150 + 100 * uniform()) * (i % 2 ? 1 : -1); s.uv[i * 2 + 1] -= (float)(150 + 100 * uniform()) * (i % 3 ? 1 : -1); }
        CHECK(run(s, r, fl, tr) == ORBX_OK);
        CHECK(finite_result(r) && r.rounds == 4 && r.nbad == 20 && r.iters[1] == 0 && r.iters[2] == 0 && r.iters[3] == 0 && tr[10].status == 2);
    }
    {   // a batch against the single calls
        const int ns[5] = {10, 65, 0, 130, 8};
        std::vector<Scene> ss;
        for (int n : ns) ss.push_back(make_scene(n));
        std::vector<orbo_problem> q;
        std::vector<const float*> xyz, uv, w;
        std::vector<float> T;
        std::vector<std::vector<uint64_t>> words(5);
        std::vector<uint64_t*> wp;
        for (int p = 0; p < 5; p++) {
            q.push_back(ss[p].q);
            xyz.push_back(ns[p] ? ss[p].xyz.data() : nullptr);
            uv.push_back(ns[p] ? ss[p].uv.data() : nullptr);
            w.push_back(ns[p] ? ss[p].w.data() : nullptr);
            T.insert(T.end(), ss[p].Tcw, ss[p].Tcw + 12);
            words[p].assign(ORBO_WORDS(ns[p]), 0);
            wp.push_back(ns[p] ? words[p].data() : nullptr);
        }
        std::vector<orbo_result> res(5);
        CHECK(orbo_pose_batch(q.data(), 5, xyz.data(), uv.data(), w.data(), T.data(), res.data(), wp.data(), nullptr, 0) == ORBX_OK);
        for (int p = 0; p < 5; p++) {
            CHECK(run(ss[p], r, fl, tr) == ORBX_OK);
            CHECK(std::memcmp(&r, &res[p], sizeof(r)) == 0 && fl == words[p]);
        }
        xyz[1] = nullptr;
        CHECK(orbo_pose_batch(q.data(), 5, xyz.data(), uv.data(), w.data(), T.data(), res.data(), wp.data(), nullptr, 0) == ORBX_ERR_ARG);
    }
    std::printf("poseopt host ok\n");
    return 0;
}
