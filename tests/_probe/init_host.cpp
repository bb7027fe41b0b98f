// The host side of the monocular initialisation (include/orbi.h) on the CPU against tests/_probe/hip_stub: the argument checks in front of the
// launches (orbi_host.h), the one-shot staging the host forms use (orbx::Staging), orbi::normalize and orbi::pose_from_rt, and the shared Jacobi
// header (orb_jacobi.h) run on the host.  With a file argument it reads matrices and the null vectors the test computed for them (text: one line
// "rows cols" then the rows x cols floats of A then the cols reference components, repeated) and prints, per size, the largest |got -+ ref| over the
// components: "jacobi <cols> <count> <discrepancy>".  tests/test_init_host.py builds this under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_host.h"
#include "orbi_host.h"
#include "orbi_math.h"

using namespace orbi;

#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {

template <int N>
void null_n(const float* A, int rows, float* v) {
    double S[N * N], V[N * N];
    for (int e = 0; e < N * N; e++) S[e] = orbj::gram_entry<N>(A, rows, e / N, e % N);
    orbj::sym_eig<N>(S, V);
    const int k = orbj::smallest_eigenvalue<N>(S);
    for (int i = 0; i < N; i++) v[i] = (float)V[i * N + k];
}

int jacobi_file(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    CHECK(f);
    double worst[10] = {0};
    int count[10] = {0};
    int rows, cols;
    while (std::fscanf(f, "%d %d", &rows, &cols) == 2) {
        CHECK(rows >= 1 && rows <= 16 && (cols == 3 || cols == 4 || cols == 9));
        std::vector<float> A((size_t)rows * cols);
        std::vector<double> ref(cols);
        for (float& a : A) CHECK(std::fscanf(f, "%f", &a) == 1);
        for (double& r : ref) CHECK(std::fscanf(f, "%lf", &r) == 1);
        float v[9];
        if (cols == 9) null_n<9>(A.data(), rows, v);
        else if (cols == 3) null_n<3>(A.data(), rows, v);
        else {
            CHECK(rows == 4);
            float A4[4][4], v4[4];
            for (int i = 0; i < 16; i++) A4[i / 4][i % 4] = A[i];
            orbj::null_vector(A4, v4);
            for (int i = 0; i < 4; i++) v[i] = v4[i];
            float vn[4];                                        // the register form and the memory form are one iteration
            null_n<4>(A.data(), 4, vn);
            for (int i = 0; i < 4; i++) CHECK(vn[i] == v4[i]);
        }
        double plus = 0, minus = 0;
        for (int i = 0; i < cols; i++) {
            plus = std::fmax(plus, std::fabs((double)v[i] - ref[i]));
            minus = std::fmax(minus, std::fabs((double)v[i] + ref[i]));
        }
        worst[cols] = std::fmax(worst[cols], std::fmin(plus, minus));
        count[cols]++;
    }
    std::fclose(f);
    for (int c : {3, 4, 9}) std::printf("jacobi %d %d %.9g\n", c, count[c], worst[c]);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<int32_t> ints(64, 7);
    std::vector<float> floats(64);
    const void* a = ints.data();
    const void* m16 = floats.data();                               // vector storage is 16-byte aligned
    {
        orbi_problem q = {};
        q.sigma = 1.0f; q.n1 = 100; q.n2 = 90; q.nmatches = 50; q.iters = 20;
        Problems PR;
        int iters = -1;
        auto models = [&](const orbi_problem* pr, int np, const void* ptr, int k1, int k2, int mc, int ic) {
            return check_models(pr, np, ptr, k1, ptr, k2, ptr, mc, ptr, ic, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, PR, iters);
        };
        CHECK(models(&q, 1, a, 100, 90, 50, 20) == ORBX_OK && iters == 20 && PR.p[0].nmatches == 50 && PR.p[1].nmatches == 0);
        CHECK(models(nullptr, 1, a, 100, 90, 50, 20) == ORBX_ERR_ARG && models(&q, 0, a, 100, 90, 50, 20) == ORBX_ERR_ARG);
        CHECK(models(&q, ORBI_MAX_PROBLEMS + 1, a, 100, 90, 50, 20) == ORBX_ERR_ARG && models(&q, 1, nullptr, 100, 90, 50, 20) == ORBX_ERR_ARG);
        CHECK(models(&q, 1, a, 99, 90, 50, 20) == ORBX_ERR_ARG && models(&q, 1, a, 100, 89, 50, 20) == ORBX_ERR_ARG);
        CHECK(models(&q, 1, a, 100, 90, 49, 20) == ORBX_ERR_ARG && models(&q, 1, a, 100, 90, 50, 19) == ORBX_ERR_ARG);
        CHECK(models(&q, 1, a, 100, 90, ORBI_MAX_MATCHES + 1, 20) == ORBX_ERR_ARG && models(&q, 1, a, 100, 90, 50, ORBI_MAX_ITERS + 1) == ORBX_ERR_ARG);
        for (int field = 0; field < 4; field++)
            for (int bad : {0, 7, 1 << 30}) {
                orbi_problem b = q;
                (field == 0 ? b.n1 : field == 1 ? b.n2 : field == 2 ? b.nmatches : b.iters) = bad;
                const bool fine = (field == 0 && bad == 7) || (field == 1 && bad == 7) || (field == 3 && bad == 7);       // only N has 8 as its floor
                CHECK((models(&b, 1, a, 100, 90, 50, 20) == ORBX_OK) == fine);
            }
        std::vector<orbi_problem> many(ORBI_MAX_PROBLEMS, q);
        many[5].iters = 33; many[31].nmatches = 8;
        CHECK(models(many.data(), ORBI_MAX_PROBLEMS, a, 100, 90, 50, 33) == ORBX_OK && iters == 33 && PR.p[31].nmatches == 8);
        many[31].nmatches = 51;
        CHECK(models(many.data(), ORBI_MAX_PROBLEMS, a, 100, 90, 50, 33) == ORBX_ERR_ARG);
    }
    {
        RtCounts C;
        const int32_t n1[2] = {100, 0}, n2[2] = {90, 90}, nm[2] = {50, 0};
        auto rt = [&](const void* ptr, int nh, int np, const int32_t* c1, const int32_t* c2, const int32_t* cm, int k1, int k2, int mc, const void* v) {
            return check_rt(ptr, nh, np, c1, c2, cm, ptr, k1, ptr, k2, ptr, mc, ptr, ptr, ptr, ptr, ptr, v, ptr, C);
        };
        CHECK(rt(a, 8, 2, n1, n2, nm, 100, 90, 50, m16) == ORBX_OK && C.n1[0] == 100 && C.n2[1] == 90 && C.nm[1] == 0 && C.nm[2] == 0);
        CHECK(rt(a, 8, 2, n1, n2, nm, 100, 90, 50, nullptr) == ORBX_OK);
        CHECK(rt(a, 8, 2, n1, n2, nm, 100, 90, 50, (const char*)m16 + 4) == ORBX_ERR_ARG);
        CHECK(rt(a, 0, 2, n1, n2, nm, 100, 90, 50, m16) == ORBX_ERR_ARG && rt(a, 9, 2, n1, n2, nm, 100, 90, 50, m16) == ORBX_ERR_ARG);
        CHECK(rt(a, 8, 0, n1, n2, nm, 100, 90, 50, m16) == ORBX_ERR_ARG && rt(nullptr, 8, 2, n1, n2, nm, 100, 90, 50, m16) == ORBX_ERR_ARG);
        CHECK(rt(a, 8, 2, nullptr, n2, nm, 100, 90, 50, m16) == ORBX_ERR_ARG && rt(a, 8, 2, n1, nullptr, nm, 100, 90, 50, m16) == ORBX_ERR_ARG);
        CHECK(rt(a, 8, 2, n1, n2, nullptr, 100, 90, 50, m16) == ORBX_ERR_ARG);
        CHECK(rt(a, 8, 2, n1, n2, nm, 99, 90, 50, m16) == ORBX_ERR_ARG && rt(a, 8, 2, n1, n2, nm, 100, 89, 50, m16) == ORBX_ERR_ARG);
        CHECK(rt(a, 8, 2, n1, n2, nm, 100, 90, 49, m16) == ORBX_ERR_ARG && rt(a, 8, 2, n1, n2, nm, 100, 90, ORBI_MAX_MATCHES + 1, m16) == ORBX_ERR_ARG);
    }
    {
        // the host forms' staging: inputs land where the slots say, outputs come back from theirs, nothing stays allocated
        orbx_keypoint kp[3] = {};
        kp[2].x = 5.0f;
        int32_t mt[4] = {1, 2, 3, 4};
        {
            orbx::Staging s;
            const auto k = s.in(kp, 3);
            const auto m = s.in(mt, 4);
            const auto o = s.out<float>(9);
            const auto none = s.out<uint8_t>(0);
            CHECK(s.alloc() == hipSuccess && hip_stub_live == 1);
            CHECK(s[k][2].x == 5.0f && s[m][3] == 4 && ((uint8_t*)s[o] - s.buf.as()) % 256 == 0 && s[none] != nullptr);
            for (int i = 0; i < 9; i++) s[o][i] = (float)i;
            float back[10] = {0};
            back[9] = -1.0f;
            CHECK(s.get(back, o, 9) == hipSuccess && back[8] == 8.0f && back[9] == -1.0f);
        }
        CHECK(hip_stub_live == 0);
        orbx::Staging fails;
        fails.in(kp, 3);
        hip_stub_fail = 1;
        CHECK(fails.alloc() != hipSuccess && hip_stub_live == 0);
    }
    {
        // Normalize on points whose sums are exact, and a pose whose products are exact
        orbx_keypoint kp[4] = {};
        const float xs[4] = {1, 3, 5, 7}, ys[4] = {10, 10, 30, 30};
        for (int i = 0; i < 4; i++) { kp[i].x = xs[i]; kp[i].y = ys[i]; }
        float out[4];
        normalize(kp, 4, out);
        CHECK(out[2] == 4.0f && out[3] == 20.0f && out[0] == 0.5f && out[1] == 0.1f);
        const float R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, t[3] = {1, 2, 4};
        orbi_pose P;
        pose_from_rt(2, 4, 8, 16, R, t, &P);
        const float P2[12] = {0, -2, 8, 34, 4, 0, 16, 72, 0, 0, 1, 4}, O2[3] = {-2, 1, -4};
        for (int i = 0; i < 12; i++) CHECK(P.P2[i] == P2[i]);
        for (int i = 0; i < 3; i++) CHECK(P.O2[i] == O2[i] && P.t[i] == t[i]);
        for (int i = 0; i < 9; i++) CHECK(P.R[i] == R[i]);
        // a point in front of both cameras, seen exactly: good; the same with the flag's pose mirrored: behind
        RtOut o;
        const float X[3] = {0.5f, -0.25f, 4.0f};
        const float Rz[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tz[3] = {-1, 0, 0};
        pose_from_rt(512, 512, 320, 240, Rz, tz, &P);
        check_rt_one(512, 512, 320, 240, P, 512 * X[0] / X[2] + 320, 512 * X[1] / X[2] + 240, 512 * (X[0] - 1) / X[2] + 320, 512 * X[1] / X[2] + 240, 4.0f, o);
        CHECK(o.status == ORBI_RT_GOOD && std::fabs(o.X[2] - 4.0f) < 1e-3f);
        float cosines[3] = {0.5f, 1.0f, 0.0f};
        CHECK(std::fabs(parallax_of(cosines, 3) - 0.0f) < 1e-6f && parallax_of(cosines, 0) == 0.0f);       // entry min(50, 2) of the sorted list is 1.0
    }
    if (argc > 1 && jacobi_file(argv[1]) != 0) return 1;
    std::printf("init host ok\n");
    return 0;
}
