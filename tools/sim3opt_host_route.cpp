// The host route tools/bench_sim3opt.py measures the device Sim3 refinement against: the host forms of include/orbg.h on one host core over the
// same arithmetic text (orb_slam_amd/csrc/orbg_math.h), the same summation order (64 lane sums and the xor butterfly, walked serially) and the same
// argument checks (orbg_host.h).  tests/test_sim3opt_host.py holds it against the numpy restatement; code written against the library links
// against this file instead and runs on the host.  `device` is ignored.  Build with -ffp-contract=off.
#include <cstring>
#include <vector>

#include "orbg_host.h"
#include "orbg_math.h"

namespace {

using namespace orbg;

struct HostLoad {
    const float *P1, *P2, *o1, *o2;
    Pair operator()(int i) const {
        const size_t k = (size_t)i * 3;
        return {{(double)P1[k], (double)P1[k + 1], (double)P1[k + 2]}, {(double)P2[k], (double)P2[k + 1], (double)P2[k + 2]},
                (double)o1[k], (double)o1[k + 1], (double)o1[k + 2], (double)o2[k], (double)o2[k + 1], (double)o2[k + 2]};
    }
};

// The butterfly as lane 0 sees it (tools/poseopt_host_route.cpp)
inline double butterfly(double (&v)[LANES]) {
    for (int d = 32; d >= 1; d >>= 1)
        for (int l = 0; l < d; l++) v[l] = v[l] + v[l + d];
    return v[0];
}

struct HostJac {
    double J[2 * DIM];
    void put(int k, double v) { J[k] = v; }
    double get(int k) const { return J[k]; }
};

struct HostSys {
    HostLoad load;
    Cam c1, c2;
    double delta, dsqr, th2;
    int n;
    Flags f[LANES];
    uint64_t* out;
    orbo_step* tr;
    Sim3 sims[2 * NSIM];
    void linearise(const Sim3& S) {
        for (int k = 0; k < NSIM; k++) {
            perturbed(S, k, sims[k]);
            sim3_inverse(sims[k], sims[NSIM + k]);
        }
    }
    void full(double (&acc)[NACC]) {
        static thread_local double part[NACC][LANES];
        HostJac jb;
        for (int l = 0; l < LANES; l++) {
            double a[NACC];
            lane_full(load, sims, c1, c2, delta, dsqr, n, l, f[l], jb, a);
            for (int k = 0; k < NACC; k++) part[k][l] = a[k];
        }
        for (int k = 0; k < NACC; k++) acc[k] = butterfly(part[k]);
    }
    double chi(const Sim3& S, const Sim3& Si) {
        double part[LANES];
        for (int l = 0; l < LANES; l++) part[l] = lane_chi(load, S, Si, c1, c2, delta, dsqr, n, l, f[l]);
        return butterfly(part);
    }
    int check(const Sim3& last, const Sim3& lasti, bool first) {
        int nbad = 0;
        if (n) std::memset(out, 0, ORBO_WORDS(n) * sizeof(uint64_t));
        for (int i = 0; i < n; i++) {
            const int l = i % LANES, k = i / LANES;
            const bool removed = f[l].get(k);
            const bool bad = !removed && pair_is_bad(load, last, lasti, c1, c2, th2, i);
            if (first && bad) f[l].set(k, true);
            if (removed || bad) out[k] |= (uint64_t)1 << l;
            nbad += bad;
        }
        return nbad;
    }
    double u(double v) const { return v; }
    void step(int slot, const orbo_step& s) {
        if (tr) tr[slot] = s;
    }
};

}  // namespace

extern "C" {

int orbg_sim3(const orbg_problem* problem, const float* P1c, const float* P2c, const float* obs1, const float* obs2, const float* S12,
              orbg_result* result, uint64_t* removed, orbo_step* trace, int) {
    if (!problem || !result || !S12 || check_candidate(*problem, P1c, P2c, obs1, obs2, removed) != ORBX_OK) return ORBX_ERR_ARG;
    HostSys sys;
    sys.load = {P1c, P2c, obs1, obs2};
    sys.c1 = {(double)problem->fx1, (double)problem->fy1, (double)problem->cx1, (double)problem->cy1};
    sys.c2 = {(double)problem->fx2, (double)problem->fy2, (double)problem->cx2, (double)problem->cy2};
    sys.th2 = (double)problem->th2;
    sys.delta = (double)(float)sqrt((double)problem->th2);
    sys.dsqr = (double)(float)(sys.delta * sys.delta);
    sys.n = problem->n;
    sys.out = removed;
    sys.tr = trace;
    std::memset(sys.sims, 0, sizeof(sys.sims));
    std::memset(result, 0, sizeof(*result));
    optimize_sim3(sys, problem->n, S12, *result);
    return ORBX_OK;
}

int orbg_sim3_batch(const orbg_problem* problems, int nproblems, const float* const* P1c, const float* const* P2c, const float* const* obs1,
                    const float* const* obs2, const float* S12, orbg_result* results, uint64_t* const* removed, orbo_step* const* trace, int) {
    if (!problems || nproblems < 1 || nproblems > ORBG_MAX_PROBLEMS || !all_set({P1c, P2c, obs1, obs2, S12, results, removed})) return ORBX_ERR_ARG;
    for (int p = 0; p < nproblems; p++)
        if (check_candidate(problems[p], P1c[p], P2c[p], obs1[p], obs2[p], removed[p]) != ORBX_OK) return ORBX_ERR_ARG;
    for (int p = 0; p < nproblems; p++) {
        const int rc = orbg_sim3(problems + p, P1c[p], P2c[p], obs1[p], obs2[p], S12 + (size_t)p * 13, results + p, removed[p], trace ? trace[p] : nullptr, 0);
        if (rc != ORBX_OK) return rc;
    }
    return ORBX_OK;
}

}  // extern "C"
