// The host side of the orbg_* calls in front of the launch: the argument checks, the table the kernel takes by value and the packing of a
// candidate's arrays into its pair table.  Plain C++, so that tests/_probe/sim3opt_host.cpp and the host route run it without a GPU.
#pragma once
#include <stdint.h>
#include <cstring>

#include "orbg.h"
#include "orbo_host.h"

namespace orbg {

using orbo::all_set;

struct Problems { orbg_problem p[ORBG_MAX_PROBLEMS]; };

inline int check_problem(const orbg_problem& q) { return q.n < 0 || q.n > ORBG_MAX_PAIRS ? ORBX_ERR_ARG : ORBX_OK; }

// the problems and the cap of a batched call; on ORBX_OK PR holds the problems
inline int check_batch(const orbg_problem* problems, int nproblems, int ncap, Problems& PR) {
    if (!problems || nproblems < 1 || nproblems > ORBG_MAX_PROBLEMS || ncap < 1 || ncap > ORBG_MAX_PAIRS) return ORBX_ERR_ARG;
    std::memset(&PR, 0, sizeof(PR));
    for (int p = 0; p < nproblems; p++) {
        if (check_problem(problems[p]) != ORBX_OK || problems[p].n > ncap) return ORBX_ERR_ARG;
        PR.p[p] = problems[p];
    }
    return ORBX_OK;
}

// the arrays of one candidate of a host form: the pair arrays and the flag words when there are pairs
inline int check_candidate(const orbg_problem& q, const float* P1c, const float* P2c, const float* obs1, const float* obs2, const uint64_t* removed) {
    if (check_problem(q) != ORBX_OK) return ORBX_ERR_ARG;
    return q.n > 0 && !all_set({P1c, P2c, obs1, obs2, removed}) ? ORBX_ERR_ARG : ORBX_OK;
}

// one candidate's arrays into its table of ORBG_PAIR_ROWS rows of ncap floats (orbg.h); columns past n are left alone
inline void pack_pairs(int n, int ncap, const float* P1c, const float* P2c, const float* obs1, const float* obs2, float* table) {
    const float* src[4] = {P1c, P2c, obs1, obs2};
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 4; a++)
            for (int r = 0; r < 3; r++) table[(size_t)(a * 3 + r) * ncap + i] = src[a][(size_t)i * 3 + r];
}

}  // namespace orbg
