// The host side of the orbo_* calls in front of the launch: the argument checks, the table the kernel takes by value and the packing of a
// frame's arrays into its edge table.  Plain C++, so that tests/_probe/poseopt_host.cpp and the host route run it without a GPU.
#pragma once
#include <stdint.h>
#include <cstring>
#include <initializer_list>

#include "orbo.h"

namespace orbo {

struct Problems { orbo_problem p[ORBO_MAX_PROBLEMS]; };

inline int check_problem(const orbo_problem& q) { return q.n < 0 || q.n > ORBO_MAX_EDGES ? ORBX_ERR_ARG : ORBX_OK; }

// the problems and the cap of a batched call; on ORBX_OK PR holds the problems
inline int check_batch(const orbo_problem* problems, int nproblems, int ncap, Problems& PR) {
    if (!problems || nproblems < 1 || nproblems > ORBO_MAX_PROBLEMS || ncap < 1 || ncap > ORBO_MAX_EDGES) return ORBX_ERR_ARG;
    std::memset(&PR, 0, sizeof(PR));
    for (int p = 0; p < nproblems; p++) {
        if (check_problem(problems[p]) != ORBX_OK || problems[p].n > ncap) return ORBX_ERR_ARG;
        PR.p[p] = problems[p];
    }
    return ORBX_OK;
}

// true when none of the pointers is null
inline bool all_set(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!p) return false;
    return true;
}

// the arrays of one frame of a host form: result and Tcw always, the edge arrays and the flag words when there are edges
inline int check_frame(const orbo_problem& q, const float* xyz, const float* uv, const float* inv_sigma2, const uint64_t* outlier) {
    if (check_problem(q) != ORBX_OK) return ORBX_ERR_ARG;
    return q.n > 0 && !all_set({xyz, uv, inv_sigma2, outlier}) ? ORBX_ERR_ARG : ORBX_OK;
}

// one frame's arrays into its table of ORBO_EDGE_ROWS rows of ncap floats (orbo.h); columns past n are left alone
inline void pack_edges(int n, int ncap, const float* xyz, const float* uv, const float* inv_sigma2, float* table) {
    for (int i = 0; i < n; i++) {
        for (int r = 0; r < 3; r++) table[(size_t)r * ncap + i] = xyz[(size_t)i * 3 + r];
        for (int r = 0; r < 2; r++) table[(size_t)(3 + r) * ncap + i] = uv[(size_t)i * 2 + r];
        table[(size_t)5 * ncap + i] = inv_sigma2[i];
    }
}

}  // namespace orbo
