// The host side of the orbe_* calls in front of the launches: the argument checks and the table the kernels take by value.  Plain C++, so that
// tests/_probe/pnp_host.cpp and the host route run it without a GPU.
#pragma once
#include <stdint.h>
#include <cstring>
#include <initializer_list>

#include "orbe.h"

namespace orbe {

struct Problems { orbe_problem p[ORBE_MAX_PROBLEMS]; };

inline int check_problem(const orbe_problem& q) {
    if (q.n < 4 || q.n > ORBE_MAX_POINTS || q.iters < 1 || q.iters > ORBE_MAX_ITERS || q.min_inliers < 4 || q.max_its < 1) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// the problems and caps of a batched call; on ORBX_OK PR holds the problems and iters the largest iteration count
inline int check_batch(const orbe_problem* problems, int nproblems, int ncap, int icap, Problems& PR, int& iters) {
    if (!problems || nproblems < 1 || nproblems > ORBE_MAX_PROBLEMS || ncap < 4 || ncap > ORBE_MAX_POINTS || icap < 1 || icap > ORBE_MAX_ITERS)
        return ORBX_ERR_ARG;
    std::memset(&PR, 0, sizeof(PR));
    iters = 0;
    for (int p = 0; p < nproblems; p++) {
        const orbe_problem& q = problems[p];
        if (check_problem(q) != ORBX_OK || q.n > ncap || q.iters > icap) return ORBX_ERR_ARG;
        PR.p[p] = q;
        if (q.iters > iters) iters = q.iters;
    }
    return ORBX_OK;
}

// true when none of the n pointers is null
inline bool all_set(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!p) return false;
    return true;
}

// a carried state a call may start from
inline int check_state(const orbe_state& st) { return st.iterations < 0 || st.best_inliers < 0 ? ORBX_ERR_ARG : ORBX_OK; }

}  // namespace orbe
