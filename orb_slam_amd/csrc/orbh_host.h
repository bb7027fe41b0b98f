// The host side of the orbh_* calls in front of the launches: the argument checks, the table the kernels take by value and the packing of a
// solver's arrays into its point table.  Plain C++, so that tests/_probe/sim3solver_host.cpp and the host route run it without a GPU.
#pragma once
#include <stdint.h>
#include <cstring>
#include <initializer_list>

#include "orbh.h"

namespace orbh {

struct Problems { orbh_problem p[ORBH_MAX_PROBLEMS]; };

inline int check_problem(const orbh_problem& q) {
    if (q.n < 3 || q.n > ORBH_MAX_POINTS || q.iters < 1 || q.iters > ORBH_MAX_ITERS || q.min_inliers < 0 || q.max_its < 1) return ORBX_ERR_ARG;
    return ORBX_OK;
}

// the problems and caps of a batched call; on ORBX_OK PR holds the problems and iters the largest iteration count
inline int check_batch(const orbh_problem* problems, int nproblems, int ncap, int icap, Problems& PR, int& iters) {
    if (!problems || nproblems < 1 || nproblems > ORBH_MAX_PROBLEMS || ncap < 3 || ncap > ORBH_MAX_POINTS || icap < 1 || icap > ORBH_MAX_ITERS)
        return ORBX_ERR_ARG;
    std::memset(&PR, 0, sizeof(PR));
    iters = 0;
    for (int p = 0; p < nproblems; p++) {
        const orbh_problem& q = problems[p];
        if (check_problem(q) != ORBX_OK || q.n > ncap || q.iters > icap) return ORBX_ERR_ARG;
        PR.p[p] = q;
        if (q.iters > iters) iters = q.iters;
    }
    return ORBX_OK;
}

// true when none of the pointers is null
inline bool all_set(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!p) return false;
    return true;
}

// a carried state a call may start from
inline int check_state(const orbh_state& st) { return st.iterations < 0 || st.best_inliers < 0 ? ORBX_ERR_ARG : ORBX_OK; }

// one solver's arrays into its table of ORBH_POINT_ROWS rows of ncap floats (orbh.h); columns past n are left alone
inline void pack_points(int n, int ncap, const float* x3dc1, const float* x3dc2, const float* p1im1, const float* p2im2, const float* maxerr1,
                        const float* maxerr2, float* table) {
    for (int i = 0; i < n; i++) {
        for (int r = 0; r < 3; r++) {
            table[(size_t)r * ncap + i] = x3dc1[(size_t)i * 3 + r];
            table[(size_t)(3 + r) * ncap + i] = x3dc2[(size_t)i * 3 + r];
        }
        for (int r = 0; r < 2; r++) {
            table[(size_t)(6 + r) * ncap + i] = p1im1[(size_t)i * 2 + r];
            table[(size_t)(8 + r) * ncap + i] = p2im2[(size_t)i * 2 + r];
        }
        table[(size_t)10 * ncap + i] = maxerr1[i];
        table[(size_t)11 * ncap + i] = maxerr2[i];
    }
}

}  // namespace orbh
