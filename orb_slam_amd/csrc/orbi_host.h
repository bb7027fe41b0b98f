// The host side of orbi_models* / orbi_check_rt* in front of the launches: the argument checks and the tables the kernels take by value.  Plain
// C++, so that tests/_probe/init_host.cpp runs it without a GPU.
#pragma once
#include <stdint.h>
#include <cstring>

#include "orbi.h"

namespace orbi {

// the kernels' by-value tables: the problems of orbi_models*, the counts of orbi_check_rt*
struct Problems { orbi_problem p[ORBI_MAX_PROBLEMS]; };
struct RtCounts { int32_t n1[ORBI_MAX_PROBLEMS], n2[ORBI_MAX_PROBLEMS], nm[ORBI_MAX_PROBLEMS]; };

inline int check_problem(const orbi_problem& q) {
    if (q.n1 < 1 || q.n1 > ORBF_MAX_FEATURES || q.n2 < 1 || q.n2 > ORBF_MAX_FEATURES || q.nmatches < 8 || q.nmatches > ORBI_MAX_MATCHES || q.iters < 1 ||
        q.iters > ORBI_MAX_ITERS)
        return ORBX_ERR_ARG;
    return ORBX_OK;
}

// orbi_models_batch_device's arguments; on ORBX_OK PR holds the problems and iters the largest iteration count
inline int check_models(const orbi_problem* problems, int nproblems, const void* d_kps1, int kcap1, const void* d_kps2, int kcap2, const void* d_matches,
                        int mcap, const void* d_sets, int icap, const void* d_scoreH, const void* d_scoreF, const void* d_H21, const void* d_H12,
                        const void* d_F21, const void* d_best, const void* d_S, const void* d_inlH, const void* d_inlF, Problems& PR, int& iters) {
    if (!problems || nproblems < 1 || nproblems > ORBI_MAX_PROBLEMS || kcap1 < 1 || kcap1 > ORBF_MAX_FEATURES || kcap2 < 1 || kcap2 > ORBF_MAX_FEATURES ||
        mcap < 8 || mcap > ORBI_MAX_MATCHES || icap < 1 || icap > ORBI_MAX_ITERS)
        return ORBX_ERR_ARG;
    if (!d_kps1 || !d_kps2 || !d_matches || !d_sets || !d_scoreH || !d_scoreF || !d_H21 || !d_H12 || !d_F21 || !d_best || !d_S || !d_inlH || !d_inlF)
        return ORBX_ERR_ARG;
    std::memset(&PR, 0, sizeof(PR));
    iters = 0;
    for (int p = 0; p < nproblems; p++) {
        const orbi_problem& q = problems[p];
        if (check_problem(q) != ORBX_OK || q.n1 > kcap1 || q.n2 > kcap2 || q.nmatches > mcap || q.iters > icap) return ORBX_ERR_ARG;
        PR.p[p] = q;
        if (q.iters > iters) iters = q.iters;
    }
    return ORBX_OK;
}

// orbi_check_rt_batch_device's arguments; on ORBX_OK C holds the counts
inline int check_rt(const void* d_poses, int nhyp, int nproblems, const int32_t* n1, const int32_t* n2, const int32_t* nmatches, const void* d_kps1,
                    int kcap1, const void* d_kps2, int kcap2, const void* d_matches, int mcap, const void* d_flags, const void* d_status,
                    const void* d_x3d, const void* d_cos, const void* d_good, const void* d_v, const void* d_ngood, RtCounts& C) {
    if (nhyp < 1 || nhyp > ORBI_MAX_HYP || nproblems < 1 || nproblems > ORBI_MAX_PROBLEMS || !n1 || !n2 || !nmatches || kcap1 < 1 ||
        kcap1 > ORBF_MAX_FEATURES || kcap2 < 1 || kcap2 > ORBF_MAX_FEATURES || mcap < 1 || mcap > ORBI_MAX_MATCHES)
        return ORBX_ERR_ARG;
    if (!d_poses || !d_kps1 || !d_kps2 || !d_matches || !d_flags || !d_status || !d_x3d || !d_cos || !d_good || !d_ngood) return ORBX_ERR_ARG;
    if (d_v && ((uintptr_t)d_v & 15)) return ORBX_ERR_ARG;             // written as float4
    std::memset(&C, 0, sizeof(C));
    for (int p = 0; p < nproblems; p++) {
        if (n1[p] < 0 || n1[p] > kcap1 || n2[p] < 0 || n2[p] > kcap2 || nmatches[p] < 0 || nmatches[p] > mcap) return ORBX_ERR_ARG;
        C.n1[p] = n1[p]; C.n2[p] = n2[p]; C.nm[p] = nmatches[p];
    }
    return ORBX_OK;
}

}  // namespace orbi
