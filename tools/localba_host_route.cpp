// The host route tools/bench_localba.py measures the device bundle adjustment against: the host forms of include/orbb.h on one host core over the same
// arithmetic text (orb_slam_amd/csrc/orbb_math.h), the same summation orders and the same argument checks (orbb_host.h), every pass as a serial loop
// over the items a kernel spreads over its threads.  tests/test_localba_host.py holds it against the numpy restatement; code written against the
// library links against this file instead and runs on the host.  `device` is ignored.  Build with -ffp-contract=off.
#include <cstring>
#include <type_traits>
#include <vector>

#include "orbb_host.h"
#include "orbb_math.h"

extern "C" {

int orbb_state_from_float(const orbb_problem* problem, const float* Tcw, const float* world, double* pose_qt, double* point_xyz) {
    return orbb::state_from_float(problem, Tcw, world, pose_qt, point_xyz);
}
int orbb_state_to_float(const orbb_problem* problem, const double* pose_qt, const double* point_xyz, float* Tcw, float* world) {
    return orbb::state_to_float(problem, pose_qt, point_xyz, Tcw, world);
}
size_t orbb_work_bytes(const orbb_problem* problem) {
    orbb::Ctx c;
    return orbb::check_problem(problem) == ORBX_OK ? orbb::layout(*problem, nullptr, c) : 0;
}

int orbb_optimize(const orbb_problem* problem, const float* cam, const int32_t* point_first, const int32_t* edge_pose, const float* edge_uv,
                  const float* edge_inv_sigma2, float huber_delta, double* pose_qt, double* point_xyz, const uint64_t* active, double* chi2,
                  int iters, orbb_result* result, uint64_t* flags, orbo_step* trace, double* dump, int) {
    using namespace orbb;
    if (check_problem(problem) != ORBX_OK || check_iters(iters) != ORBX_OK || !all_set({cam, point_first, pose_qt, result})) return ORBX_ERR_ARG;
    const orbb_problem& q = *problem;
    if (q.npoints > 0 && !point_xyz) return ORBX_ERR_ARG;
    if (q.nedges > 0 && !all_set({edge_pose, edge_uv, edge_inv_sigma2, active, chi2, flags})) return ORBX_ERR_ARG;
    if (check_indices(q, point_first, edge_pose) != ORBX_OK) return ORBX_ERR_ARG;
    HostSys sys;
    std::vector<uint8_t> work(layout(q, nullptr, sys.c) + 256, 0);
    void* base = work.data() + (256 - (uintptr_t)work.data() % 256) % 256;
    layout(q, base, sys.c);
    Ctx& c = sys.c;
    set_huber(c, huber_delta);
    c.cam = cam;
    c.point_first = point_first;
    c.edge_pose = edge_pose;
    c.edge_uv = edge_uv;
    c.edge_w = edge_inv_sigma2;
    c.active = active;
    c.chi2 = chi2;
    sys.dump = dump;
    if (dump) std::memset(dump, 0, ORBB_DUMP_DOUBLES(q.nfree, q.npoints) * sizeof(double));
    std::memcpy(c.pose[0], pose_qt, (size_t)c.np * 7 * sizeof(double));
    if (q.npoints) std::memcpy(c.point[0], point_xyz, (size_t)q.npoints * 3 * sizeof(double));
    sys.setup();
    std::memset(result, 0, sizeof(*result));
    const int rc = optimize(sys, iters, *result, trace);
    if (rc != ORBX_OK) return rc;
    std::memcpy(pose_qt, c.pose[sys.cur], (size_t)c.np * 7 * sizeof(double));
    if (q.npoints) std::memcpy(point_xyz, c.point[sys.cur], (size_t)q.npoints * 3 * sizeof(double));
    if (q.nedges) std::memset(flags, 0, ORBB_WORDS(q.nedges) * sizeof(uint64_t));
    for (int e = 0; e < q.nedges; e++)
        if (edge_flag(c, pose_qt, point_xyz, e)) flags[e >> 6] |= (uint64_t)1 << (e & 63);
    return ORBX_OK;
}

}  // extern "C"
