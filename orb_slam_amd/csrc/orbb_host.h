// The host side of the orbb_* calls: the argument checks, the layout of the work buffer, the state helpers and the serial form of every pass (the
// host route's system, HostSys).  Plain C++, so that tests/_probe/localba_host.cpp and the host route run it without a GPU.
#pragma once
#include <stdint.h>
#include <cstring>
#include <vector>

#include "orbb.h"
#include "orbb_math.h"
#include "orbo_host.h"

namespace orbb {

using orbo::all_set;

inline int check_problem(const orbb_problem* q) {
    if (!q) return ORBX_ERR_ARG;
    if (q->nfree < 1 || q->nfree > ORBB_MAX_FREE || q->nfixed < 0 || q->nfree + q->nfixed > ORBB_MAX_POSES) return ORBX_ERR_ARG;
    if (q->npoints < 0 || q->npoints > ORBB_MAX_POINTS || q->nedges < 0 || q->nedges > ORBB_MAX_EDGES) return ORBX_ERR_ARG;
    return ORBX_OK;
}
inline int check_iters(int iters) { return iters < 0 || iters > ORBB_MAX_ITERS ? ORBX_ERR_ARG : ORBX_OK; }

// the index arrays of a host form: ranges that tile the edges in order, pose indices inside the problem, at most one edge per (point, pose)
inline int check_indices(const orbb_problem& q, const int32_t* point_first, const int32_t* edge_pose) {
    if (point_first[0] != 0 || point_first[q.npoints] != q.nedges) return ORBX_ERR_ARG;
    std::vector<int32_t> seen((size_t)q.nfree + q.nfixed, -1);
    for (int j = 0; j < q.npoints; j++) {
        if (point_first[j + 1] < point_first[j] || point_first[j + 1] > q.nedges) return ORBX_ERR_ARG;
        for (int e = point_first[j]; e < point_first[j + 1]; e++) {
            const int p = edge_pose[e];
            if (p < 0 || p >= q.nfree + q.nfixed || seen[p] == j) return ORBX_ERR_ARG;
            seen[p] = j;
        }
    }
    return ORBX_OK;
}

// The work buffer: every array at a multiple of 256 bytes.  base == nullptr only measures.  Returns the bytes.
inline size_t layout(const orbb_problem& q, void* base, Ctx& c) {
    size_t off = 0;
    auto take = [&](auto*& ptr, size_t count) {
        using T = std::remove_reference_t<decltype(*ptr)>;
        ptr = base ? reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off) : nullptr;
        off = (off + (count ? count : 1) * sizeof(T) + 255) & ~(size_t)255;
    };
    const size_t np = (size_t)q.nfree + q.nfixed, P = q.npoints, E = q.nedges, n = (size_t)6 * q.nfree;
    c.nfree = q.nfree;
    c.np = (int)np;
    c.npoints = q.npoints;
    c.nedges = q.nedges;
    c.n = (int)n;
    take(c.ctl, ORBB_CTL);
    take(c.pose[0], np * 7);
    take(c.pose[1], np * 7);
    take(c.point[0], P * 3);
    take(c.point[1], P * 3);
    take(c.Hpp, (size_t)q.nfree * NACC);
    take(c.Hll, P * 6);
    take(c.bl, P * 3);
    take(c.Dinv, P * 6);
    take(c.Hpl, E * 18);
    take(c.S, n * n);
    take(c.bs, n);
    take(c.xp, n);
    take(c.xl, P * 3);
    take(c.pt_chi, P);
    take(c.pt_scale, P);
    take(c.pt_diag, P);
    take(c.edge_point, E);
    take(c.pose_first, (size_t)q.nfree + 1);
    take(c.pose_count, (size_t)q.nfree);
    take(c.pose_edges, E);
    take(c.pose_nact, (size_t)q.nfree);
    take(c.pt_nact, P);
    return off;
}

inline void set_huber(Ctx& c, float huber_delta) {
    c.delta = (double)huber_delta;
    c.dsqr = (double)(float)(c.delta * c.delta);
}

inline int state_from_float(const orbb_problem* q, const float* Tcw, const float* world, double* pose_qt, double* point_xyz) {
    if (check_problem(q) != ORBX_OK || !all_set({Tcw, pose_qt}) || (q->npoints > 0 && !all_set({world, point_xyz}))) return ORBX_ERR_ARG;
    for (int p = 0; p < q->nfree + q->nfixed; p++) {
        const float* R = Tcw + (size_t)p * 12;
        const float T[16] = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8], R[9], R[10], R[11], 0, 0, 0, 1};
        Pose P;
        orbo::pose_from_Tcw(T, P);
        store_pose(pose_qt, p, P);
    }
    for (size_t i = 0; i < (size_t)q->npoints * 3; i++) point_xyz[i] = (double)world[i];
    return ORBX_OK;
}
inline int state_to_float(const orbb_problem* q, const double* pose_qt, const double* point_xyz, float* Tcw, float* world) {
    if (check_problem(q) != ORBX_OK || !all_set({Tcw, pose_qt}) || (q->npoints > 0 && !all_set({world, point_xyz}))) return ORBX_ERR_ARG;
    for (int p = 0; p < q->nfree + q->nfixed; p++) {
        float T[16];
        orbo::pose_to_Tcw(load_pose(pose_qt, p), T);
        std::memcpy(Tcw + (size_t)p * 16, T, sizeof(T));
    }
    for (size_t i = 0; i < (size_t)q->npoints * 3; i++) world[i] = (float)point_xyz[i];
    return ORBX_OK;
}

// the first-build dump out of the work buffer (S and bs are copied before the solve destroys them: `part` 0; the rest after the back-substitution: 1)
template <class Copy>
inline void dump_part(const Ctx& c, double* dump, int part, Copy copy) {
    const size_t nf = c.nfree, P = c.npoints, n = c.n;
    double* d = dump;
    if (part == 1) copy(d, c.Hpp, nf * NACC);
    d += nf * NACC;
    if (part == 1) copy(d, c.Hll, P * 6);
    d += P * 6;
    if (part == 1) copy(d, c.bl, P * 3);
    d += P * 3;
    if (part == 0) copy(d, c.S, n * n);
    d += n * n;
    if (part == 0) copy(d, c.bs, n);
    d += n;
    if (part == 1) copy(d, c.xp, n);
    d += n;
    if (part == 1) copy(d, c.xl, P * 3);
}

// ---- the host route: every pass as a serial loop over the items a kernel spreads over its threads ----
struct HostSys {
    Ctx c;
    int cur = 0;
    double* dump = nullptr;
    std::vector<double> y;

    void setup() {
        const size_t E = c.nedges;
        for (size_t e = 0; e < E; e++) c.edge_point[e] = -1;
        for (int j = 0; j < c.npoints; j++) point_setup(c, j);
        // the by-pose list: stable, ascending in edge index
        for (int p = 0; p < c.nfree; p++) c.pose_count[p] = 0;
        for (int e = 0; e < c.nedges; e++)
            if ((unsigned)c.edge_pose[e] < (unsigned)c.nfree) c.pose_count[c.edge_pose[e]]++;
        c.pose_first[0] = 0;
        for (int p = 0; p < c.nfree; p++) c.pose_first[p + 1] = c.pose_first[p] + c.pose_count[p];
        std::vector<int32_t> at(c.pose_first, c.pose_first + c.nfree);
        for (int e = 0; e < c.nedges; e++)
            if ((unsigned)c.edge_pose[e] < (unsigned)c.nfree) c.pose_edges[at[c.edge_pose[e]]++] = e;
    }
    void reduce() {
        std::vector<Red> v(RL);
        for (int l = 0; l < RL; l++) v[l] = reduce_lane(c, l);
        for (int d = RL / 2; d >= 1; d >>= 1)
            for (int l = 0; l < d; l++) reduce_join(v[l], v[l + d]);
        reduce_finish(c, v[0]);
    }
    int chi_only(double* ctl) {
        for (int j = 0; j < c.npoints; j++) point_linearize<false>(c, c.pose[cur], c.point[cur], j);
        // pt_nact is what the reduction counts; a call that iterates nothing has not set it
        reduce();
        std::memcpy(ctl, c.ctl, sizeof(double) * ORBB_CTL);
        return ORBX_OK;
    }
    int build(double* ctl) {
        for (int j = 0; j < c.npoints; j++) point_linearize<true>(c, c.pose[cur], c.point[cur], j);
        for (int p = 0; p < c.nfree; p++) {
            double part[NACC][LANES], acc[NACC];
            int nact = 0, na;
            for (int l = 0; l < LANES; l++) {
                pose_lane_sums(c, c.pose[cur], c.point[cur], p, l, acc, na);
                nact += na;
                for (int a = 0; a < NACC; a++) part[a][l] = acc[a];
            }
            for (int a = 0; a < NACC; a++) {
                for (int d = 32; d >= 1; d >>= 1)
                    for (int l = 0; l < d; l++) part[a][l] = part[a][l] + part[a][l + d];
                c.Hpp[(size_t)p * NACC + a] = part[a][0];
            }
            c.pose_nact[p] = nact;
        }
        reduce();
        std::memcpy(ctl, c.ctl, sizeof(double) * ORBB_CTL);
        return ORBX_OK;
    }
    void schur_row(double lambda, int p1) {
        const int n = c.n;
        std::vector<double> row((size_t)6 * n);
        double bsr[6], BD[18];
        for (int a = 0; a < 6; a++) {
            for (int col = 0; col < n; col++) row[(size_t)a * n + col] = schur_row_init(c, lambda, p1, a, col);
            bsr[a] = schur_rhs_init(c, p1, a);
        }
        for (int k = c.pose_first[p1]; k < c.pose_first[p1 + 1]; k++) {
            const int e1 = c.pose_edges[k], j = c.edge_point[e1];
            if (!edge_active(c, e1) || j < 0) continue;
            for (int t = 0; t < 18; t++) BD[t] = schur_bd(c, e1, j, t / 3, t % 3);
            for (int a = 0; a < 6; a++) bsr[a] = bsr[a] - schur_rhs_term(c, BD, j, a);
            int lo, hi;
            point_range(c, j, lo, hi);
            for (int e2 = lo; e2 < hi; e2++) {
                if (!schur_pairs(c, e2, p1)) continue;
                const int p2 = c.edge_pose[e2];
                for (int a = 0; a < 6; a++)
                    for (int b = 0; b < 6; b++) row[(size_t)a * n + p2 * 6 + b] = row[(size_t)a * n + p2 * 6 + b] - schur_term(c, BD, e2, a, b);
            }
        }
        for (int a = 0; a < 6; a++) {
            for (int col = 0; col < (p1 + 1) * 6; col++) c.S[(size_t)(p1 * 6 + a) * n + col] = row[(size_t)a * n + col];
            c.bs[p1 * 6 + a] = bsr[a];
        }
    }
    int trial(double lambda, bool first, double* ctl) {
        const auto copy = [](double* d, const double* s, size_t k) { std::memcpy(d, s, k * sizeof(double)); };
        for (int j = 0; j < c.npoints; j++) point_dinv(c, lambda, j);
        for (int p = 0; p < c.nfree; p++) schur_row(lambda, p);
        if (first && dump) dump_part(c, dump, 0, copy);
        y.resize(c.n);
        const bool solved = ldl_solve_serial(c, y.data());
        c.ctl[CTL_SOLVED] = solved ? 1.0 : 0.0;
        c.ctl[CTL_SCALE_POSES] = scale_poses(c, lambda);
        for (int j = 0; j < c.npoints; j++) point_back(c, lambda, solved, c.point[cur], c.point[cur ^ 1], j);
        for (int p = 0; p < c.np; p++) pose_back(c, c.pose[cur], c.pose[cur ^ 1], p);
        if (first && dump) dump_part(c, dump, 1, copy);
        for (int j = 0; j < c.npoints; j++) point_linearize<false>(c, c.pose[cur ^ 1], c.point[cur ^ 1], j);
        reduce();
        std::memcpy(ctl, c.ctl, sizeof(double) * ORBB_CTL);
        return ORBX_OK;
    }
    void accept() { cur ^= 1; }
};

}  // namespace orbb
