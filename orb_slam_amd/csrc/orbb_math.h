// The arithmetic of the bundle adjustment (include/orbb.h states it): g2o's Levenberg iteration over a BlockSolver with the Schur complement as
// Optimizer::LocalBundleAdjustment and Optimizer::BundleAdjustment use it.  One text for the device (orbb_ba.hip), the host route
// (tools/localba_host_route.cpp) and tests/_probe/localba_host.cpp: the per-item functions below are what a thread of a kernel runs for its point,
// pose lane, matrix entry or edge, and what the host route runs in a serial loop over the same items; the orders of the sums live here.  Error,
// Huber, the pose Jacobian, exp and the pose conversions are orbo_math.h's.  Everything is double.  Compile with -ffp-contract=off.
//
// The steps NOT pinned to Eigen are point_dinv (the 3 x 3 inverse) and the dense LDL' (ldl_* and the loops around them).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "orbb.h"
#include "orbo_math.h"

namespace orbb {

using orbo::Cam;
using orbo::Edge;
using orbo::LANES;
using orbo::NACC;
using orbo::Pose;
using orbo::dot3;

constexpr int RL = ORBB_REDUCE_LANES;
// the control block (ORBB_CTL doubles) a pass leaves for the host
enum { CTL_CHI = 0, CTL_SCALE_POSES = 1, CTL_SCALE_POINTS = 2, CTL_MAXDIAG = 3, CTL_SOLVED = 4, CTL_NACTIVE = 5 };

// One problem's arrays: the caller's (device or host memory alike) and the work buffer's (orbb_host.h lays it out).
struct Ctx {
    int nfree, np, npoints, nedges, n;                      // np = nfree + nfixed, n = 6*nfree
    double delta, dsqr;                                     // the Huber kernel's two constants
    const float* cam;
    const int32_t* point_first;
    const int32_t* edge_pose;
    const float* edge_uv;
    const float* edge_w;
    const uint64_t* active;
    double* chi2;
    int32_t *edge_point, *pose_first, *pose_count, *pose_edges, *pose_nact, *pt_nact;
    double *pose[2], *point[2];                             // the estimate and the trial, swapped on accept
    double *Hpp, *Hll, *bl, *Dinv, *Hpl, *S, *bs, *xp, *xl, *pt_chi, *pt_scale, *pt_diag, *ctl;
};

ORB_HD bool pose_in_problem(const Ctx& c, int e) { return (unsigned)c.edge_pose[e] < (unsigned)c.np; }
ORB_HD bool edge_active(const Ctx& c, int e) { return ((c.active[e >> 6] >> (e & 63)) & 1) && pose_in_problem(c, e); }
ORB_HD void point_range(const Ctx& c, int j, int& lo, int& hi) {
    lo = c.point_first[j];
    hi = c.point_first[j + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > c.nedges ? c.nedges : hi;
}
ORB_HD Pose load_pose(const double* poses, int p) {
    Pose P;
ORB_UNROLL
    for (int i = 0; i < 4; i++) P.q[i] = poses[(size_t)p * 7 + i];
ORB_UNROLL
    for (int i = 0; i < 3; i++) P.t[i] = poses[(size_t)p * 7 + 4 + i];
    return P;
}
ORB_HD void store_pose(double* poses, int p, const Pose& P) {
ORB_UNROLL
    for (int i = 0; i < 4; i++) poses[(size_t)p * 7 + i] = P.q[i];
ORB_UNROLL
    for (int i = 0; i < 3; i++) poses[(size_t)p * 7 + 4 + i] = P.t[i];
}
ORB_HD Cam load_cam(const Ctx& c, int p) {
    return {(double)c.cam[(size_t)p * 4], (double)c.cam[(size_t)p * 4 + 1], (double)c.cam[(size_t)p * 4 + 2], (double)c.cam[(size_t)p * 4 + 3]};
}
ORB_HD Edge load_edge(const Ctx& c, const double* points, int j, int e) {
    return {points[(size_t)j * 3], points[(size_t)j * 3 + 1], points[(size_t)j * 3 + 2], (double)c.edge_uv[(size_t)e * 2], (double)c.edge_uv[(size_t)e * 2 + 1],
            (double)c.edge_w[e]};
}
// std::max(fabs(h), m)
ORB_HD double max_abs(double h, double m) {
    h = fabs(h);
    return (h < m) ? m : h;
}

// the Jacobian of the error by the point (types_six_dof_expmap.cpp:110-119) at the camera point p
ORB_HD void point_jacobian(const Cam& c, const double (&p)[3], const double (&R)[3][3], double (&J)[2][3]) {
    const double x = p[0], y = p[1], z = p[2];
    const double s = -1.0 / z;
    const double T[2][3] = {{s * c.fx, s * 0.0, s * (((-x) / z) * c.fx)}, {s * 0.0, s * c.fy, s * (((-y) / z) * c.fy)}};
ORB_UNROLL
    for (int r = 0; r < 2; r++)
ORB_UNROLL
        for (int k = 0; k < 3; k++) J[r][k] = dot3(T[r][0], R[0][k], T[r][1], R[1][k], T[r][2], R[2][k]);
}

// ---- setup: every edge's point ----
ORB_HD void point_setup(const Ctx& c, int j) {
    int lo, hi;
    point_range(c, j, lo, hi);
    for (int e = lo; e < hi; e++) c.edge_point[e] = j;
}

// ---- a point's pass over its edges: the errors and chi2 (the trial pass), with FULL also Hll, bl and the Hpl blocks ----
template <bool FULL>
ORB_HD void point_linearize(const Ctx& c, const double* poses, const double* points, int j) {
    int lo, hi;
    point_range(c, j, lo, hi);
    double hll[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bl[3] = {0.0, 0.0, 0.0}, chi = 0.0;
    int nact = 0;
    for (int e = lo; e < hi; e++) {
        if (!edge_active(c, e)) continue;
        const int p = c.edge_pose[e];
        const Pose P = load_pose(poses, p);
        const Cam cam = load_cam(c, p);
        const Edge E = load_edge(c, points, j, e);
        double pc[3], er[2];
        const double chi2 = orbo::edge_error(cam, P, E, pc, er);
        c.chi2[e] = chi2;
        double rho0, rho1;
        orbo::huber(chi2, c.delta, c.dsqr, rho0, rho1);
        chi = chi + rho0;
        nact++;
        if (FULL) {
            double Jp[2][6], Jl[2][3], R[3][3];
            orbo::pose_jacobian(cam, pc, Jp);
            orbo::rotation_matrix(P.q, R);
            point_jacobian(cam, pc, R, Jl);
            const double wr = E.w * rho1;
            const double r0 = ((-E.w) * er[0]) * rho1, r1 = ((-E.w) * er[1]) * rho1;
            int a = 0;
ORB_UNROLL
            for (int k = 0; k < 3; k++)
ORB_UNROLL
                for (int d = k; d < 3; d++, a++) hll[a] = hll[a] + ((Jl[0][k] * wr) * Jl[0][d] + (Jl[1][k] * wr) * Jl[1][d]);
ORB_UNROLL
            for (int k = 0; k < 3; k++) bl[k] = bl[k] + (Jl[0][k] * r0 + Jl[1][k] * r1);
            if (p < c.nfree) {
                double* H = c.Hpl + (size_t)e * 18;
ORB_UNROLL
                for (int k = 0; k < 3; k++)
ORB_UNROLL
                    for (int i = 0; i < 6; i++) H[k * 6 + i] = (Jl[0][k] * wr) * Jp[0][i] + (Jl[1][k] * wr) * Jp[1][i];
            }
        }
    }
    c.pt_chi[j] = chi;
    if (FULL) {
ORB_UNROLL
        for (int a = 0; a < 6; a++) c.Hll[(size_t)j * 6 + a] = hll[a];
ORB_UNROLL
        for (int k = 0; k < 3; k++) c.bl[(size_t)j * 3 + k] = bl[k];
        c.pt_nact[j] = nact;
        c.pt_diag[j] = max_abs(hll[5], max_abs(hll[3], max_abs(hll[0], 0.0)));
    }
}

// ---- a lane's share of a free pose's sums: the active edges at the positions lane, lane + 64, ... of the pose's list ----
ORB_HD void pose_lane_sums(const Ctx& c, const double* poses, const double* points, int p, int lane, double (&acc)[NACC], int& nact) {
ORB_UNROLL
    for (int a = 0; a < NACC; a++) acc[a] = 0.0;
    nact = 0;
    const Pose P = load_pose(poses, p);
    const Cam cam = load_cam(c, p);
    const int lo = c.pose_first[p], hi = c.pose_first[p + 1];
    for (int k = lo + lane; k < hi; k += LANES) {
        const int e = c.pose_edges[k];
        const int j = c.edge_point[e];
        if (!edge_active(c, e) || j < 0) continue;
        orbo::add_edge(cam, P, load_edge(c, points, j, e), c.delta, c.dsqr, acc);
        nact++;
    }
}

// entry (a, b) of the symmetric 6 x 6 block packed row by row as 21 upper entries (orbo.h)
ORB_HD int sym6(int a, int b) {
    const int i = a < b ? a : b, j = a < b ? b : a;
    return i * 6 - (i * (i - 1)) / 2 + (j - i);
}
// entry (r, k) of a symmetric 3 x 3 packed 00 01 02 11 12 22
ORB_HD int sym3(int r, int k) {
    const int i = r < k ? r : k, j = r < k ? k : r;
    return i == 0 ? j : i == 1 ? 2 + j : 5;
}

// ---- (Hll + lambda*I)^-1 of a point: NOT pinned to Eigen (orbb.h, step 1) ----
ORB_HD void point_dinv(const Ctx& c, double lambda, int j) {
    const double* H = c.Hll + (size_t)j * 6;
    const double a = H[0] + lambda, b = H[1], cc = H[2], d = H[3] + lambda, e = H[4], f = H[5] + lambda;
    const double c00 = d * f - e * e, c01 = cc * e - b * f, c02 = b * e - cc * d, c11 = a * f - cc * cc, c12 = b * cc - a * e, c22 = a * d - b * b;
    const double det = (a * c00 + b * c01) + cc * c02;
    double* D = c.Dinv + (size_t)j * 6;
    D[0] = c00 / det;
    D[1] = c01 / det;
    D[2] = c02 / det;
    D[3] = c11 / det;
    D[4] = c12 / det;
    D[5] = c22 / det;
}

// ---- the Schur complement, one block row p1 at a time (block_solver.hpp:367-486) ----
// the row's start: Hpp + lambda*I in the diagonal block (the identity for a pose without an active edge), zeros elsewhere; idx = a*n + col
ORB_HD double schur_row_init(const Ctx& c, double lambda, int p1, int a, int col) {
    const int p2 = col / 6, b = col % 6;
    if (p2 != p1) return 0.0;
    if (c.pose_nact[p1] == 0) return a == b ? 1.0 : 0.0;
    const double h = c.Hpp[(size_t)p1 * NACC + sym6(a, b)];
    return a == b ? h + lambda : h;
}
ORB_HD double schur_rhs_init(const Ctx& c, int p1, int a) { return c.pose_nact[p1] == 0 ? 0.0 : c.Hpp[(size_t)p1 * NACC + 21 + a]; }
// BD[a][k] of edge e1 of point j
ORB_HD double schur_bd(const Ctx& c, int e1, int j, int a, int k) {
    const double* H = c.Hpl + (size_t)e1 * 18;
    const double* D = c.Dinv + (size_t)j * 6;
    return dot3(H[a], D[sym3(0, k)], H[6 + a], D[sym3(1, k)], H[12 + a], D[sym3(2, k)]);
}
ORB_HD double schur_rhs_term(const Ctx& c, const double* BD, int j, int a) {
    const double* bl = c.bl + (size_t)j * 3;
    return dot3(BD[a * 3], bl[0], BD[a * 3 + 1], bl[1], BD[a * 3 + 2], bl[2]);
}
ORB_HD double schur_term(const Ctx& c, const double* BD, int e2, int a, int b) {
    const double* H = c.Hpl + (size_t)e2 * 18;
    return dot3(BD[a * 3], H[b], BD[a * 3 + 1], H[6 + b], BD[a * 3 + 2], H[12 + b]);
}
// does edge e2 of the point of e1 subtract from row p1?
ORB_HD bool schur_pairs(const Ctx& c, int e2, int p1) { return edge_active(c, e2) && c.edge_pose[e2] <= p1; }

// ---- the dense LDL': NOT pinned to Eigen (orbb.h, step 2).  The loops are the kernel's and the host route's; these are the operations. ----
ORB_HD bool ldl_pivot_ok(double d) { return !(d < 0 || !__builtin_isfinite(d)); }
ORB_HD double ldl_update(double a, double lik, double ljk, double dk) { return a - (lik * ljk) * dk; }
ORB_HD double sub_update(double y, double l, double yk) { return y - l * yk; }
// the pose part of computeScale, serially
ORB_HD double scale_poses(const Ctx& c, double lambda) {
    double s = 0.0;
    for (int j = 0; j < c.n; j++) s = s + c.xp[j] * (lambda * c.xp[j] + schur_rhs_init(c, j / 6, j % 6));
    return s;
}
// the whole solve in serial form (the host route; the kernel runs the same operations with the i and j loops spread over its threads)
inline bool ldl_solve_serial(const Ctx& c, double* y) {
    const int n = c.n;
    double* S = c.S;
    bool ok = true;
    for (int k = 0; k < n; k++) {
        const double dk = S[(size_t)k * n + k];
        ok = ok && ldl_pivot_ok(dk);
        for (int i = k + 1; i < n; i++) S[(size_t)i * n + k] = S[(size_t)i * n + k] / dk;
        for (int i = k + 1; i < n; i++)
            for (int j = k + 1; j <= i; j++) S[(size_t)i * n + j] = ldl_update(S[(size_t)i * n + j], S[(size_t)i * n + k], S[(size_t)j * n + k], dk);
    }
    for (int i = 0; i < n; i++) y[i] = c.bs[i];
    for (int k = 0; k < n; k++)
        for (int i = k + 1; i < n; i++) y[i] = sub_update(y[i], S[(size_t)i * n + k], y[k]);
    for (int i = 0; i < n; i++) y[i] = y[i] / S[(size_t)i * n + i];
    for (int k = n - 1; k >= 1; k--)
        for (int i = 0; i < k; i++) y[i] = sub_update(y[i], S[(size_t)k * n + i], y[k]);
    if (ok)
        for (int i = 0; i < n; i++) c.xp[i] = y[i];
    return ok;
}

// ---- back-substitution and the trial estimate of a point; its share of computeScale ----
ORB_HD void point_back(const Ctx& c, double lambda, bool solved, const double* est, double* trial, int j) {
    double* xl = c.xl + (size_t)j * 3;
    if (c.pt_nact[j] == 0) {
ORB_UNROLL
        for (int k = 0; k < 3; k++) {
            xl[k] = 0.0;
            trial[(size_t)j * 3 + k] = est[(size_t)j * 3 + k];
        }
        c.pt_scale[j] = 0.0;
        return;
    }
    const double* bl = c.bl + (size_t)j * 3;
    if (solved) {
        double cl[3] = {bl[0], bl[1], bl[2]};
        int lo, hi;
        point_range(c, j, lo, hi);
        for (int e = lo; e < hi; e++) {
            if (!edge_active(c, e) || c.edge_pose[e] >= c.nfree) continue;
            const double* H = c.Hpl + (size_t)e * 18;
            const double* x = c.xp + (size_t)c.edge_pose[e] * 6;
ORB_UNROLL
            for (int k = 0; k < 3; k++)
                cl[k] = cl[k] - (((((H[k * 6] * x[0] + H[k * 6 + 1] * x[1]) + H[k * 6 + 2] * x[2]) + H[k * 6 + 3] * x[3]) + H[k * 6 + 4] * x[4]) + H[k * 6 + 5] * x[5]);
        }
        const double* D = c.Dinv + (size_t)j * 6;
ORB_UNROLL
        for (int r = 0; r < 3; r++) xl[r] = dot3(D[sym3(r, 0)], cl[0], D[sym3(r, 1)], cl[1], D[sym3(r, 2)], cl[2]);
    }
ORB_UNROLL
    for (int k = 0; k < 3; k++) trial[(size_t)j * 3 + k] = est[(size_t)j * 3 + k] + xl[k];
    c.pt_scale[j] = (xl[0] * (lambda * xl[0] + bl[0]) + xl[1] * (lambda * xl[1] + bl[1])) + xl[2] * (lambda * xl[2] + bl[2]);
}
// the trial estimate of a pose
ORB_HD void pose_back(const Ctx& c, const double* est, double* trial, int p) {
    const Pose P = load_pose(est, p);
    if (p >= c.nfree || c.pose_nact[p] == 0) {
        store_pose(trial, p, P);
        return;
    }
    double x[6];
ORB_UNROLL
    for (int i = 0; i < 6; i++) x[i] = c.xp[(size_t)p * 6 + i];
    Pose out;
    orbo::exp_update(x, P, out);
    store_pose(trial, p, out);
}

// ---- the sums over the points: a lane's share, then the tree (orbb.h) ----
struct Red { double chi, scale, diag, nact; };
ORB_HD Red reduce_lane(const Ctx& c, int lane) {
    Red r = {0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < c.npoints; j += RL) {
        r.chi = r.chi + c.pt_chi[j];
        r.scale = r.scale + c.pt_scale[j];
        r.diag = max_abs(c.pt_diag[j], r.diag);
        r.nact = r.nact + (double)c.pt_nact[j];
    }
    return r;
}
ORB_HD void reduce_join(Red& a, const Red& b) {
    a.chi = a.chi + b.chi;
    a.scale = a.scale + b.scale;
    a.diag = (b.diag < a.diag) ? a.diag : b.diag;
    a.nact = a.nact + b.nact;
}
ORB_HD void reduce_finish(const Ctx& c, const Red& r) {
    double m = 0.0;
    for (int p = 0; p < c.nfree; p++)
        for (int i = 0; i < 6; i++) m = max_abs(c.Hpp[(size_t)p * NACC + sym6(i, i)], m);
    c.ctl[CTL_CHI] = r.chi;
    c.ctl[CTL_SCALE_POINTS] = r.scale;
    c.ctl[CTL_MAXDIAG] = (r.diag < m) ? m : r.diag;
    c.ctl[CTL_NACTIVE] = r.nact;
}

// ---- the flag of an edge (Optimizer.cc:461) at the final estimate ----
ORB_HD bool edge_flag(const Ctx& c, const double* poses, const double* points, int e) {
    const int j = c.edge_point[e];
    if (!edge_active(c, e) || j < 0) return false;
    const Pose P = load_pose(poses, c.edge_pose[e]);
    double r[3];
    orbo::rotate(P.q, points[(size_t)j * 3], points[(size_t)j * 3 + 1], points[(size_t)j * 3 + 2], r);
    const double z = r[2] + P.t[2];
    return c.chi2[e] > 5.991 || !(z > 0.0);
}

// ---- OptimizationAlgorithmLevenberg::solve and SparseOptimizer::optimize: plain IEEE on the host, from the control block ----
// Sys: build(ctl) linearises at the estimate (chi, the largest diagonal, the number of active edges); trial(lambda, first, ctl) damps, reduces,
// solves, makes the trial estimate and its chi; accept() makes the trial the estimate; chi_only(ctl) computes the errors at the estimate.
// Every one of them returns an orbx status.
template <class Sys>
inline int optimize(Sys& sys, int iters, orbb_result& res, orbo_step* trace) {
    double ctl[ORBB_CTL];
    res.chi_first = res.chi_last = res.lambda = 0.0;
    res.iters = 0;
    res.status = ORBB_RUN_NOTHING;
    if (trace)
        for (int i = 0; i < ORBB_MAX_ITERS; i++) trace[i] = orbo::step_not_run();
    if (iters <= 0) {
        const int rc = sys.chi_only(ctl);
        res.chi_first = res.chi_last = ctl[CTL_CHI];
        return rc;
    }
    double lambda = 0.0, ni = 2.0, currentChi = 0.0;
    int stalled = 0;
    bool ok = true;
    for (int it = 0; it < iters && ok; it++) {
        int rc = sys.build(ctl);
        if (rc != ORBX_OK) return rc;
        currentChi = ctl[CTL_CHI];
        double tempChi = currentChi;
        const double iniChi = currentChi;
        if (it == 0) {
            res.chi_first = res.chi_last = currentChi;
            if (ctl[CTL_NACTIVE] == 0.0) return ORBX_OK;                            // sparse_optimizer.cpp:356-359
            lambda = 1e-5 * ctl[CTL_MAXDIAG];                                       // computeLambdaInit
            ni = 2.0;
            stalled = 0;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            rc = sys.trial(lambda, it == 0 && qmax == 0, ctl);
            if (rc != ORBX_OK) return rc;
            tempChi = ctl[CTL_CHI];
            if (ctl[CTL_SOLVED] == 0.0) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            const double scale = (ctl[CTL_SCALE_POSES] + ctl[CTL_SCALE_POINTS]) + 1e-3;
            rho = rho / scale;
            if (rho > 0 && __builtin_isfinite(tempChi)) {
                const double cc = 2 * rho - 1;
                double alpha = 1.0 - (cc * cc) * cc;
                const double upper = 2.0 / 3.0, lower = 1.0 / 3.0;
                alpha = (upper < alpha) ? upper : alpha;
                const double scaleFactor = (lower < alpha) ? alpha : lower;
                lambda = lambda * scaleFactor;
                ni = 2.0;
                currentChi = tempChi;
                sys.accept();
            } else {
                lambda = lambda * ni;
                ni = ni * 2.0;
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        bool terminate = qmax == 10 || rho == 0;
        if (!terminate) {
            if ((iniChi - currentChi) * 1e3 < iniChi) stalled++;
            else stalled = 0;
            terminate = stalled >= 3;
        }
        if (trace) {
            orbo_step s;
            s.chi_in = iniChi;
            s.chi_out = currentChi;
            s.lambda = lambda;
            s.trials = qmax;
            s.status = terminate ? 1 : 0;
            trace[it] = s;
        }
        res.iters = it + 1;
        res.chi_last = currentChi;
        res.lambda = lambda;
        res.status = terminate ? ORBB_RUN_TERMINATE : ORBB_RUN_OK;
        ok = !terminate;
    }
    return ORBX_OK;
}

}  // namespace orbb
