// The arithmetic of loop closing's Sim3 refinement (include/orbg.h states it): g2o's Levenberg iteration over one 7-dof similarity vertex as
// Optimizer::OptimizeSim3 uses it, with the numeric Jacobian of BaseBinaryEdge::linearizeOplus.  One text for the device (orbg_sim3.hip), the host
// route (tools/sim3opt_host_route.cpp) and tests/_probe/sim3opt_host.cpp, over orbo_math.h: Huber, q*X, Quaterniond(R), toRotationMatrix, the flags,
// the LDL' (ldlt_solve_n at dimension 7) and the trace record are that file's.  Everything is double.  What the two sides do differently is how the
// 64 lane sums meet and where the thirty similarities of a linearisation wait, and that is behind `Sys`.  Compile with -ffp-contract=off.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "orbg.h"
#include "orbo_math.h"

namespace orbg {

using orbo::Flags;
using orbo::LANES;
using orbo::dot3;

constexpr int DIM = 7;
constexpr int NH = 28;                                      // upper entries of H row by row
constexpr int NACC = 36;                                    // H, 7 of b, chi
// the similarities of one linearisation: slot 2*d is Sim3(+1e-9*e_d)*S, slot 2*d + 1 is Sim3(-1e-9*e_d)*S, slot 14 is S; slot NSIM + k is the
// inverse of slot k
constexpr int NSIM = 15;
constexpr int PHASE1_ITERS = 5;                             // Optimizer.cc:928

struct Sim3 { double q[4], t[3], s; };                      // x y z w
struct Cam { double fx, fy, cx, cy; };
struct Pair { double P1[3], P2[3], u1, v1, w1, u2, v2, w2; };

// Sim3(R, t, s) (sim3.h:64-67) of the float arguments of LoopClosing.cc:320: Quaterniond(R), not normalised
ORB_HD void sim3_from_float(const float* S12, Sim3& S) {
    double R[3][3];
ORB_UNROLL
    for (int r = 0; r < 3; r++) {
ORB_UNROLL
        for (int c = 0; c < 3; c++) R[r][c] = (double)S12[r * 3 + c];
        S.t[r] = (double)S12[9 + r];
    }
    orbo::quat_from_matrix(R, S.q);
    S.s = (double)S12[12];
}

// Eigen's Hamilton product a*b as orbo.h writes it
ORB_HD void quat_mul(const double (&a)[4], const double (&b)[4], double (&o)[4]) {
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    o[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    o[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    o[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
    o[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
}

// Sim3::operator* (sim3.h:266-272)
ORB_HD void sim3_mul(const Sim3& a, const Sim3& b, Sim3& o) {
    double r[3];
    orbo::rotate(a.q, b.t[0], b.t[1], b.t[2], r);
    quat_mul(a.q, b.q, o.q);
ORB_UNROLL
    for (int i = 0; i < 3; i++) o.t[i] = a.s * r[i] + a.t[i];
    o.s = a.s * b.s;
}

// Sim3::inverse (sim3.h:233-236)
ORB_HD void sim3_inverse(const Sim3& a, Sim3& o) {
    o.q[0] = -a.q[0];
    o.q[1] = -a.q[1];
    o.q[2] = -a.q[2];
    o.q[3] = a.q[3];
    const double m = -1.0 / a.s;
    orbo::rotate(o.q, m * a.t[0], m * a.t[1], m * a.t[2], o.t);
    o.s = 1.0 / a.s;
}

// Sim3(update) (sim3.h:70-142), all four branches
ORB_HD void sim3_exp(const double (&x)[DIM], Sim3& out) {
    const double o0 = x[0], o1 = x[1], o2 = x[2], sigma = x[6];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double O[3][3] = {{0.0, -o2, o1}, {o2, 0.0, -o0}, {-o1, o0, 0.0}};
    double O2[3][3], R[3][3];
ORB_UNROLL
    for (int i = 0; i < 3; i++)
ORB_UNROLL
        for (int j = 0; j < 3; j++) O2[i][j] = dot3(O[i][0], O[0][j], O[i][1], O[1][j], O[i][2], O[2][j]);
    const double s = exp(sigma);
    const double eps = 0.00001;
    const bool small = theta < eps;
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta), b = s * cos(theta);
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2;
        }
    }
    if (small) {
ORB_UNROLL
        for (int i = 0; i < 3; i++)
ORB_UNROLL
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {
        const double ka = sin(theta) / theta, kb = (1.0 - cos(theta)) / (theta * theta);
ORB_UNROLL
        for (int i = 0; i < 3; i++)
ORB_UNROLL
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + ka * O[i][j]) + kb * O2[i][j];
    }
    orbo::quat_from_matrix(R, out.q);
    double W[3][3];
ORB_UNROLL
    for (int i = 0; i < 3; i++)
ORB_UNROLL
        for (int j = 0; j < 3; j++) W[i][j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);
ORB_UNROLL
    for (int i = 0; i < 3; i++) out.t[i] = dot3(W[i][0], x[3], W[i][1], x[4], W[i][2], x[5]);
    out.s = s;
}

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69, _fix_scale false): Sim3(update)*estimate
ORB_HD void oplus(const double (&x)[DIM], const Sim3& est, Sim3& out) {
    Sim3 e;
    sim3_exp(x, e);
    sim3_mul(e, est, out);
}

// slot k of a linearisation (base_binary_edge.hpp:147-173): the vertex after oplus(+-1e-9*e_d), or the estimate itself (k == 14).  The update is
// built with selects so that k may differ between the lanes of a wave.
ORB_HD void perturbed(const Sim3& est, int k, Sim3& out) {
    if (k >= NSIM - 1) {
        out = est;
        return;
    }
    const double delta = 1e-9;
    const double v = (k & 1) ? -delta : delta;
    double x[DIM];
ORB_UNROLL
    for (int j = 0; j < DIM; j++) x[j] = ((k >> 1) == j) ? v : 0.0;
    oplus(x, est, out);
}

// computeError of either edge (types_seven_dof_expmap.h:138-145, :160-167): obs - cam_map(project(S.map(X))); S is the estimate for edge 12 and
// its inverse for edge 21
ORB_HD void edge_error(const Sim3& S, const Cam& c, const double (&X)[3], double u, double v, double (&e)[2]) {
    double p[3];
    orbo::rotate(S.q, X[0], X[1], X[2], p);
ORB_UNROLL
    for (int i = 0; i < 3; i++) p[i] = S.s * p[i] + S.t[i];
    e[0] = u - ((p[0] / p[2]) * c.fx + c.cx);
    e[1] = v - ((p[1] / p[2]) * c.fy + c.cy);
}
ORB_HD double edge_chi2(const Sim3& S, const Cam& c, const double (&X)[3], double u, double v, double w) {
    double e[2];
    edge_error(S, c, X, u, v, e);
    return w * (e[0] * e[0] + e[1] * e[1]);
}

// one edge into a lane's sums: the numeric linearizeOplus (base_binary_edge.hpp:130-205) over the fifteen similarities sims[0 .. NSIM) and
// constructQuadraticForm (:91-113).  Columns first, products second: the loop over the columns stays a loop (fifteen unrolled projections keep
// every similarity in registers at once) and hands the 2 x 7 Jacobian over through jb, a lane's own fourteen doubles wherever Sys keeps them:
// jb.put(2*d + r, v), jb.get(2*d + r).
template <class JB>
ORB_HD void add_edge(const Sim3* sims, const Cam& c, const double (&X)[3], double u, double v, double w, double delta, double dsqr, JB& jb,
                     double (&acc)[NACC]) {
    const double scalar = 1.0 / (2 * 1e-9);
ORBO_NOUNROLL
    for (int d = 0; d < DIM; d++) {
        double ep[2], em[2];
        edge_error(sims[2 * d], c, X, u, v, ep);
        edge_error(sims[2 * d + 1], c, X, u, v, em);
        jb.put(2 * d, scalar * (ep[0] - em[0]));
        jb.put(2 * d + 1, scalar * (ep[1] - em[1]));
    }
    double e[2];
    edge_error(sims[NSIM - 1], c, X, u, v, e);
    const double chi2 = w * (e[0] * e[0] + e[1] * e[1]);
    double rho0, rho1;
    orbo::huber(chi2, delta, dsqr, rho0, rho1);
    const double wr = w * rho1;
    const double r0 = ((-w) * e[0]) * rho1, r1 = ((-w) * e[1]) * rho1;
    double J[2][DIM];
ORB_UNROLL
    for (int d = 0; d < DIM; d++) {
        J[0][d] = jb.get(2 * d);
        J[1][d] = jb.get(2 * d + 1);
    }
    int a = 0;
ORB_UNROLL
    for (int i = 0; i < DIM; i++)
ORB_UNROLL
        for (int j = i; j < DIM; j++, a++) acc[a] = acc[a] + ((J[0][i] * wr) * J[0][j] + (J[1][i] * wr) * J[1][j]);
ORB_UNROLL
    for (int i = 0; i < DIM; i++) acc[NH + i] = acc[NH + i] + (J[0][i] * r0 + J[1][i] * r1);
    acc[NACC - 1] = acc[NACC - 1] + rho0;
}

// what a lane sums: its active pairs lane, lane + 64, ... in index order, edge 12 before edge 21.  load(i) is pair i; sims holds the 2*NSIM
// similarities of the linearisation.
template <class Load, class JB>
ORB_HD void lane_full(const Load& load, const Sim3* sims, const Cam& c1, const Cam& c2, double delta, double dsqr, int n, int lane, const Flags& f,
                      JB& jb, double (&acc)[NACC]) {
ORB_UNROLL
    for (int a = 0; a < NACC; a++) acc[a] = 0.0;
    for (int i = lane, k = 0; i < n; i += LANES, k++)
        if (!f.get(k)) {
            const Pair P = load(i);
            add_edge(sims, c1, P.P2, P.u1, P.v1, P.w1, delta, dsqr, jb, acc);
            add_edge(sims + NSIM, c2, P.P1, P.u2, P.v2, P.w2, delta, dsqr, jb, acc);
        }
}
template <class Load>
ORB_HD double lane_chi(const Load& load, const Sim3& S, const Sim3& Si, const Cam& c1, const Cam& c2, double delta, double dsqr, int n, int lane,
                       const Flags& f) {
    double chi = 0.0;
    for (int i = lane, k = 0; i < n; i += LANES, k++)
        if (!f.get(k)) {
            const Pair P = load(i);
            double rho0, rho1;
            orbo::huber(edge_chi2(S, c1, P.P2, P.u1, P.v1, P.w1), delta, dsqr, rho0, rho1);
            chi = chi + rho0;
            orbo::huber(edge_chi2(Si, c2, P.P1, P.u2, P.v2, P.w2), delta, dsqr, rho0, rho1);
            chi = chi + rho0;
        }
    return chi;
}

// the test of Optimizer.cc:939 and :973 on the errors the two edges last computed (at `last` and its inverse); a NaN chi2 fails both comparisons
template <class Load>
ORB_HD bool pair_is_bad(const Load& load, const Sim3& last, const Sim3& lasti, const Cam& c1, const Cam& c2, double th2, int i) {
    const Pair P = load(i);
    const double chi12 = edge_chi2(last, c1, P.P2, P.u1, P.v1, P.w1), chi21 = edge_chi2(lasti, c2, P.P1, P.u2, P.v2, P.w2);
    return chi12 > th2 || chi21 > th2;
}

template <class Sys> ORB_HD void uniform_sim3(Sys& sys, Sim3& S) {
ORB_UNROLL
    for (int i = 0; i < 4; i++) S.q[i] = sys.u(S.q[i]);
ORB_UNROLL
    for (int i = 0; i < 3; i++) S.t[i] = sys.u(S.t[i]);
    S.s = sys.u(S.s);
}

// SparseOptimizer::optimize(maxit) with OptimizationAlgorithmLevenberg::solve (orbo.h's text at dimension 7) over the active pairs.  Sys:
//   linearise(S)   the 2*NSIM similarities of a linearisation at S, wherever the lanes read them from
//   full(acc)      the 36 sums over the active pairs at the last linearise(), in the ABI's order
//   chi(S, Si)     the robust chi2 sum alone at S (Si its inverse)
//   step(slot, s)  one record of the trace
//   u(v)           v itself; on the device, says that every lane holds the same value (orbo_math.h)
// Returns the outer iterations made; `last` is the vertex at which the edges last computed their errors.
template <class Sys>
ORB_HD int optimize(Sys& sys, bool any, int maxit, int slot0, Sim3& est, Sim3& last, double (&x)[DIM]) {
    int done = 0;
    bool ok = any;                                                                  // sparse_optimizer.cpp:356-359
    double lambda = 0.0, ni = 2.0;
    int stalled = 0;                                                                // _nBad
ORBO_NOUNROLL
    for (int it = 0; it < maxit; it++) {
        if (!ok) {
            sys.step(slot0 + it, orbo::step_not_run());
            continue;
        }
        double acc[NACC];
        sys.linearise(est);
        sys.full(acc);                                                              // every lane holds the same bits; the sums are not
                                                                                    // named uniform: 72 scalar registers are more than are free
        double currentChi = acc[NACC - 1], tempChi = currentChi;
        const double iniChi = currentChi;
        if (it == 0) {                                                              // computeLambdaInit (:166-180)
            double maxDiagonal = 0.0;
            int a = 0;
ORB_UNROLL
            for (int j = 0; j < DIM; a += DIM - j, j++) {
                const double h = fabs(acc[a]);
                maxDiagonal = (h < maxDiagonal) ? maxDiagonal : h;                  // std::max(fabs(h), maxDiagonal)
            }
            lambda = sys.u(1e-5 * maxDiagonal);
            ni = 2.0;
            stalled = 0;
        }
        double rho = 0.0;
        int qmax = 0;
ORBO_NOUNROLL
        do {
            const bool ok2 = orbo::ldlt_solve_n<DIM, NACC>(acc, lambda, x);
ORB_UNROLL
            for (int j = 0; j < DIM; j++) x[j] = sys.u(x[j]);
            Sim3 trial, triali;
            oplus(x, est, trial);
            uniform_sim3(sys, trial);
            sim3_inverse(trial, triali);
            uniform_sim3(sys, triali);
            tempChi = sys.u(sys.chi(trial, triali));
            last = trial;
            if (!ok2) tempChi = DBL_MAX;
            rho = currentChi - tempChi;
            double scale = 0.0;
ORB_UNROLL
            for (int j = 0; j < DIM; j++) scale = scale + x[j] * (lambda * x[j] + acc[NH + j]);
            scale = scale + 1e-3;
            rho = rho / scale;
            if (rho > 0 && __builtin_isfinite(tempChi)) {
                const double c = 2 * rho - 1;
                double alpha = 1.0 - (c * c) * c;
                const double upper = 2.0 / 3.0, lower = 1.0 / 3.0;
                alpha = (upper < alpha) ? upper : alpha;                            // std::min(alpha, _goodStepUpperScale)
                const double scaleFactor = (lower < alpha) ? alpha : lower;         // std::max(_goodStepLowerScale, alpha)
                lambda = sys.u(lambda * scaleFactor);
                ni = 2.0;
                currentChi = tempChi;
                est = trial;
            } else {
                lambda = sys.u(lambda * ni);
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
        orbo_step s;
        s.chi_in = iniChi;
        s.chi_out = currentChi;
        s.lambda = lambda;
        s.trials = qmax;
        s.status = terminate ? 1 : 0;
        sys.step(slot0 + it, s);
        done++;
        ok = !terminate;
    }
    return done;
}

// Converter::toCvMat(g2o::Sim3) (Converter.cc:56-62)
ORB_HD void sim3_to_float(const Sim3& S, float (&T)[16]) {
    double R[3][3];
    orbo::rotation_matrix(S.q, R);
ORB_UNROLL
    for (int r = 0; r < 3; r++) {
ORB_UNROLL
        for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)(S.s * R[r][c]);
        T[r * 4 + 3] = (float)S.t[r];
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

// Optimizer::OptimizeSim3 from `vSim3->setEstimate` on (Optimizer.cc:815, :927-986).  Besides what optimize() asks of it Sys has
//   check(last, lasti, th2, first)   Optimizer.cc:932-949 (first) or :966-980 over every pair not yet removed: sets the flags, returns how many
//                                    pairs the test removed
//   active()                         pairs not removed
template <class Sys>
ORB_HD void optimize_sim3(Sys& sys, int n, const float* S12, orbg_result& res) {
    Sim3 est, last, lasti;
    sim3_from_float(S12, est);
    uniform_sim3(sys, est);
    last = est;
    double x[DIM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    res.iters[0] = optimize(sys, n > 0, PHASE1_ITERS, 0, est, last, x);
    sim3_inverse(last, lasti);
    const int nbad = sys.check(last, lasti, true);
    const int more = nbad > 0 ? 10 : 5;
    const bool ret0 = n - nbad < 10;
    int nin = 0, it2 = 0;
    if (ret0) {
        for (int slot = PHASE1_ITERS; slot < ORBG_MAX_ITERS; slot++) sys.step(slot, orbo::step_not_run());
        sim3_from_float(S12, est);                                                  // g2oS12 untouched
    } else {
        it2 = optimize(sys, true, more, PHASE1_ITERS, est, last, x);
        for (int slot = PHASE1_ITERS + more; slot < ORBG_MAX_ITERS; slot++) sys.step(slot, orbo::step_not_run());
        sim3_inverse(last, lasti);
        nin = (n - nbad) - sys.check(last, lasti, false);
    }
    res.iters[1] = it2;
    sim3_to_float(est, res.S12);
ORB_UNROLL
    for (int i = 0; i < 4; i++) res.q[i] = est.q[i];
ORB_UNROLL
    for (int i = 0; i < 3; i++) res.t[i] = est.t[i];
    res.s = est.s;
    res.ncorr = n;
    res.nbad = nbad;
    res.nin = nin;
    res.ret0 = ret0 ? 1 : 0;
}

}  // namespace orbg
