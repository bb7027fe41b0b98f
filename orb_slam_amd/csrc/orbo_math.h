// The arithmetic of the motion-only pose optimisation (include/orbo.h states it): g2o's Levenberg iteration over one SE3 vertex as
// Optimizer::PoseOptimization uses it.  One text for the device (orbo_pose.hip), the host route (tools/poseopt_host_route.cpp) and
// tests/_probe/poseopt_host.cpp.  Everything is double; every array has compile-time indices and lives in registers.  The one thing the two sides
// do differently is how the 64 lane sums meet, and that is behind `Sys` (the same order on both).  Compile with -ffp-contract=off.
//
// The steps NOT pinned to Eigen are quat_from_matrix (Quaterniond(R)) and ldlt_solve (LinearSolverDense).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "orb_jacobi.h"
#include "orbo.h"

#if defined(__HIPCC__)
#define ORBO_NOUNROLL _Pragma("nounroll")
#else
#define ORBO_NOUNROLL
#endif

namespace orbo {

constexpr int LANES = 64;
constexpr int NACC = 28;                                    // 21 upper entries of H row by row, 6 of b, chi
// Optimizer.cc:243 and a round's first record of the trace (selects, not tables: a table indexed by the round would live in memory)
ORB_HD int round_iters(int r) { return r < 2 ? 10 : r == 2 ? 7 : 5; }
ORB_HD int round_slot(int r) { return r == 0 ? 0 : r == 1 ? 10 : r == 2 ? 20 : 27; }

struct Pose { double q[4], t[3]; };                         // x y z w
struct Cam { double fx, fy, cx, cy; };
struct Edge { double X, Y, Z, u, v, w; };                   // w: invSigma2

// a lane's outlier flags: bit k is edge lane + 64*k (k < ORBO_MAX_EDGES/64 = 128)
struct Flags {
    uint64_t lo = 0, hi = 0;
    ORB_HD bool get(int k) const { return (((k < 64) ? lo : hi) >> (k & 63)) & 1; }
    ORB_HD void set(int k, bool b) {
        const uint64_t m = (uint64_t)1 << (k & 63);
        if (k < 64) lo = b ? (lo | m) : (lo & ~m);
        else hi = b ? (hi | m) : (hi & ~m);
    }
};

// the Huber kernel's two constants: `const float delta = sqrt(5.991)` (Optimizer.cc:189) and the kernel's float member dsqr
ORB_HD double huber_delta() { return (double)(float)sqrt(5.991); }
ORB_HD double huber_dsqr() { const double d = huber_delta(); return (double)(float)(d * d); }
// `const float chi2[4]` (Optimizer.cc:242)
ORB_HD double round_threshold(int r) { return r == 0 ? (double)9.210f : r == 1 ? (double)7.378f : (double)5.991f; }

// SE3Quat::normalizeRotation (se3quat.h:280-285)
ORB_HD void normalize_rotation(double (&q)[4]) {
    if (q[3] < 0) {
ORB_UNROLL
        for (int i = 0; i < 4; i++) q[i] = q[i] * -1.0;
    }
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
ORB_UNROLL
    for (int i = 0; i < 4; i++) q[i] = q[i] / nrm;
}

// Quaterniond(R): NOT pinned to Eigen (orbo.h, step 1)
ORB_HD void quat_from_matrix(const double (&R)[3][3], double (&q)[4]) {
    const double tr = (R[0][0] + R[1][1]) + R[2][2];
    if (tr > 0) {
        double s = sqrt(tr + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (R[2][1] - R[1][2]) * s;
        q[1] = (R[0][2] - R[2][0]) * s;
        q[2] = (R[1][0] - R[0][1]) * s;
        return;
    }
    int i = 0;
    if (R[1][1] > R[0][0]) i = 1;
    if (R[2][2] > (i == 1 ? R[1][1] : R[0][0])) i = 2;
    if (i == 0) {
        double s = sqrt(((R[0][0] - R[1][1]) - R[2][2]) + 1.0);
        q[0] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (R[2][1] - R[1][2]) * s;
        q[1] = (R[1][0] + R[0][1]) * s;
        q[2] = (R[2][0] + R[0][2]) * s;
    } else if (i == 1) {
        double s = sqrt(((R[1][1] - R[2][2]) - R[0][0]) + 1.0);
        q[1] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (R[0][2] - R[2][0]) * s;
        q[2] = (R[2][1] + R[1][2]) * s;
        q[0] = (R[0][1] + R[1][0]) * s;
    } else {
        double s = sqrt(((R[2][2] - R[0][0]) - R[1][1]) + 1.0);
        q[2] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (R[1][0] - R[0][1]) * s;
        q[0] = (R[0][2] + R[2][0]) * s;
        q[1] = (R[1][2] + R[2][1]) * s;
    }
}

// Converter::toSE3Quat (Converter.cc:38-48): the rows of the float [R | t]
ORB_HD void pose_from_Tcw(const float* T, Pose& P) {
    double R[3][3];
ORB_UNROLL
    for (int r = 0; r < 3; r++) {
ORB_UNROLL
        for (int c = 0; c < 3; c++) R[r][c] = (double)T[r * 4 + c];
        P.t[r] = (double)T[r * 4 + 3];
    }
    quat_from_matrix(R, P.q);
    normalize_rotation(P.q);
}

// q*X
ORB_HD void rotate(const double (&q)[4], double X, double Y, double Z, double (&o)[3]) {
    double u0 = q[1] * Z - q[2] * Y, u1 = q[2] * X - q[0] * Z, u2 = q[0] * Y - q[1] * X;
    u0 = u0 + u0;
    u1 = u1 + u1;
    u2 = u2 + u2;
    o[0] = (X + q[3] * u0) + (q[1] * u2 - q[2] * u1);
    o[1] = (Y + q[3] * u1) + (q[2] * u0 - q[0] * u2);
    o[2] = (Z + q[3] * u2) + (q[0] * u1 - q[1] * u0);
}

// toRotationMatrix (orbo.h, output)
ORB_HD void rotation_matrix(const double (&q)[4], double (&R)[3][3]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0][0] = 1.0 - (tyy + tzz);
    R[0][1] = txy - twz;
    R[0][2] = txz + twy;
    R[1][0] = txy + twz;
    R[1][1] = 1.0 - (txx + tzz);
    R[1][2] = tyz - twx;
    R[2][0] = txz - twy;
    R[2][1] = tyz + twx;
    R[2][2] = 1.0 - (txx + tyy);
}

// to_homogeneous_matrix (se3quat.h:270-278) narrowed to float
ORB_HD void pose_to_Tcw(const Pose& P, float (&T)[16]) {
    double R[3][3];
    rotation_matrix(P.q, R);
ORB_UNROLL
    for (int r = 0; r < 3; r++)
ORB_UNROLL
        for (int c = 0; c < 3; c++) T[r * 4 + c] = (float)R[r][c];
    T[3] = (float)P.t[0];
    T[7] = (float)P.t[1];
    T[11] = (float)P.t[2];
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

// computeError (types_six_dof_expmap.h:88, .cpp:136-142): the camera point p, the error e; returns chi2
ORB_HD double edge_error(const Cam& c, const Pose& P, const Edge& E, double (&p)[3], double (&e)[2]) {
    rotate(P.q, E.X, E.Y, E.Z, p);
ORB_UNROLL
    for (int i = 0; i < 3; i++) p[i] = p[i] + P.t[i];
    e[0] = E.u - ((p[0] / p[2]) * c.fx + c.cx);
    e[1] = E.v - ((p[1] / p[2]) * c.fy + c.cy);
    return E.w * (e[0] * e[0] + e[1] * e[1]);
}
ORB_HD double edge_chi2(const Cam& c, const Pose& P, const Edge& E) {
    double p[3], e[2];
    return edge_error(c, P, E, p, e);
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]
// (delta and dsqr as arguments: the bundle adjustment of orbb_math.h takes its delta from the caller)
ORB_HD void huber(double chi2, double delta, double dsqr, double& rho0, double& rho1) {
    if (chi2 <= dsqr) {
        rho0 = chi2;
        rho1 = 1.0;
    } else {
        const double s = sqrt(chi2);
        rho0 = (2 * s) * delta - dsqr;
        rho1 = delta / s;
    }
}
ORB_HD void huber(double chi2, double& rho0, double& rho1) { huber(chi2, huber_delta(), huber_dsqr(), rho0, rho1); }

// the Jacobian of the error by the pose (linearizeOplus, .cpp:121-133) at the camera point p
ORB_HD void pose_jacobian(const Cam& c, const double (&p)[3], double (&J)[2][6]) {
    const double x = p[0], y = p[1], z = p[2], z2 = z * z;
    J[0][0] = ((x * y) / z2) * c.fx;
    J[0][1] = (-(1.0 + (x * x) / z2)) * c.fx;
    J[0][2] = (y / z) * c.fx;
    J[0][3] = (-1.0 / z) * c.fx;
    J[0][4] = 0.0;
    J[0][5] = (x / z2) * c.fx;
    J[1][0] = (1.0 + (y * y) / z2) * c.fy;
    J[1][1] = (((-x) * y) / z2) * c.fy;
    J[1][2] = ((-x) / z) * c.fy;
    J[1][3] = 0.0;
    J[1][4] = (-1.0 / z) * c.fy;
    J[1][5] = (y / z2) * c.fy;
}

// one edge into a lane's sums: linearizeOplus (.cpp:97-134) and constructQuadraticForm (base_binary_edge.hpp:91-113)
ORB_HD void add_edge(const Cam& c, const Pose& P, const Edge& E, double delta, double dsqr, double (&acc)[NACC]) {
    double p[3], e[2];
    const double chi2 = edge_error(c, P, E, p, e);
    double rho0, rho1;
    huber(chi2, delta, dsqr, rho0, rho1);
    double J[2][6];
    pose_jacobian(c, p, J);
    const double wr = E.w * rho1;
    const double r0 = ((-E.w) * e[0]) * rho1, r1 = ((-E.w) * e[1]) * rho1;
    int a = 0;
ORB_UNROLL
    for (int i = 0; i < 6; i++)
ORB_UNROLL
        for (int j = i; j < 6; j++, a++) acc[a] = acc[a] + ((J[0][i] * wr) * J[0][j] + (J[1][i] * wr) * J[1][j]);
ORB_UNROLL
    for (int i = 0; i < 6; i++) acc[21 + i] = acc[21 + i] + (J[0][i] * r0 + J[1][i] * r1);
    acc[27] = acc[27] + rho0;
}
ORB_HD void add_edge(const Cam& c, const Pose& P, const Edge& E, double (&acc)[NACC]) { add_edge(c, P, E, huber_delta(), huber_dsqr(), acc); }

// what a lane sums: its active edges lane, lane + 64, ... in index order.  load(i) is edge i.
template <class Load>
ORB_HD void lane_full(const Load& load, const Cam& c, const Pose& P, int n, int lane, const Flags& f, double (&acc)[NACC]) {
ORB_UNROLL
    for (int a = 0; a < NACC; a++) acc[a] = 0.0;
    for (int i = lane, k = 0; i < n; i += LANES, k++)
        if (!f.get(k)) add_edge(c, P, load(i), acc);
}
template <class Load>
ORB_HD double lane_chi(const Load& load, const Cam& c, const Pose& P, int n, int lane, const Flags& f) {
    double chi = 0.0;
    for (int i = lane, k = 0; i < n; i += LANES, k++)
        if (!f.get(k)) {
            double rho0, rho1;
            huber(edge_chi2(c, P, load(i)), rho0, rho1);
            chi = chi + rho0;
        }
    return chi;
}

// one edge's classification (Optimizer.cc:252-272): the chi2 of the error it last computed against the round's threshold
template <class Load>
ORB_HD void classify_edge(const Load& load, const Cam& c, const Pose& est, const Pose& last, double th, int i, bool& outlier, bool& bad) {
    const double chi2 = edge_chi2(c, outlier ? est : last, load(i));
    bad = false;
    if (chi2 > th) {
        outlier = true;
        bad = true;
    } else if (chi2 <= th) {
        outlier = false;
    }
}

// LinearSolverDense on (H + lambda*I) x = b: NOT pinned to Eigen (orbo.h, step 2).  x is written only when the solve succeeds.
// Dimension N: acc holds the N*(N + 1)/2 upper entries of H row by row, then the N of b (6 here, 7 for the similarity of orbg_math.h).
template <int N, int NA>
ORB_HD bool ldlt_solve_n(const double (&acc)[NA], double lambda, double (&x)[N]) {
    constexpr int NB = N * (N + 1) / 2;
    double A[N][N], L[N][N], d[N];
    int a = 0;
ORB_UNROLL
    for (int i = 0; i < N; i++)
ORB_UNROLL
        for (int j = i; j < N; j++, a++) A[j][i] = (i == j) ? acc[a] + lambda : acc[a];      // the lower triangle
    bool ok = true;
ORB_UNROLL
    for (int j = 0; j < N; j++) {
        double s = A[j][j];
ORB_UNROLL
        for (int k = 0; k < j; k++) s = s - (L[j][k] * L[j][k]) * d[k];
        d[j] = s;
        if (s < 0 || !__builtin_isfinite(s)) ok = false;
ORB_UNROLL
        for (int i = j + 1; i < N; i++) {
            double t = A[i][j];
ORB_UNROLL
            for (int k = 0; k < j; k++) t = t - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = t / s;
        }
    }
    if (!ok) return false;
    double y[N];
ORB_UNROLL
    for (int i = 0; i < N; i++) {
        double s = acc[NB + i];
ORB_UNROLL
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s;
    }
ORB_UNROLL
    for (int i = 0; i < N; i++) y[i] = y[i] / d[i];
ORB_UNROLL
    for (int i = N - 1; i >= 0; i--) {
        double s = y[i];
ORB_UNROLL
        for (int k = i + 1; k < N; k++) s = s - L[k][i] * x[k];
        x[i] = s;
    }
    return true;
}
ORB_HD bool ldlt_solve(const double (&acc)[NACC], double lambda, double (&x)[6]) { return ldlt_solve_n<6, NACC>(acc, lambda, x); }

ORB_HD double dot3(double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// VertexSE3Expmap::oplusImpl: SE3Quat::exp(x)*estimate (se3quat.h:223-257, :104-110)
ORB_HD void exp_update(const double (&x)[6], const Pose& est, Pose& out) {
    const double o0 = x[0], o1 = x[1], o2 = x[2];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double O[3][3] = {{0.0, -o2, o1}, {o2, 0.0, -o0}, {-o1, o0, 0.0}};
    double O2[3][3], R[3][3], V[3][3];
ORB_UNROLL
    for (int i = 0; i < 3; i++)
ORB_UNROLL
        for (int j = 0; j < 3; j++) O2[i][j] = dot3(O[i][0], O[0][j], O[i][1], O[1][j], O[i][2], O[2][j]);
    if (theta < 0.00001) {
ORB_UNROLL
        for (int i = 0; i < 3; i++)
ORB_UNROLL
            for (int j = 0; j < 3; j++) V[i][j] = R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {
        const double sn = sin(theta), cs = cos(theta);
        const double ka = sn / theta, kb = (1.0 - cs) / (theta * theta), kc = (theta - sn) / pow(theta, 3.0);
ORB_UNROLL
        for (int i = 0; i < 3; i++)
ORB_UNROLL
            for (int j = 0; j < 3; j++) {
                const double id = i == j ? 1.0 : 0.0;
                R[i][j] = (id + ka * O[i][j]) + kb * O2[i][j];
                V[i][j] = (id + kb * O[i][j]) + kc * O2[i][j];
            }
    }
    double qe[4], te[3], rt[3];
    quat_from_matrix(R, qe);
    normalize_rotation(qe);
ORB_UNROLL
    for (int i = 0; i < 3; i++) te[i] = dot3(V[i][0], x[3], V[i][1], x[4], V[i][2], x[5]);
    rotate(qe, est.t[0], est.t[1], est.t[2], rt);
ORB_UNROLL
    for (int i = 0; i < 3; i++) out.t[i] = te[i] + rt[i];
    const double ax = qe[0], ay = qe[1], az = qe[2], aw = qe[3], bx = est.q[0], by = est.q[1], bz = est.q[2], bw = est.q[3];
    out.q[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    out.q[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    out.q[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
    out.q[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
    normalize_rotation(out.q);
}

ORB_HD orbo_step step_not_run() {
    orbo_step s;
    s.chi_in = s.chi_out = s.lambda = 0.0;
    s.trials = 0;
    s.status = 2;
    return s;
}

// Optimizer::PoseOptimization from `vSE3->setEstimate` on (Optimizer.cc:172, :242-284).  Sys is one frame's edges with their flags:
//   full(P, acc)   the 28 sums over the active edges at P, in the ABI's order
//   chi(P)         the robust chi2 sum alone
//   classify(est, last, th, nbad, nout)   Optimizer.cc:252-272 over every edge; nout: the outlier flags set afterwards
//   step(slot, s)  one record of the trace
//   u(v)           v itself; on the device every lane runs this with the same values, and u() says so for the values that live long (the estimate,
//                  the last trial, x, the sums, lambda), which then wait in scalar registers while the lanes walk the edges
template <class Sys> ORB_HD void uniform_pose(Sys& sys, Pose& P) {
ORB_UNROLL
    for (int i = 0; i < 4; i++) P.q[i] = sys.u(P.q[i]);
ORB_UNROLL
    for (int i = 0; i < 3; i++) P.t[i] = sys.u(P.t[i]);
}
template <class Sys>
ORB_HD void pose_optimization(Sys& sys, int n, const float* Tcw, orbo_result& res) {
    Pose est, last;
    pose_from_Tcw(Tcw, est);
    uniform_pose(sys, est);
    last = est;
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int nbad = 0, nout = 0, rounds = 0;
ORB_UNROLL
    for (int r = 0; r < ORBO_ROUNDS; r++) res.iters[r] = 0;
ORBO_NOUNROLL
    for (int r = 0; r < ORBO_ROUNDS; r++) {
        int done = 0;
        bool ok = n - nout > 0;                                                     // sparse_optimizer.cpp:356-359
        double lambda = 0.0, ni = 2.0;
        int stalled = 0;                                                            // _nBad
ORBO_NOUNROLL
        for (int it = 0; it < round_iters(r); it++) {
            if (!ok) {
                sys.step(round_slot(r) + it, step_not_run());
                continue;
            }
            double acc[NACC];
            sys.full(est, acc);
ORB_UNROLL
            for (int a = 0; a < NACC; a++) acc[a] = sys.u(acc[a]);
            double currentChi = acc[27], tempChi = currentChi;
            const double iniChi = currentChi;
            if (it == 0) {                                                          // computeLambdaInit (:166-180)
                double maxDiagonal = 0.0;
                int a = 0;
ORB_UNROLL
                for (int j = 0; j < 6; a += 6 - j, j++) {
                    const double h = fabs(acc[a]);
                    maxDiagonal = (h < maxDiagonal) ? maxDiagonal : h;              // std::max(fabs(h), maxDiagonal)
                }
                lambda = sys.u(1e-5 * maxDiagonal);
                ni = 2.0;
                stalled = 0;
            }
            double rho = 0.0;
            int qmax = 0;
ORBO_NOUNROLL
            do {
                const bool ok2 = ldlt_solve(acc, lambda, x);
ORB_UNROLL
                for (int j = 0; j < 6; j++) x[j] = sys.u(x[j]);
                Pose trial;
                exp_update(x, est, trial);
                uniform_pose(sys, trial);
                tempChi = sys.u(sys.chi(trial));
                last = trial;
                if (!ok2) tempChi = DBL_MAX;
                rho = currentChi - tempChi;
                double scale = 0.0;
ORB_UNROLL
                for (int j = 0; j < 6; j++) scale = scale + x[j] * (lambda * x[j] + acc[21 + j]);
                scale = scale + 1e-3;
                rho = rho / scale;
                if (rho > 0 && __builtin_isfinite(tempChi)) {
                    const double c = 2 * rho - 1;
                    double alpha = 1.0 - (c * c) * c;
                    const double upper = 2.0 / 3.0, lower = 1.0 / 3.0;
                    alpha = (upper < alpha) ? upper : alpha;                        // std::min(alpha, _goodStepUpperScale)
                    const double scaleFactor = (lower < alpha) ? alpha : lower;     // std::max(_goodStepLowerScale, alpha)
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
            sys.step(round_slot(r) + it, s);
            done++;
            ok = !terminate;
        }
ORB_UNROLL
        for (int r2 = 0; r2 < ORBO_ROUNDS; r2++)
            if (r2 == r) res.iters[r2] = done;
        sys.classify(est, last, round_threshold(r), nbad, nout);
        rounds++;
        if (n < 10) {
            for (int slot = round_slot(r) + round_iters(r); slot < ORBO_MAX_ITERS; slot++) sys.step(slot, step_not_run());
            break;
        }
    }
    pose_to_Tcw(est, res.Tcw);
ORB_UNROLL
    for (int i = 0; i < 4; i++) res.q[i] = est.q[i];
ORB_UNROLL
    for (int i = 0; i < 3; i++) res.t[i] = est.t[i];
    res.ninitial = n;
    res.nbad = nbad;
    res.rounds = rounds;
    res.noutlier = nout;
}

}  // namespace orbo
