// The arithmetic of the EPnP RANSAC (include/orbe.h states it), one text for the device (orbe_pnp.hip), the host route (tools/pnp_host_route.cpp)
// and tests/_probe/pnp_host.cpp.  Build with -ffp-contract=off.
//
// The fit is written against a context Cx that says which share of the parallel steps the caller owns: cx.tid / cx.stride spread the 64 partial
// sums and the small per-entry loops, cx.sync() separates the steps, cx.eig12() is the 12 x 12 decomposition.  On the host one "thread" with
// stride 1 runs every share in turn; on the device the workgroup's threads do, and every thread calls fit() (the barriers are uniform).  Either way
// every value is computed by the same operations in the same order.
#pragma once
#include <math.h>
#include <stdint.h>

#include "orb_jacobi.h"
#include "orbe.h"

namespace orbe {

constexpr int LANES = 64;             // partial sums of the fixed order
constexpr int NCHUNK = 36;            // the widest group of sums taken at once (three rows of M'M)

struct Cam { double fu, fv, uc, vc; };

// the correspondences of one fit: position k of the list names correspondence list[k]
struct Points {
    const float* p3d;
    const float* p2d;
    const uint16_t* list;
    int n;
};

// work arrays of one least-squares branch
struct Branch {
    double A[30], G[25], GV[25], g[5], x[5], betas[4];
    double ga[24], gb[6], gx[4], A1[4], A2[4];
};

// work arrays of one fit (LDS on the device) for at most MAXPART partial sums that are not zero: a fit over n correspondences needs min(n, 64), so the
// four-point fit takes WorkT<4> (9.1 KB) and Refine WorkT<64> (26.6 KB).  A row of partial sums is padded by one: the second step reads down a column.
template <int MAXPART>
struct WorkT {
    static constexpr int PS = MAXPART + 1;
    double part[NCHUNK * PS];
    double sums[NCHUNK];
    double S[144], V[144];
    double cws[4][3], cc[9], ci[9];
    double vecs[4][12];
    double l[60], rho[6];
    Branch br[3];
    double ccs[4][3], pc0[3], pw0[3], abt[9], U[9], w3[3], Vt[9];
    double Rs[3][9], ts[3][3], err[3];
    double S3[9], V3[9];
    int order[12];
};
using Work = WorkT<LANES>;
using Work4 = WorkT<4>;

struct HostCx {
    int tid = 0;
    static constexpr int stride = 1;
    void sync() {}
    void eig12(double* S, double* V) { orbj::sym_eig<12>(S, V); }
};

ORB_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ORB_HD double dist2(const double* a, const double* b) {
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// K sums over the n list positions in the fixed order of orbe.h: term(k, v) fills the K terms of position k.  PS: the stride of a row of `part`;
// min(n, 64) < PS.  Partial sums past min(n, 64) are zero, enter no sum and are not stored.
template <int K, int PS, class Cx, class Term>
ORB_HD void ordered_sums(Cx& cx, int n, double* part, double* out, Term term) {
    const int m = n < LANES ? n : LANES;
    for (int l = cx.tid; l < m; l += cx.stride) {
        double acc[K];
ORB_UNROLL
        for (int q = 0; q < K; q++) acc[q] = 0.0;
        for (int k = l; k < n; k += LANES) {
            double v[K];
            term(k, v);
ORB_UNROLL
            for (int q = 0; q < K; q++) acc[q] = acc[q] + v[q];
        }
ORB_UNROLL
        for (int q = 0; q < K; q++) part[q * PS + l] = acc[q];
    }
    cx.sync();
    for (int q = cx.tid; q < K; q += cx.stride) {
        double s = 0.0;
        for (int l = 0; l < m; l++) s = s + part[q * PS + l];
        out[q] = s;
    }
    cx.sync();
}

// eigen-decomposition of the symmetric k x k G (k = 3, 4, 5) in place, eigenvectors by column in GV
ORB_HD void sym_eig_k(double* G, double* GV, int k) {
    if (k == 3) orbj::sym_eig<3>(G, GV);
    else if (k == 4) orbj::sym_eig<4>(G, GV);
    else orbj::sym_eig<5>(G, GV);
}

// minimum-norm least-squares x of the rows x k system A x = b (orbe.h); G, GV, g: work arrays
ORB_HD void lsq(const double* A, const double* b, int rows, int k, double* G, double* GV, double* g, double* x) {
    for (int i = 0; i < k; i++) {
        for (int j = 0; j < k; j++) {
            double s = 0.0;
            for (int r = 0; r < rows; r++) s = s + A[r * k + i] * A[r * k + j];
            G[i * k + j] = s;
        }
        double s = 0.0;
        for (int r = 0; r < rows; r++) s = s + A[r * k + i] * b[r];
        g[i] = s;
    }
    sym_eig_k(G, GV, k);
    double lmax = G[0];
    for (int i = 1; i < k; i++)
        if (G[i * k + i] > lmax) lmax = G[i * k + i];
    for (int j = 0; j < k; j++) x[j] = 0.0;
    for (int i = 0; i < k; i++) {
        const double li = G[i * k + i];
        if (!(li > ORBE_LSQ_CUT * lmax)) continue;
        double d = 0.0;
        for (int s = 0; s < k; s++) d = d + GV[s * k + i] * g[s];
        d = d / li;
        for (int j = 0; j < k; j++) x[j] = x[j] + GV[j * k + i] * d;
    }
}

// the pseudo-inverse of the 3 x 3 A (row major) by the same rule, column by column
ORB_HD void pinv3(const double* A, double* G, double* GV, double* out) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int r = 0; r < 3; r++) s = s + A[r * 3 + i] * A[r * 3 + j];
            G[i * 3 + j] = s;
        }
    orbj::sym_eig<3>(G, GV);
    double lmax = G[0];
    for (int i = 1; i < 3; i++)
        if (G[i * 4] > lmax) lmax = G[i * 4];
    for (int e = 0; e < 9; e++) out[e] = 0.0;
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 3; i++) {
            const double li = G[i * 4];
            if (!(li > ORBE_LSQ_CUT * lmax)) continue;
            double d = 0.0;
            for (int s = 0; s < 3; s++) d = d + GV[s * 3 + i] * A[c * 3 + s];      // (A')[s][c] = A[c][s]
            d = d / li;
            for (int r = 0; r < 3; r++) out[r * 3 + c] = out[r * 3 + c] + GV[r * 3 + i] * d;
        }
}

// compute_L_6x10 (:761-801); v[i] = vecs + 12*i
ORB_HD void compute_L_6x10(const double* vecs, double* l_6x10) {
    for (int i = 0; i < 6; i++) {
        // the pair (a, b) of row i: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
        const int a = i < 3 ? 0 : i < 5 ? 1 : 2;
        const int b = i < 3 ? i + 1 : i < 5 ? i - 1 : 3;
        double dv[4][3];
        for (int k = 0; k < 4; k++)
            for (int c = 0; c < 3; c++) dv[k][c] = vecs[12 * k + 3 * a + c] - vecs[12 * k + 3 * b + c];
        double* row = l_6x10 + 10 * i;
        row[0] = dot3(dv[0], dv[0]);
        row[1] = 2.0f * dot3(dv[0], dv[1]);
        row[2] = dot3(dv[1], dv[1]);
        row[3] = 2.0f * dot3(dv[0], dv[2]);
        row[4] = 2.0f * dot3(dv[1], dv[2]);
        row[5] = dot3(dv[2], dv[2]);
        row[6] = 2.0f * dot3(dv[0], dv[3]);
        row[7] = 2.0f * dot3(dv[1], dv[3]);
        row[8] = 2.0f * dot3(dv[2], dv[3]);
        row[9] = dot3(dv[3], dv[3]);
    }
}

// find_betas_approx_1/2/3 (:668-759) for branch 0, 1, 2: the columns taken, the solve, the sign and branch logic
ORB_HD void find_betas(const double* l, const double* rho, int branch, Branch& w) {
    const int k = branch == 0 ? 4 : branch == 1 ? 3 : 5;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < k; j++) {
            const int col = branch == 0 ? (j == 0 ? 0 : j == 1 ? 1 : j == 2 ? 3 : 6) : j;
            w.A[i * k + j] = l[i * 10 + col];
        }
    lsq(w.A, rho, 6, k, w.G, w.GV, w.g, w.x);
    const double* b = w.x;
    double* betas = w.betas;
    if (branch == 0) {
        if (b[0] < 0) {
            betas[0] = sqrt(-b[0]);
            betas[1] = -b[1] / betas[0];
            betas[2] = -b[2] / betas[0];
            betas[3] = -b[3] / betas[0];
        } else {
            betas[0] = sqrt(b[0]);
            betas[1] = b[1] / betas[0];
            betas[2] = b[2] / betas[0];
            betas[3] = b[3] / betas[0];
        }
        return;
    }
    if (b[0] < 0) {
        betas[0] = sqrt(-b[0]);
        betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
    } else {
        betas[0] = sqrt(b[0]);
        betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = branch == 1 ? 0.0 : b[3] / betas[0];
    betas[3] = 0.0;
}

// compute_A_and_b_gauss_newton (:813-839)
ORB_HD void gn_A_and_b(const double* l_6x10, const double* rho, const double* betas, double* A, double* b) {
    for (int i = 0; i < 6; i++) {
        const double* rowL = l_6x10 + i * 10;
        double* rowA = A + i * 4;
        rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
        rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
        rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
        rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
        b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                         rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] + rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                         rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
    }
}

// qr_solve (:861-951) for the 6 x 4 system; false on the source's `eta == 0` return, X then stays as it was
ORB_HD bool qr_solve(double* pA, double* pb, double* pX, double* A1, double* A2) {
    const int nr = 6, nc = 4;
    for (int k = 0; k < nc; k++) {
        const int kk = k * nc + k;
        double eta = fabs(pA[kk]);
        for (int i = k + 1; i < nr; i++) {                       // as the source: it reads element (i - 1, k), so the last row is never looked at
            const double elt = fabs(pA[(i - 1) * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) {
            A1[k] = A2[k] = 0.0;
            return false;
        }
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) {
            pA[i * nc + k] *= inv_eta;
            sum += pA[i * nc + k] * pA[i * nc + k];
        }
        double sigma = sqrt(sum);
        if (pA[kk] < 0) sigma = -sigma;
        pA[kk] += sigma;
        A1[k] = sigma * pA[kk];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s = 0;
            for (int i = k; i < nr; i++) s += pA[i * nc + k] * pA[i * nc + j];
            const double tau = s / A1[k];
            for (int i = k; i < nr; i++) pA[i * nc + j] -= tau * pA[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {
        double tau = 0;
        for (int i = j; i < nr; i++) tau += pA[i * nc + j] * pb[i];
        tau /= A1[j];
        for (int i = j; i < nr; i++) pb[i] -= tau * pA[i * nc + j];
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < nc; j++) sum += pA[i * nc + j] * pX[j];
        pX[i] = (pb[i] - sum) / A2[i];
    }
    return true;
}

// gauss_newton (:841-859)
ORB_HD void gauss_newton(const double* l, const double* rho, Branch& w) {
    for (int i = 0; i < 4; i++) w.gx[i] = 0.0;
    for (int k = 0; k < 5; k++) {
        gn_A_and_b(l, rho, w.betas, w.ga, w.gb);
        qr_solve(w.ga, w.gb, w.gx, w.A1, w.A2);
        for (int i = 0; i < 4; i++) w.betas[i] += w.gx[i];
    }
}

// the alphas of one correspondence (:424-434)
ORB_HD void alphas_of(const double* ci, const double cws[4][3], const double* pi, double* a) {
    for (int j = 0; j < 3; j++)
        a[1 + j] = ci[3 * j] * (pi[0] - cws[0][0]) + ci[3 * j + 1] * (pi[1] - cws[0][1]) + ci[3 * j + 2] * (pi[2] - cws[0][2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
}

ORB_HD void point_w(const Points& P, int k, double* pw) {
    const int i = P.list[k];
    pw[0] = P.p3d[i * 3]; pw[1] = P.p3d[i * 3 + 1]; pw[2] = P.p3d[i * 3 + 2];
}

// compute_pcs of one correspondence (:467-476) with the sign of solve_for_sign folded into ccs
template <class W>
ORB_HD void point_c(const W& w, const Points& P, int k, double* pw, double* pc) {
    double a[4];
    point_w(P, k, pw);
    alphas_of(w.ci, w.cws, pw, a);
    for (int j = 0; j < 3; j++) pc[j] = a[0] * w.ccs[0][j] + a[1] * w.ccs[1][j] + a[2] * w.ccs[2][j] + a[3] * w.ccs[3][j];
}

// indices of the diagonal of the n x n S sorted descending, the first of equal ones first
ORB_HD void order_descending(const double* S, int n, int* order) {
    for (int i = 0; i < n; i++) order[i] = i;
    for (int a = 1; a < n; a++) {                                  // insertion sort: stable
        const int o = order[a];
        int b = a;
        while (b > 0 && S[order[b - 1] * (n + 1)] < S[o * (n + 1)]) { order[b] = order[b - 1]; b--; }
        order[b] = o;
    }
}

// compute_pose (:478-526) over the correspondences P: R[9], t[3], errs[3], *branch = 1..3; vecs_out (48 doubles) may be null.
// Every thread of the context calls it; the outputs are written by thread 0 and complete after the final sync.
template <class Cx, class W>
ORB_HD void fit(Cx& cx, W& w, const Cam& cam, const Points& P, double* R, double* t, double* errs, int32_t* branch, double* vecs_out) {
    const int n = P.n;
    // choose_control_points (:376-410)
    ordered_sums<3, W::PS>(cx, n, w.part, w.sums, [&](int k, double* v) { point_w(P, k, v); });
    if (cx.tid == 0)
        for (int j = 0; j < 3; j++) w.cws[0][j] = w.sums[j] / n;
    cx.sync();
    ordered_sums<9, W::PS>(cx, n, w.part, w.S3, [&](int k, double* v) {
        double pw[3];
        point_w(P, k, pw);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) v[i * 3 + j] = (pw[i] - w.cws[0][i]) * (pw[j] - w.cws[0][j]);
    });
    if (cx.tid == 0) {
        orbj::sym_eig<3>(w.S3, w.V3);
        order_descending(w.S3, 3, w.order);
        for (int i = 1; i < 4; i++) {
            const int c = w.order[i - 1];
            const double k = sqrt(fabs(w.S3[c * 4]) / n);
            int big = 0;                                            // the axis' sign: its component of largest magnitude (the first of equal ones) positive
            for (int j = 1; j < 3; j++)
                if (fabs(w.V3[j * 3 + c]) > fabs(w.V3[big * 3 + c])) big = j;
            const bool flip = w.V3[big * 3 + c] < 0;
            for (int j = 0; j < 3; j++) w.cws[i][j] = w.cws[0][j] + k * (flip ? -w.V3[j * 3 + c] : w.V3[j * 3 + c]);
        }
        // compute_barycentric_coordinates (:412-422)
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) w.cc[3 * i + j - 1] = w.cws[j][i] - w.cws[0][i];
        pinv3(w.cc, w.S3, w.V3, w.ci);
    }
    cx.sync();
    // M'M, three rows (one control point) at a time
    for (int g = 0; g < 4; g++) {
        ordered_sums<36, W::PS>(cx, n, w.part, w.S + 36 * g, [&](int k, double* v) {
            double pw[3], a[4], M1[12], M2[12];
            point_w(P, k, pw);
            alphas_of(w.ci, w.cws, pw, a);
            const int i = P.list[k];
            const double u = P.p2d[i * 2], vv = P.p2d[i * 2 + 1];
ORB_UNROLL
            for (int c = 0; c < 4; c++) {                          // fill_M (:437-452)
                M1[3 * c] = a[c] * cam.fu; M1[3 * c + 1] = 0.0; M1[3 * c + 2] = a[c] * (cam.uc - u);
                M2[3 * c] = 0.0; M2[3 * c + 1] = a[c] * cam.fv; M2[3 * c + 2] = a[c] * (cam.vc - vv);
            }
            const double ag = g == 0 ? a[0] : g == 1 ? a[1] : g == 2 ? a[2] : a[3];
            const double r1[3] = {ag * cam.fu, 0.0, ag * (cam.uc - u)};
            const double r2[3] = {0.0, ag * cam.fv, ag * (cam.vc - vv)};
ORB_UNROLL
            for (int c = 0; c < 3; c++)
ORB_UNROLL
                for (int j = 0; j < 12; j++) v[c * 12 + j] = r1[c] * M1[j] + r2[c] * M2[j];
        });
    }
    cx.eig12(w.S, w.V);
    cx.sync();
    if (cx.tid == 0) order_descending(w.S, 12, w.order);
    cx.sync();
    for (int e = cx.tid; e < 48; e += cx.stride) {
        const double x = w.V[(e % 12) * 12 + w.order[11 - e / 12]];
        w.vecs[e / 12][e % 12] = x;
        if (vecs_out) vecs_out[e] = x;
    }
    cx.sync();
    if (cx.tid == 0) {
        compute_L_6x10(&w.vecs[0][0], w.l);
        w.rho[0] = dist2(w.cws[0], w.cws[1]);                       // compute_rho (:803-811)
        w.rho[1] = dist2(w.cws[0], w.cws[2]);
        w.rho[2] = dist2(w.cws[0], w.cws[3]);
        w.rho[3] = dist2(w.cws[1], w.cws[2]);
        w.rho[4] = dist2(w.cws[1], w.cws[3]);
        w.rho[5] = dist2(w.cws[2], w.cws[3]);
    }
    cx.sync();
#if defined(ORBE_SERIAL_BETAS)                                         // measurement aid (NOTES §32): one thread takes the three branches in turn
    if (cx.tid == 0)
        for (int b = 0; b < 3; b++) {
            find_betas(w.l, w.rho, b, w.br[b]);
            gauss_newton(w.l, w.rho, w.br[b]);
        }
#else
    for (int b = cx.tid; b < 3; b += cx.stride) {
        find_betas(w.l, w.rho, b, w.br[b]);
        gauss_newton(w.l, w.rho, w.br[b]);
    }
#endif
    cx.sync();
    // compute_R_and_t (:652-663) of the three branches
    for (int b = 0; b < 3; b++) {
        if (cx.tid == 0) {
            const double* betas = w.br[b].betas;
            for (int i = 0; i < 4; i++) w.ccs[i][0] = w.ccs[i][1] = w.ccs[i][2] = 0.0f;
            for (int i = 0; i < 4; i++)                             // compute_ccs (:454-465)
                for (int j = 0; j < 4; j++)
                    for (int k = 0; k < 3; k++) w.ccs[j][k] += betas[i] * w.vecs[i][3 * j + k];
            double pw[3], pc[3];
            point_c(w, P, 0, pw, pc);
            if (pc[2] < 0.0)                                        // solve_for_sign (:637-650)
                for (int i = 0; i < 4; i++)
                    for (int j = 0; j < 3; j++) w.ccs[i][j] = -w.ccs[i][j];
        }
        cx.sync();
        // estimate_R_and_t (:570-628)
        ordered_sums<6, W::PS>(cx, n, w.part, w.sums, [&](int k, double* v) { point_c(w, P, k, v + 3, v); });
        if (cx.tid == 0)
            for (int j = 0; j < 3; j++) {
                w.pc0[j] = w.sums[j] / n;
                w.pw0[j] = w.sums[3 + j] / n;
            }
        cx.sync();
        ordered_sums<9, W::PS>(cx, n, w.part, w.abt, [&](int k, double* v) {
            double pw[3], pc[3];
            point_c(w, P, k, pw, pc);
            for (int j = 0; j < 3; j++)
                for (int c = 0; c < 3; c++) v[3 * j + c] = (pc[j] - w.pc0[j]) * (pw[c] - w.pw0[c]);
        });
        double* Rb = w.Rs[b];
        double* tb = w.ts[b];
        if (cx.tid == 0) {
            orbj::svd3(w.abt, w.U, w.w3, w.Vt);
            if (!(w.w3[2] > 1e-4 * w.w3[0])) {                      // svd3 took the cross product for U's third column: give it the sign of ABt*v3
                double d = 0.0;
                for (int r = 0; r < 3; r++) d = d + w.U[r * 3 + 2] * dot3(w.abt + r * 3, w.Vt + 6);
                if (d < 0)
                    for (int r = 0; r < 3; r++) w.U[r * 3 + 2] = -w.U[r * 3 + 2];
            }
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) Rb[i * 3 + j] = w.U[i * 3] * w.Vt[j] + w.U[i * 3 + 1] * w.Vt[3 + j] + w.U[i * 3 + 2] * w.Vt[6 + j];
            const double det = Rb[0] * Rb[4] * Rb[8] + Rb[1] * Rb[5] * Rb[6] + Rb[2] * Rb[3] * Rb[7] - Rb[2] * Rb[4] * Rb[6] - Rb[1] * Rb[3] * Rb[8] -
                               Rb[0] * Rb[5] * Rb[7];
            if (det < 0) {
                Rb[6] = -Rb[6];
                Rb[7] = -Rb[7];
                Rb[8] = -Rb[8];
            }
            tb[0] = w.pc0[0] - dot3(Rb, w.pw0);
            tb[1] = w.pc0[1] - dot3(Rb + 3, w.pw0);
            tb[2] = w.pc0[2] - dot3(Rb + 6, w.pw0);
        }
        cx.sync();
        // reprojection_error (:551-568)
        ordered_sums<1, W::PS>(cx, n, w.part, w.sums, [&](int k, double* v) {
            double pw[3];
            point_w(P, k, pw);
            const double Xc = dot3(Rb, pw) + tb[0];
            const double Yc = dot3(Rb + 3, pw) + tb[1];
            const double inv_Zc = 1.0 / (dot3(Rb + 6, pw) + tb[2]);
            const double ue = cam.uc + cam.fu * Xc * inv_Zc;
            const double ve = cam.vc + cam.fv * Yc * inv_Zc;
            const int i = P.list[k];
            const double u = P.p2d[i * 2], vv = P.p2d[i * 2 + 1];
            v[0] = sqrt((u - ue) * (u - ue) + (vv - ve) * (vv - ve));
        });
        if (cx.tid == 0) w.err[b] = w.sums[0] / n;
        cx.sync();
    }
    if (cx.tid == 0) {
        int N = 0;                                                  // :519-521 (branches 1, 2, 3 of the source are 0, 1, 2 here)
        if (w.err[1] < w.err[0]) N = 1;
        if (w.err[2] < w.err[N]) N = 2;
        for (int i = 0; i < 9; i++) R[i] = w.Rs[N][i];
        for (int i = 0; i < 3; i++) {
            t[i] = w.ts[N][i];
            errs[i] = w.err[i];
        }
        *branch = N + 1;
    }
    cx.sync();
}

// CheckInliers of one correspondence (:315-330) with the source's mix of float and double
ORB_HD bool is_inlier(const Cam& cam, const double* R, const double* t, const float* p3, const float* p2, float maxerr) {
    const double x = p3[0], y = p3[1], z = p3[2];
    const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
    const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
    const float invZc = (float)(1 / (R[6] * x + R[7] * y + R[8] * z + t[2]));
    const double ue = cam.uc + cam.fu * Xc * invZc;
    const double ve = cam.vc + cam.fv * Yc * invZc;
    const float distX = (float)(p2[0] - ue);
    const float distY = (float)(p2[1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < maxerr;
}

// rows 0-2 of [R|t] rounded to float once (convertTo(CV_32F))
ORB_HD void tcw_of(const double* R, const double* t, float* tcw) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) tcw[r * 4 + c] = (float)R[r * 3 + c];
        tcw[r * 4 + 3] = (float)t[r];
    }
}

// true when iteration `it` of a range is a record (orbe.h)
ORB_HD bool is_record(const int32_t* count, int it, int min_inliers, int best_in) {
    const int c = count[it];
    if (c < min_inliers || c <= best_in) return false;
    for (int j = 0; j < it; j++)
        if (count[j] >= c) return false;
    return true;
}

struct Walk { int best_it, flags_from; };     // best_it: the iteration that became the best (-1: the carried one stays)

// The decisions of iterate() (:183-258) over one range: updates st, fills res (but not the flag arrays) and says where the flags come from.
ORB_HD Walk walk(const orbe_problem& q, const double* R, const double* t, const int32_t* count, const double* rR, const double* rt, const int32_t* rcount,
                 const int32_t* rok, orbe_state& st, orbe_result& res) {
    Walk w = {-1, 0};
    res.kind = ORBE_KIND_NONE;
    res.stop = q.iters;
    res.no_more = 0;
    res.ninliers = 0;
    for (int i = 0; i < 12; i++) res.tcw[i] = 0.0f;
    for (int j = 0; j < q.iters; j++) {
        st.iterations++;
        const int c = count[j];
        if (c < q.min_inliers) continue;
        if (c > st.best_inliers) {
            st.best_inliers = c;
            w.best_it = j;
            tcw_of(R + (size_t)j * 9, t + (size_t)j * 3, st.best_tcw);
            st.refine_ok = rok[j] ? 1 : 0;
            st.refined_inliers = rcount[j];
            if (st.refine_ok) tcw_of(rR + (size_t)j * 9, rt + (size_t)j * 3, st.refined_tcw);
        }
        if (st.refine_ok) {
            res.kind = ORBE_KIND_REFINED;
            res.stop = j;
            res.ninliers = st.refined_inliers;
            for (int i = 0; i < 12; i++) res.tcw[i] = st.refined_tcw[i];
            return w;
        }
    }
    if (st.iterations >= q.max_its) {
        res.no_more = 1;
        if (st.best_inliers >= q.min_inliers) {
            res.kind = ORBE_KIND_BEST;
            res.ninliers = st.best_inliers;
            for (int i = 0; i < 12; i++) res.tcw[i] = st.best_tcw[i];
        }
    }
    return w;
}

// SetRansacParameters (:122-158) with the source's types
inline void ransac_parameters(int N, double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2, const float* sigma2,
                              int32_t* min_inliers_out, int32_t* max_its_out, float* epsilon_out, float* maxerr) {
    int mRansacMinInliers = minInliers;
    int mRansacMaxIts = maxIterations;
    float mRansacEpsilon = epsilon;
    int nMinInliers = (int)(N * mRansacEpsilon);
    if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;
    if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N) {
        nIterations = 1;
    } else {
        const double x = ceil(log(1 - probability) / log(1 - pow((double)mRansacEpsilon, 3.0)));
        // a value an int cannot hold (NaN when epsilon > 1, -inf when epsilon^3 underflows): the source's conversion is undefined; x86 gives INT_MIN
        nIterations = (x > -2147483649.0 && x < 2147483648.0) ? (int)x : (int)-2147483647 - 1;
    }
    const int m = nIterations < mRansacMaxIts ? nIterations : mRansacMaxIts;
    mRansacMaxIts = m > 1 ? m : 1;
    *min_inliers_out = mRansacMinInliers;
    *max_its_out = mRansacMaxIts;
    *epsilon_out = mRansacEpsilon;
    for (int i = 0; i < N; i++) maxerr[i] = sigma2[i] * th2;
}

}  // namespace orbe
