// The arithmetic of the Sim3 RANSAC (include/orbh.h states it): Horn's closed form over three correspondences, the inlier test and the walk of
// iterate().  One text for the device (orbh_sim3solver.hip), the host route (tools/sim3solver_host_route.cpp) and tests/_probe/sim3solver_host.cpp.
// A fit is private to one lane (every array below has compile-time indices and lives in registers), so unlike orbe::fit it takes no context:
// there is nothing for lanes to share and no barrier to place.  Compile with -ffp-contract=off.
//
// Float steps follow the stand-in cv::Mat arithmetic (oracle/matcherstub/opencv2/core/core.hpp); the steps NOT pinned to OpenCV are
// top_quaternion (cv::eigen) and rotation (cv::Rodrigues of 2*ang*vec/norm(vec)).
#pragma once
#include <math.h>
#include <stdint.h>

#include "orb_jacobi.h"
#include "orbh.h"

namespace orbh {

ORB_HD float nanf_() { return __builtin_nanf(""); }
ORB_HD float canon(float x) { return x != x ? nanf_() : x; }
ORB_HD double canon(double x) { return x != x ? __builtin_nan("") : x; }

// one entry of a cv::Mat product with three terms: float s = 0; s += a*b in k order
ORB_HD float dot3f(float a0, float b0, float a1, float b1, float a2, float b2) {
    float s = 0.0f;
    s = s + a0 * b0;
    s = s + a1 * b1;
    s = s + a2 * b2;
    return s;
}

// Sim3Solver::centroid (:215-224); P holds one point per COLUMN
ORB_HD void centroid(const float (&P)[3][3], float (&Pr)[3][3], float (&C)[3]) {
ORB_UNROLL
    for (int r = 0; r < 3; r++) {
        float s = P[r][0];
        s = s + P[r][1];
        s = s + P[r][2];
        C[r] = (float)((double)s / 3.0);
    }
ORB_UNROLL
    for (int r = 0; r < 3; r++)
ORB_UNROLL
        for (int c = 0; c < 3; c++) Pr[r][c] = P[r][c] - C[r];
}

// M = Pr2*Pr1.t() (:243) and the float N of :251-265
ORB_HD void horn_matrices(const float (&Pr1)[3][3], const float (&Pr2)[3][3], float (&M)[3][3], float (&N)[4][4]) {
ORB_UNROLL
    for (int y = 0; y < 3; y++)
ORB_UNROLL
        for (int x = 0; x < 3; x++) M[y][x] = dot3f(Pr2[y][0], Pr1[x][0], Pr2[y][1], Pr1[x][1], Pr2[y][2], Pr1[x][2]);
    const float N11 = M[0][0] + M[1][1] + M[2][2];
    const float N12 = M[1][2] - M[2][1];
    const float N13 = M[2][0] - M[0][2];
    const float N14 = M[0][1] - M[1][0];
    const float N22 = M[0][0] - M[1][1] - M[2][2];
    const float N23 = M[0][1] + M[1][0];
    const float N24 = M[2][0] + M[0][2];
    const float N33 = -M[0][0] + M[1][1] - M[2][2];
    const float N34 = M[1][2] + M[2][1];
    const float N44 = -M[0][0] - M[1][1] + M[2][2];
    N[0][0] = N11; N[0][1] = N12; N[0][2] = N13; N[0][3] = N14;
    N[1][0] = N12; N[1][1] = N22; N[1][2] = N23; N[1][3] = N24;
    N[2][0] = N13; N[2][1] = N23; N[2][2] = N33; N[2][3] = N34;
    N[3][0] = N14; N[3][1] = N24; N[3][2] = N34; N[3][3] = N44;
}

// NOT PINNED (cv::eigen): the eigenvector of the widened N for its largest eigenvalue (the first of equal ones), with q[0] >= 0
ORB_HD void top_quaternion(const float (&N)[4][4], double (&q)[4]) {
    double S[4][4], V[4][4];
ORB_UNROLL
    for (int i = 0; i < 4; i++)
ORB_UNROLL
        for (int j = 0; j < 4; j++) {
            S[i][j] = (double)N[i][j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < orbj::MAX_SWEEPS; sweep++) {
        const double off = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[0][3] * S[0][3] + S[1][2] * S[1][2] + S[1][3] * S[1][3] + S[2][3] * S[2][3];
        const double diag = S[0][0] * S[0][0] + S[1][1] * S[1][1] + S[2][2] * S[2][2] + S[3][3] * S[3][3];
        if (!(off > 1e-36 * diag)) break;                    // converged, a zero matrix, or NaN
        orbj::rotate<0, 1>(S, V); orbj::rotate<0, 2>(S, V); orbj::rotate<0, 3>(S, V);
        orbj::rotate<1, 2>(S, V); orbj::rotate<1, 3>(S, V); orbj::rotate<2, 3>(S, V);
    }
    int k = 0;
    double best = S[0][0];
    if (S[1][1] > best) { best = S[1][1]; k = 1; }
    if (S[2][2] > best) { best = S[2][2]; k = 2; }
    if (S[3][3] > best) { best = S[3][3]; k = 3; }
ORB_UNROLL
    for (int i = 0; i < 4; i++) q[i] = k == 0 ? V[i][0] : k == 1 ? V[i][1] : k == 2 ? V[i][2] : V[i][3];
    if (q[0] < 0.0) {
ORB_UNROLL
        for (int i = 0; i < 4; i++) q[i] = -q[i];
    }
}

// NOT PINNED (cv::Rodrigues): the rotation of the quaternion in double, rounded to float once; NaN where norm(vec) == 0 (orbh.h)
ORB_HD void rotation(const double (&q)[4], float (&R)[3][3]) {
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    const double aa = a * a, bb = b * b, cc = c * c, dd = d * d;
    const double vv = (bb + cc) + dd, n2 = aa + vv;
    const bool none = vv == 0.0;
    const double r[3][3] = {{(aa + bb) - (cc + dd), 2.0 * (b * c - a * d), 2.0 * (b * d + a * c)},
                            {2.0 * (b * c + a * d), (aa + cc) - (bb + dd), 2.0 * (c * d - a * b)},
                            {2.0 * (b * d - a * c), 2.0 * (c * d + a * b), (aa + dd) - (bb + cc)}};
ORB_UNROLL
    for (int y = 0; y < 3; y++)
ORB_UNROLL
        for (int x = 0; x < 3; x++) R[y][x] = none ? nanf_() : (float)(r[y][x] / n2);
}

// computeT after its rotation (:286-331): scale, translation, T12 and T21 from the float R12
ORB_HD void similarity(const float (&R)[3][3], const float (&Pr1)[3][3], const float (&Pr2)[3][3], const float (&O1)[3], const float (&O2)[3], orbh_hyp& h) {
    float P3[3][3];
ORB_UNROLL
    for (int y = 0; y < 3; y++)
ORB_UNROLL
        for (int x = 0; x < 3; x++) P3[y][x] = dot3f(R[y][0], Pr2[0][x], R[y][1], Pr2[1][x], R[y][2], Pr2[2][x]);
    double nom = 0.0, den = 0.0;
ORB_UNROLL
    for (int y = 0; y < 3; y++)
ORB_UNROLL
        for (int x = 0; x < 3; x++) nom = nom + (double)Pr1[y][x] * (double)P3[y][x];
ORB_UNROLL
    for (int y = 0; y < 3; y++)
ORB_UNROLL
        for (int x = 0; x < 3; x++) {
            const float sq = P3[y][x] * P3[y][x];
            den = den + (double)sq;
        }
    const float s = (float)(nom / den);
    const double inv = 1.0 / (double)s;
    float sR[3][3], sRinv[3][3], t[3], tinv[3];
ORB_UNROLL
    for (int y = 0; y < 3; y++)
ORB_UNROLL
        for (int x = 0; x < 3; x++) {
            sR[y][x] = (float)((double)R[y][x] * (double)s);
            sRinv[y][x] = (float)((double)R[x][y] * inv);
        }
ORB_UNROLL
    for (int y = 0; y < 3; y++) t[y] = O1[y] - dot3f(sR[y][0], O2[0], sR[y][1], O2[1], sR[y][2], O2[2]);
ORB_UNROLL
    for (int y = 0; y < 3; y++) {
        const float n0 = (float)((double)sRinv[y][0] * -1.0), n1 = (float)((double)sRinv[y][1] * -1.0), n2 = (float)((double)sRinv[y][2] * -1.0);
        tinv[y] = dot3f(n0, t[0], n1, t[1], n2, t[2]);
    }
    h.s = canon(s);
ORB_UNROLL
    for (int y = 0; y < 3; y++) {
ORB_UNROLL
        for (int x = 0; x < 3; x++) {
            h.R[y * 3 + x] = canon(R[y][x]);
            h.T12[y * 4 + x] = canon(sR[y][x]);
            h.T21[y * 4 + x] = canon(sRinv[y][x]);
        }
        h.t[y] = canon(t[y]);
        h.T12[y * 4 + 3] = canon(t[y]);
        h.T21[y * 4 + 3] = canon(tinv[y]);
    }
    h.T12[12] = h.T12[13] = h.T12[14] = 0.0f; h.T12[15] = 1.0f;
    h.T21[12] = h.T21[13] = h.T21[14] = 0.0f; h.T21[15] = 1.0f;
}

// computeT (:226-332) over the three correspondences a, b, c (each x, y, z of set 1 then of set 2); count is left alone
ORB_HD void fit(const float (&A)[6], const float (&B)[6], const float (&C)[6], orbh_hyp& h) {
    float P1[3][3], P2[3][3], Pr1[3][3], Pr2[3][3], O1[3], O2[3], M[3][3], N[4][4], R[3][3];
ORB_UNROLL
    for (int r = 0; r < 3; r++) {
        P1[r][0] = A[r]; P1[r][1] = B[r]; P1[r][2] = C[r];
        P2[r][0] = A[3 + r]; P2[r][1] = B[3 + r]; P2[r][2] = C[3 + r];
    }
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
    horn_matrices(Pr1, Pr2, M, N);
    double q[4];
    top_quaternion(N, q);
    rotation(q, R);
ORB_UNROLL
    for (int i = 0; i < 4; i++) h.q[i] = canon(q[i]);
    similarity(R, Pr1, Pr2, O1, O2, h);
}

// a set that names an index outside [0, N)
ORB_HD void void_hyp(orbh_hyp& h) {
    for (int i = 0; i < 4; i++) h.q[i] = __builtin_nan("");
    for (int i = 0; i < 9; i++) h.R[i] = nanf_();
    for (int i = 0; i < 3; i++) h.t[i] = nanf_();
    h.s = nanf_();
    for (int i = 0; i < 16; i++) h.T12[i] = h.T21[i] = nanf_();
    h.count = 0;
}

// Project (:377-398) of one point through the first three rows of T
ORB_HD void project(const float* T, float fx, float fy, float cx, float cy, float X, float Y, float Z, float& u, float& v) {
    const float x = dot3f(T[0], X, T[1], Y, T[2], Z) + T[3];
    const float y = dot3f(T[4], X, T[5], Y, T[6], Z) + T[7];
    const float z = dot3f(T[8], X, T[9], Y, T[10], Z) + T[11];
    const float invz = 1.0f / z;
    const float px = x * invz, py = y * invz;
    u = fx * px + cx;
    v = fy * py + cy;
}

// the squared distance of :345-349: a double dot product rounded to float
ORB_HD float err2(float d0, float d1) {
    double s = 0.0;
    s = s + (double)d0 * (double)d0;
    s = s + (double)d1 * (double)d1;
    return (float)s;
}

// one correspondence of CheckInliers (:335-359)
ORB_HD bool is_inlier(const orbh_problem& k, const float* T12, const float* T21, float x1, float y1, float z1, float x2, float y2, float z2, float u1,
                      float v1, float u2, float v2, float maxerr1, float maxerr2) {
    float a, b, c, d;
    project(T12, k.fx1, k.fy1, k.cx1, k.cy1, x2, y2, z2, a, b);        // vP2im1
    project(T21, k.fx2, k.fy2, k.cx2, k.cy2, x1, y1, z1, c, d);        // vP1im2
    const float e1 = err2(u1 - a, v1 - b);
    const float e2 = err2(c - u2, d - v2);
    return e1 < maxerr1 && e2 < maxerr2;
}

// SetRansacParameters (:114-138)
inline int ransac_parameters(int N, double probability, int minInliers, int maxIterations) {
    const float epsilon = (float)minInliers / N;
    int nIterations;
    if (minInliers == N) {
        nIterations = 1;
    } else {
        const double x = ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0)));
        // a value an int cannot hold (NaN when epsilon > 1, -inf when epsilon^3 underflows): the source's conversion is undefined; x86 gives INT_MIN
        nIterations = (x > -2147483649.0 && x < 2147483648.0) ? (int)x : (int)-2147483647 - 1;
    }
    const int m = nIterations < maxIterations ? nIterations : maxIterations;
    return m > 1 ? m : 1;
}

// mvnMaxError (:87-88, a std::vector<size_t>) as the comparison of :351 sees it
inline float max_error(float sigma2) {
    const double e = 9.210 * sigma2;
    return (float)(e >= 0.0 && e < 18446744073709551616.0 ? (size_t)e : (size_t)0);
}

// the walk of iterate() (:140-207) over the counts of a range; best_it = the iteration whose hypothesis became the best (-1: none did).  The counts
// alone decide it, so the device walks them from LDS; take_best then copies the one hypothesis that matters.
struct Walk { int best_it; };

ORB_HD Walk walk(const orbh_problem& q, const int32_t* count, orbh_state& st, orbh_result& res) {
    Walk w = {-1};
    res.found = 0; res.stop = 0; res.no_more = 0; res.ninliers = 0;
    for (int i = 0; i < 16; i++) res.T12[i] = 0.0f;
    if (q.n < q.min_inliers) {
        res.no_more = 1;
        return w;
    }
    int it = 0;
    while (st.iterations < q.max_its && it < q.iters) {
        st.iterations++;
        const int c = count[it];
        if (c >= st.best_inliers) {
            w.best_it = it;
            st.best_inliers = c;
            if (c > q.min_inliers) {
                res.found = 1;
                res.ninliers = c;
                break;
            }
        }
        it++;
    }
    res.stop = it;
    if (!res.found && st.iterations >= q.max_its) res.no_more = 1;
    return w;
}

// the hypothesis of iteration Walk::best_it into the state (:185-190) and, when the walk returned there, into the result (:198)
ORB_HD void take_best(const orbh_hyp& b, orbh_state& st, orbh_result& res) {
    for (int i = 0; i < 16; i++) st.best_T12[i] = b.T12[i];
    for (int i = 0; i < 9; i++) st.best_R[i] = b.R[i];
    for (int i = 0; i < 3; i++) st.best_t[i] = b.t[i];
    st.best_s = b.s;
    if (res.found)
        for (int i = 0; i < 16; i++) res.T12[i] = b.T12[i];
}

}  // namespace orbh
