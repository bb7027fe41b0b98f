// The arithmetic of the monocular initialisation (include/orbi.h states it), one text for the kernels of orbi_init.hip and for the host:
// the drop-in's host steps, the host route of tools/ and tests/_probe/init_host.cpp.  Build with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "orb_jacobi.h"
#include "orbi.h"

namespace orbi {

struct Terms { float t1, t2; bool in; };     // what one match adds to the score (0: excluded) and its inlier flag

// CheckHomography (src/Initializer.cc:335-383) for one match
ORB_HD Terms homography_terms(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float invSigmaSquare) {
    const float th = 5.991f;
    Terms r = {0.0f, 0.0f, true};
    const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) r.in = false;
    else r.t1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) r.in = false;
    else r.t2 = th - chiSquare2;
    return r;
}

// CheckFundamental (src/Initializer.cc:411-463) for one match
ORB_HD Terms fundamental_terms(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare) {
    const float th = 3.841f, thScore = 5.991f;
    Terms r = {0.0f, 0.0f, true};
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) r.in = false;
    else r.t1 = thScore - chiSquare1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) r.in = false;
    else r.t2 = thScore - chiSquare2;
    return r;
}

ORB_HD float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// row r (0 .. 15) of ComputeH21's A (:237-255) for the normalised pair (u1, v1) -> (u2, v2) of point r / 2
ORB_HD void homography_row(int r, float u1, float v1, float u2, float v2, float* a) {
    if ((r & 1) == 0) {
        a[0] = 0.0f; a[1] = 0.0f; a[2] = 0.0f; a[3] = -u1; a[4] = -v1; a[5] = -1.0f; a[6] = v2 * u1; a[7] = v2 * v1; a[8] = v2;
    } else {
        a[0] = u1; a[1] = v1; a[2] = 1.0f; a[3] = 0.0f; a[4] = 0.0f; a[5] = 0.0f; a[6] = -u2 * u1; a[7] = -u2 * v1; a[8] = -u2;
    }
}

// row of ComputeF21's A (:279-287)
ORB_HD void fundamental_row(float u1, float v1, float u2, float v2, float* a) {
    a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1.0f;
}

// the float T of Normalize (:788-792) from nrm = {sX, sY, meanX, meanY}, as doubles
ORB_HD void norm_matrix(const float* nrm, double* T) {
    const float t02 = -nrm[2] * nrm[0], t12 = -nrm[3] * nrm[1];
    T[0] = (double)nrm[0]; T[1] = 0.0; T[2] = (double)t02;
    T[3] = 0.0; T[4] = (double)nrm[1]; T[5] = (double)t12;
    T[6] = 0.0; T[7] = 0.0; T[8] = 1.0;
}

// C = A*B, 3 x 3 doubles, each entry a sum from 0.0 left to right
ORB_HD void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s = s + A[i * 3 + k] * B[k * 3 + j];
            C[i * 3 + j] = s;
        }
}

// H21 = inv(T2)*Hn*T1 in double, rounded once; H12 = adj(H21)/det(H21) in double from the float H21, rounded
ORB_HD void homography_chain(const float* hn, const float* norm1, const float* norm2, float* H21, float* H12) {
    double T1[9], T2[9], Ti[9], Hd[9], M[9], R[9];
    norm_matrix(norm1, T1);
    norm_matrix(norm2, T2);
    for (int i = 0; i < 9; i++) { Hd[i] = (double)hn[i]; Ti[i] = 0.0; }
    Ti[0] = 1.0 / T2[0]; Ti[2] = -T2[2] / T2[0];
    Ti[4] = 1.0 / T2[4]; Ti[5] = -T2[5] / T2[4];
    Ti[8] = 1.0;
    mul3(Hd, T1, M);
    mul3(Ti, M, R);
    double h[9];
    for (int i = 0; i < 9; i++) { H21[i] = (float)R[i]; h[i] = (double)H21[i]; }
    double adj[9];
    adj[0] = h[4] * h[8] - h[5] * h[7]; adj[1] = h[2] * h[7] - h[1] * h[8]; adj[2] = h[1] * h[5] - h[2] * h[4];
    adj[3] = h[5] * h[6] - h[3] * h[8]; adj[4] = h[0] * h[8] - h[2] * h[6]; adj[5] = h[2] * h[3] - h[0] * h[5];
    adj[6] = h[3] * h[7] - h[4] * h[6]; adj[7] = h[1] * h[6] - h[0] * h[7]; adj[8] = h[0] * h[4] - h[1] * h[3];
    const double det = (h[0] * adj[0] + h[1] * adj[3]) + h[2] * adj[6];
    for (int i = 0; i < 9; i++) H12[i] = (float)(adj[i] / det);
}

// Fn = Fpre - (Fpre*v)*v' with v = column k of V (the eigenvectors of Fpre'Fpre); F21 = T2'*Fn*T1 in double, rounded to float
ORB_HD void fundamental_chain(const float* fpre, const double* V, int k, const float* norm1, const float* norm2, float* F21) {
    double T1[9], T2[9], Tt[9], Fn[9], M[9], R[9];
    norm_matrix(norm1, T1);
    norm_matrix(norm2, T2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Tt[i * 3 + j] = T2[j * 3 + i];
    const double v[3] = {V[k], V[3 + k], V[6 + k]};
    for (int i = 0; i < 3; i++) {
        double fv = 0.0;
        for (int j = 0; j < 3; j++) fv = fv + (double)fpre[i * 3 + j] * v[j];
        for (int j = 0; j < 3; j++) Fn[i * 3 + j] = (double)fpre[i * 3 + j] - fv * v[j];
    }
    mul3(Fn, T1, M);
    mul3(Tt, M, R);
    for (int i = 0; i < 9; i++) F21[i] = (float)R[i];
}

// the symmetric Fpre'Fpre in double (the 3 x 3 step's input)
ORB_HD void gram3(const float* fpre, double* S) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) S[i * 3 + j] = orbj::gram_entry<3>(fpre, 3, i, j);
}

struct RtOut { float X[3]; float v[4]; float cosp; int status; };

ORB_HD bool finite_f(float x) { return x - x == 0.0f; }

// the body of CheckRT's loop (src/Initializer.cc:833-891) with Triangulate (:732-745) for one flagged match
ORB_HD void check_rt_one(float fx, float fy, float cx, float cy, const orbi_pose& P, float k1x, float k1y, float k2x, float k2y, float th2, RtOut& o) {
    const float P1[3][4] = {{fx, 0.0f, cx, 0.0f}, {0.0f, fy, cy, 0.0f}, {0.0f, 0.0f, 1.0f, 0.0f}};
    float A[4][4];
ORB_UNROLL
    for (int c = 0; c < 4; c++) {
        A[0][c] = k1x * P1[2][c] - P1[0][c];
        A[1][c] = k1y * P1[2][c] - P1[1][c];
        A[2][c] = k2x * P.P2[8 + c] - P.P2[c];
        A[3][c] = k2y * P.P2[8 + c] - P.P2[4 + c];
    }
    orbj::null_vector(A, o.v);
    o.cosp = 0.0f;
    float X[3];
ORB_UNROLL
    for (int i = 0; i < 3; i++) { X[i] = o.v[i] / o.v[3]; o.X[i] = 0.0f; }
    if (!finite_f(X[0]) || !finite_f(X[1]) || !finite_f(X[2])) { o.status = ORBI_RT_NONFINITE; return; }
ORB_UNROLL
    for (int i = 0; i < 3; i++) o.X[i] = X[i];
    double s1 = 0.0, s2 = 0.0, dot = 0.0;
    float n2[3];
ORB_UNROLL
    for (int i = 0; i < 3; i++) {
        const float n1 = X[i] - 0.0f;
        n2[i] = X[i] - P.O2[i];
        s1 = s1 + (double)n1 * (double)n1;
        s2 = s2 + (double)n2[i] * (double)n2[i];
        dot = dot + (double)n1 * (double)n2[i];
    }
    const float dist1 = (float)sqrt(s1), dist2 = (float)sqrt(s2);
    const float cosp = (float)(dot / (double)(dist1 * dist2));
    o.cosp = cosp;
    const bool parallax = (double)cosp < 0.99998;
    if (X[2] <= 0.0f && parallax) { o.status = ORBI_RT_DEPTH1; return; }
    float p2[3];
ORB_UNROLL
    for (int r = 0; r < 3; r++) {
        float s = 0.0f;
        s = s + P.R[r * 3] * X[0];
        s = s + P.R[r * 3 + 1] * X[1];
        s = s + P.R[r * 3 + 2] * X[2];
        p2[r] = s + P.t[r];
    }
    if (p2[2] <= 0.0f && parallax) { o.status = ORBI_RT_DEPTH2; return; }
    const float invZ1 = (float)(1.0 / (double)X[2]);
    const float im1x = fx * X[0] * invZ1 + cx, im1y = fy * X[1] * invZ1 + cy;
    const float e1 = (im1x - k1x) * (im1x - k1x) + (im1y - k1y) * (im1y - k1y);
    if (e1 > th2) { o.status = ORBI_RT_REPROJ1; return; }
    const float invZ2 = (float)(1.0 / (double)p2[2]);
    const float im2x = fx * p2[0] * invZ2 + cx, im2y = fy * p2[1] * invZ2 + cy;
    const float e2 = (im2x - k2x) * (im2x - k2x) + (im2y - k2y) * (im2y - k2y);
    if (e2 > th2) { o.status = ORBI_RT_REPROJ2; return; }
    o.status = parallax ? ORBI_RT_GOOD : ORBI_RT_COUNTED;
}

// Normalize (src/Initializer.cc:747-793): float sums in index order over all key points
inline void normalize(const orbx_keypoint* kps, int n, float* out) {
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += kps[i].x; meanY += kps[i].y; }
    meanX = meanX / n;
    meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < n; i++) {
        meanDevX += fabsf(kps[i].x - meanX);
        meanDevY += fabsf(kps[i].y - meanY);
    }
    meanDevX = meanDevX / n;
    meanDevY = meanDevY / n;
    out[0] = (float)(1.0 / (double)meanDevX);
    out[1] = (float)(1.0 / (double)meanDevY);
    out[2] = meanX;
    out[3] = meanY;
}

inline void pose_from_rt(float fx, float fy, float cx, float cy, const float* R, const float* t, orbi_pose* pose) {
    const float K[3][3] = {{fx, 0.0f, cx}, {0.0f, fy, cy}, {0.0f, 0.0f, 1.0f}};
    for (int i = 0; i < 9; i++) pose->R[i] = R[i];
    for (int i = 0; i < 3; i++) pose->t[i] = t[i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            float s = 0.0f;
            for (int k = 0; k < 3; k++) s = s + K[i][k] * (j < 3 ? R[k * 3 + j] : t[k]);
            pose->P2[i * 4 + j] = s;
        }
    for (int i = 0; i < 3; i++) {
        float s = 0.0f;
        for (int k = 0; k < 3; k++) s = s + (-R[k * 3 + i]) * t[k];
        pose->O2[i] = s;
    }
}

// parallax of :896-902 from the cosines of the counted entries (sorted in place): acos is std::acos(float) in the source
inline float parallax_of(float* cosines, int n) {
    if (n <= 0) return 0.0f;
    std::sort(cosines, cosines + n);
    const int idx = n - 1 < 50 ? n - 1 : 50;
    return (float)((double)(acosf(cosines[idx]) * 180) / 3.1415926535897932384626433832795);
}

}  // namespace orbi
