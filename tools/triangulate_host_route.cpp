// The host route tools/bench_triangulate.py measures the device triangulation against: the match loop of
// LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:269-353) on one core, over downloaded arrays, with the arithmetic
// include/orbt.h states (built with -ffp-contract=off) and its own double-precision Jacobi for the null vector.  Also what
// tests/test_triangulate_host.py holds against the numpy restatement without a GPU.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbt.h"

namespace {

// eigenvector of the symmetric S for its smallest eigenvalue by cyclic Jacobi rotations, accumulated in V
void smallest_eigenvector(double S[4][4], double out[4]) {
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 12; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 4; i++) {
            diag += S[i][i] * S[i][i];
            for (int j = i + 1; j < 4; j++) off += S[i][j] * S[i][j];
        }
        if (!(off > 1e-36 * diag)) break;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                const double apq = S[p][q];
                if (!(apq != 0.0) || apq != apq) continue;
                const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; k++) {
                    if (k != p && k != q) {
                        const double skp = S[k][p], skq = S[k][q];
                        S[k][p] = S[p][k] = c * skp - s * skq;
                        S[k][q] = S[q][k] = s * skp + c * skq;
                    }
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
                S[p][p] -= t * apq;
                S[q][q] += t * apq;
                S[p][q] = S[q][p] = 0.0;
            }
    }
    int k = 0;
    for (int i = 1; i < 4; i++)
        if (S[i][i] < S[k][k]) k = i;
    for (int i = 0; i < 4; i++) out[i] = V[i][k];
}

float cam_coord(const orbt_camera& C, int r, const float X[3]) {
    double d = 0.0;
    for (int k = 0; k < 3; k++) d = d + (double)C.Rcw[r * 3 + k] * (double)X[k];
    return (float)(d + (double)C.tcw[r]);
}

void normalised(const orbt_camera& C, float x, float y, float xn[3], float ray[3]) {
    const float invfx = 1.0f / C.fx, invfy = 1.0f / C.fy;
    xn[0] = (x - C.cx) * invfx;
    xn[1] = (y - C.cy) * invfy;
    xn[2] = 1.0f;
    for (int i = 0; i < 3; i++) {
        float s = 0.0f;
        for (int k = 0; k < 3; k++) s = s + C.Rcw[k * 3 + i] * xn[k];
        ray[i] = s;
    }
}

bool reprojection_fails(const orbt_camera& C, const float X[3], float z, float kx, float ky, float sigma2) {
    const float x = cam_coord(C, 0, X), y = cam_coord(C, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = C.fx * x * invz + C.cx, v = C.fy * y * invz + C.cy;
    const float ex = u - kx, ey = v - ky;
    const float e2 = ex * ex + ey * ey;
    return !((double)e2 <= 5.991 * (double)sigma2);
}

float distance_to(const float X[3], const float O[3]) {
    double s = 0.0;
    for (int i = 0; i < 3; i++) {
        const double d = (double)(X[i] - O[i]);
        s = s + d * d;
    }
    return (float)std::sqrt(s);
}

int one_match(const orbt_pair& P, const float* f1, const float* s1, const float* f2, const float* s2, int nlevels, const orbx_keypoint& k1,
              const orbx_keypoint& k2, float X[3], float v[4]) {
    const int o1 = k1.octave, o2 = k2.octave;
    if (o1 < 0 || o1 >= nlevels || o2 < 0 || o2 >= nlevels) return ORBT_SKIP_OCTAVE;
    float xn1[3], xn2[3], r1[3], r2[3];
    normalised(P.kf1, k1.x, k1.y, xn1, r1);
    normalised(P.kf2, k2.x, k2.y, xn2, r2);
    double dot = 0.0, n1 = 0.0, n2 = 0.0;
    for (int i = 0; i < 3; i++) {
        dot = dot + (double)r1[i] * (double)r2[i];
        n1 = n1 + (double)r1[i] * (double)r1[i];
        n2 = n2 + (double)r2[i] * (double)r2[i];
    }
    const float cosp = (float)(dot / (std::sqrt(n1) * std::sqrt(n2)));
    if (!(cosp >= 0.0f && (double)cosp <= 0.9998)) return ORBT_PARALLAX;
    float A[4][4];
    const orbt_camera* cams[2] = {&P.kf1, &P.kf2};
    const float* xns[2] = {xn1, xn2};
    for (int h = 0; h < 2; h++)
        for (int c = 0; c < 4; c++) {
            const orbt_camera& C = *cams[h];
            const float t0 = c < 3 ? C.Rcw[c] : C.tcw[0], t1 = c < 3 ? C.Rcw[3 + c] : C.tcw[1], t2 = c < 3 ? C.Rcw[6 + c] : C.tcw[2];
            A[2 * h][c] = xns[h][0] * t2 - t0;
            A[2 * h + 1][c] = xns[h][1] * t2 - t1;
        }
    double S[4][4], e[4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int r = 0; r < 4; r++) s = s + (double)A[r][i] * (double)A[r][j];
            S[i][j] = s;
        }
    smallest_eigenvector(S, e);
    for (int i = 0; i < 4; i++) v[i] = (float)e[i];
    if (!(v[3] != 0.0f) || v[3] != v[3]) return ORBT_W_ZERO;
    for (int i = 0; i < 3; i++) X[i] = v[i] / v[3];
    const float z1 = cam_coord(P.kf1, 2, X);
    if (!(z1 > 0.0f)) return ORBT_DEPTH1;
    const float z2 = cam_coord(P.kf2, 2, X);
    if (!(z2 > 0.0f)) return ORBT_DEPTH2;
    if (reprojection_fails(P.kf1, X, z1, k1.x, k1.y, s1[o1])) return ORBT_REPROJ1;
    if (reprojection_fails(P.kf2, X, z2, k2.x, k2.y, s2[o2])) return ORBT_REPROJ2;
    const float d1 = distance_to(X, P.kf1.Ow), d2 = distance_to(X, P.kf2.Ow);
    if (d1 == 0.0f || d2 == 0.0f || d1 != d1 || d2 != d2) return ORBT_ZERO_DIST;
    const float ratio_dist = d1 / d2;
    const float ratio_octave = f1[o1] / f2[o2];
    const float ratio_factor = 1.5f * P.scale_factor;
    if (!(ratio_dist * ratio_factor >= ratio_octave && ratio_dist <= ratio_octave * ratio_factor)) return ORBT_SCALE;
    return ORBT_ACCEPTED;
}

}  // namespace

// One pair over host arrays, the interface of orbt_triangulate plus the two flag arrays (either may be NULL).  Returns the number of
// accepted matches; the first min(that, ocap) are listed.
extern "C" int triangulate_host(const orbt_pair* pair, const float* f1, const float* s1, const float* f2, const float* s2, int nlevels,
                                const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, const int32_t* match12, uint8_t* status,
                                float* x3d, float* v, int32_t* acc_idx, float* acc_x3d, int ocap, uint8_t* qvalid, uint8_t* claimed) {
    int count = 0;
    for (int i = 0; i < n1; i++) {
        float X[3] = {0, 0, 0}, nv[4] = {0, 0, 0, 0};
        const int j = match12[i];
        int st = ORBT_NONE;
        if (j != -1) st = j < 0 || j >= n2 ? ORBT_SKIP_INDEX : one_match(*pair, f1, s1, f2, s2, nlevels, kps1[i], kps2[j], X, nv);
        status[i] = (uint8_t)st;
        std::memcpy(x3d + (size_t)i * 3, X, sizeof(X));
        if (v) std::memcpy(v + (size_t)i * 4, nv, sizeof(nv));
        if (st != ORBT_ACCEPTED) continue;
        if (count < ocap) {
            acc_idx[count * 2] = i;
            acc_idx[count * 2 + 1] = j;
            std::memcpy(acc_x3d + (size_t)count * 3, X, sizeof(X));
        }
        if (qvalid) qvalid[i] = 0;
        if (claimed) claimed[j] = 1;
        count++;
    }
    return count;
}

// The same from the matches as the search leaves them (q2t by query position, qindex = KF1's feature of each position): vMatches12 is
// rebuilt in match12[n1] first, as a host caller of the search has to.
extern "C" int triangulate_host_queries(const orbt_pair* pair, const float* f1, const float* s1, const float* f2, const float* s2, int nlevels,
                                        const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, const int32_t* q2t, const int32_t* qindex,
                                        int nq, int32_t* match12, uint8_t* status, float* x3d, int32_t* acc_idx, float* acc_x3d, int ocap,
                                        uint8_t* qvalid, uint8_t* claimed) {
    for (int i = 0; i < n1; i++) match12[i] = -1;
    for (int q = 0; q < nq; q++)
        if (qindex[q] >= 0 && qindex[q] < n1) match12[qindex[q]] = q2t[q];
    return triangulate_host(pair, f1, s1, f2, s2, nlevels, kps1, n1, kps2, n2, match12, status, x3d, nullptr, acc_idx, acc_x3d, ocap, qvalid, claimed);
}
