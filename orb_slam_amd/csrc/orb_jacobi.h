// The cyclic Jacobi iteration in FP64 behind every "right singular vector for the smallest singular value" of this library: the 4 x 4
// triangulation matrices (k_triangulate, k_init_check_rt), the 16 x 9 and 8 x 9 matrices of the monocular initialisation and the 3 x 3
// rank-2 step of its fundamental matrices (k_init_models).  One text for the device and for the host: the drop-in Initializer, the host
// route of tools/ and tests/_probe/init_host.cpp compile it with a plain C++ compiler.
//
//   rotate<P, Q>, null_vector     4 x 4, both matrices in registers (every loop unrolled, no indexed array survives): one lane per matrix.
//   jacobi_* <N>, sym_eig<N>      N x N over arrays in memory (LDS on the device), cut into the three pieces of one rotation so that a
//                                 wave can spread the rows over its lanes (sym_eig_wave<N>) and still compute, element by element, what
//                                 the serial loop computes: the pieces touch disjoint elements.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ORB_HD __host__ __device__ __forceinline__
#define ORB_UNROLL _Pragma("unroll")
#else
#define ORB_HD inline
#define ORB_UNROLL
#endif

namespace orbj {

constexpr int MAX_SWEEPS = 12;        // a 4 x 4 symmetric matrix converges in 5-7; the bound ends a NaN matrix
constexpr int MAX_SWEEPS_N = 30;      // 9 x 9 converges in 8-10

// one Jacobi rotation of the symmetric S (both halves kept) in the (P, Q) plane, accumulated into V
template <int P, int Q>
ORB_HD void rotate(double (&S)[4][4], double (&V)[4][4]) {
    const double apq = S[P][Q];
    if (!(apq != 0.0) || apq != apq) return;
    const double theta = (S[Q][Q] - S[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
ORB_UNROLL
    for (int k = 0; k < 4; k++) {
        if (k != P && k != Q) {
            const double skp = S[k][P], skq = S[k][Q];
            S[k][P] = S[P][k] = c * skp - s * skq;
            S[k][Q] = S[Q][k] = s * skp + c * skq;
        }
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
    S[P][P] = S[P][P] - t * apq;
    S[Q][Q] = S[Q][Q] + t * apq;
    S[P][Q] = S[Q][P] = 0.0;
}

// the right singular vector of the float A (row major) for its smallest singular value: the eigenvector of A'A for its smallest
// eigenvalue, in double, rounded to float
ORB_HD void null_vector(const float (&A)[4][4], float (&v)[4]) {
    double S[4][4], V[4][4];
ORB_UNROLL
    for (int i = 0; i < 4; i++)
ORB_UNROLL
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
ORB_UNROLL
            for (int r = 0; r < 4; r++) s = s + (double)A[r][i] * (double)A[r][j];
            S[i][j] = s;
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < MAX_SWEEPS; sweep++) {
        const double off = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[0][3] * S[0][3] + S[1][2] * S[1][2] + S[1][3] * S[1][3] + S[2][3] * S[2][3];
        const double diag = S[0][0] * S[0][0] + S[1][1] * S[1][1] + S[2][2] * S[2][2] + S[3][3] * S[3][3];
        if (!(off > 1e-36 * diag)) break;                    // converged, a zero matrix, or NaN
        rotate<0, 1>(S, V); rotate<0, 2>(S, V); rotate<0, 3>(S, V);
        rotate<1, 2>(S, V); rotate<1, 3>(S, V); rotate<2, 3>(S, V);
    }
    int k = 0;
    double best = S[0][0];
ORB_UNROLL
    for (int i = 1; i < 4; i++)
        if (S[i][i] < best) { best = S[i][i]; k = i; }
ORB_UNROLL
    for (int i = 0; i < 4; i++) v[i] = (float)(k == 0 ? V[i][0] : k == 1 ? V[i][1] : k == 2 ? V[i][2] : V[i][3]);
}

// ---- N x N over memory: S and V row major, N * N doubles each ----

// S[i][j] = sum over r of (double)A[r][i] * (double)A[r][j] (A: rows x N floats, row major), a double sum from 0.0 in row order
template <int N>
ORB_HD double gram_entry(const float* A, int rows, int i, int j) {
    double s = 0.0;
    for (int r = 0; r < rows; r++) s = s + (double)A[r * N + i] * (double)A[r * N + j];
    return s;
}

// the rule of null_vector: true while the off-diagonal part still counts (false: converged, a zero matrix, or NaN)
template <int N>
ORB_HD bool jacobi_unconverged(const double* S) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < N; i++) {
        for (int j = i + 1; j < N; j++) off = off + S[i * N + j] * S[i * N + j];
        diag = diag + S[i * N + i] * S[i * N + i];
    }
    return off > 1e-36 * diag;
}

struct Rotation { double c, s, t, apq; bool skip; };

// the angle of the rotation in the (p, q) plane, from S[p][p], S[q][q], S[p][q] alone
template <int N>
ORB_HD Rotation jacobi_angle(const double* S, int p, int q) {
    Rotation r;
    r.apq = S[p * N + q];
    r.skip = !(r.apq != 0.0) || r.apq != r.apq;
    r.c = 1.0; r.s = 0.0; r.t = 0.0;
    if (r.skip) return r;
    const double theta = (S[q * N + q] - S[p * N + p]) / (2.0 * r.apq);
    r.t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    r.c = 1.0 / sqrt(r.t * r.t + 1.0);
    r.s = r.t * r.c;
    return r;
}

// row k's share of the rotation: S[k][p], S[k][q] and their mirrors (k outside {p, q}), V[k][p], V[k][q]
template <int N>
ORB_HD void jacobi_row(double* S, double* V, int p, int q, int k, const Rotation& r) {
    if (k != p && k != q) {
        const double skp = S[k * N + p], skq = S[k * N + q];
        S[k * N + p] = S[p * N + k] = r.c * skp - r.s * skq;
        S[k * N + q] = S[q * N + k] = r.s * skp + r.c * skq;
    }
    const double vkp = V[k * N + p], vkq = V[k * N + q];
    V[k * N + p] = r.c * vkp - r.s * vkq;
    V[k * N + q] = r.s * vkp + r.c * vkq;
}

// the 2 x 2 block the rotation diagonalises
template <int N>
ORB_HD void jacobi_block(double* S, int p, int q, const Rotation& r) {
    S[p * N + p] = S[p * N + p] - r.t * r.apq;
    S[q * N + q] = S[q * N + q] + r.t * r.apq;
    S[p * N + q] = S[q * N + p] = 0.0;
}

// the column of V for the smallest diagonal entry of S (the first of equal ones)
template <int N>
ORB_HD int smallest_eigenvalue(const double* S) {
    int k = 0;
    double best = S[0];
    for (int i = 1; i < N; i++)
        if (S[i * N + i] < best) { best = S[i * N + i]; k = i; }
    return k;
}

// eigen-decomposition of the symmetric S in place (its diagonal ends as the eigenvalues), V = the eigenvectors by column; serial
template <int N>
ORB_HD void sym_eig(double* S, double* V) {
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) V[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < MAX_SWEEPS_N; sweep++) {
        if (!jacobi_unconverged<N>(S)) break;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                const Rotation r = jacobi_angle<N>(S, p, q);
                if (r.skip) continue;
                for (int k = 0; k < N; k++) jacobi_row<N>(S, V, p, q, k, r);
                jacobi_block<N>(S, p, q, r);
            }
    }
}

// ---- 3 x 3 singular value decomposition in double (the host steps of the monocular initialisation: DecomposeE, the Faugeras decomposition) ----

ORB_HD double det3(const double* M) {
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// A = U diag(w) Vt (all row major), w descending: V from the Jacobi iteration on A'A, U's columns as A v / w.  Where the smallest singular value
// is below 1e-4 of the largest (an essential matrix) A v / w is noise, and the third column of U is the cross product of the first two; either sign
// is then a singular vector.
ORB_HD void svd3(const double* A, double* U, double* w, double* Vt) {
    double S[9], V[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int r = 0; r < 3; r++) s = s + A[r * 3 + i] * A[r * 3 + j];
            S[i * 3 + j] = s;
        }
    sym_eig<3>(S, V);
    int order[3] = {0, 1, 2};
    for (int a = 0; a < 2; a++)
        for (int b = a + 1; b < 3; b++)
            if (S[order[b] * 4] > S[order[a] * 4]) { const int t = order[a]; order[a] = order[b]; order[b] = t; }
    for (int i = 0; i < 3; i++) {
        const int c = order[i];
        const double l = S[c * 4];
        w[i] = l > 0.0 ? sqrt(l) : 0.0;
        for (int j = 0; j < 3; j++) Vt[i * 3 + j] = V[j * 3 + c];
    }
    for (int i = 0; i < 3; i++) {
        if (i == 2 && !(w[2] > 1e-4 * w[0])) {
            U[2] = U[3] * U[7] - U[6] * U[4];
            U[5] = U[6] * U[1] - U[0] * U[7];
            U[8] = U[0] * U[4] - U[3] * U[1];
            break;
        }
        for (int r = 0; r < 3; r++) U[r * 3 + i] = ((A[r * 3] * Vt[i * 3] + A[r * 3 + 1] * Vt[i * 3 + 1]) + A[r * 3 + 2] * Vt[i * 3 + 2]) / w[i];
    }
}

#if defined(__HIPCC__)
// The same by a whole workgroup (every thread calls it, so that the uniform __syncthreads order its LDS traffic): S and V in LDS, thread k < N owns
// row k, thread N the 2 x 2 block; threads above N only read.  k_init_models and k_pnp_hypotheses call it with ONE wave, k_pnp_refine with four (the
// initialising stores of V by threads 64 and above repeat the same values).  Every thread reads the same three entries for the angle, so the decision
// to skip is uniform.
template <int N>
__device__ __forceinline__ void sym_eig_wave(double* S, double* V, int lane) {
    for (int e = lane; e < N * N; e += 64) V[e] = e / N == e % N ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < MAX_SWEEPS_N; sweep++) {
        if (!jacobi_unconverged<N>(S)) break;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                const Rotation r = jacobi_angle<N>(S, p, q);
                if (r.skip) continue;
                __syncthreads();                             // every lane has read the block before it changes
                if (lane < N) jacobi_row<N>(S, V, p, q, lane, r);
                if (lane == N) jacobi_block<N>(S, p, q, r);
                __syncthreads();
            }
    }
}
#endif

}  // namespace orbj
