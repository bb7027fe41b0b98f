// The host route tools/bench_init.py measures the device chain of the monocular initialisation against: the same algorithm (include/orbi.h) on one
// host core over flat arrays, with the same double Jacobi iteration (orb_slam_amd/csrc/orb_jacobi.h) and the same arithmetic text
// (orb_slam_amd/csrc/orbi_math.h).  tests/test_init_host.py holds it against the numpy restatement.  Build with -ffp-contract=off.
#include <cstring>
#include <vector>

#include "orbi_math.h"

namespace {

bool match_points(const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2, const int32_t* matches, int i, float& u1, float& v1, float& u2,
                  float& v2) {
    const int i1 = matches[i * 2], i2 = matches[i * 2 + 1];
    if (i1 < 0 || i1 >= n1 || i2 < 0 || i2 >= n2) return false;
    u1 = k1[i1].x; v1 = k1[i1].y;
    u2 = k2[i2].x; v2 = k2[i2].y;
    return true;
}

// the unit null vector of the rows x 9 float A, rounded to float
void null9(const float* A, int rows, float* vec) {
    double S[81], V[81];
    for (int e = 0; e < 81; e++) S[e] = orbj::gram_entry<9>(A, rows, e / 9, e % 9);
    orbj::sym_eig<9>(S, V);
    const int k = orbj::smallest_eigenvalue<9>(S);
    for (int i = 0; i < 9; i++) vec[i] = (float)V[i * 9 + k];
}

}  // namespace

extern "C" {

// orbi_models on the host
int init_host_models(const orbi_problem* q, const orbx_keypoint* kps1, const orbx_keypoint* kps2, const int32_t* matches, const int32_t* sets,
                     float* scoreH, float* scoreF, float* H21, float* H12, float* F21, float* hn, float* fpre, int32_t* best, float* S, uint8_t* inlH,
                     uint8_t* inlF) {
    const int N = q->nmatches, n1 = q->n1, n2 = q->n2;
    const float iss = orbi::inv_sigma_square(q->sigma);
    std::vector<uint8_t> cur(N);
    best[0] = best[1] = -1;
    S[0] = S[1] = 0.0f;
    std::memset(inlH, 0, N);
    std::memset(inlF, 0, N);
    for (int model = 0; model < 2; model++)
        for (int it = 0; it < q->iters; it++) {
            float A[16 * 9], vec[9], m1[9], m2[9];
            bool bad = false;
            for (int j = 0; j < 8 && !bad; j++) {
                const int idx = sets[it * 8 + j];
                float u1, v1, u2, v2;
                if (idx < 0 || idx >= N || !match_points(kps1, n1, kps2, n2, matches, idx, u1, v1, u2, v2)) { bad = true; break; }
                u1 = (u1 - q->norm1[2]) * q->norm1[0]; v1 = (v1 - q->norm1[3]) * q->norm1[1];
                u2 = (u2 - q->norm2[2]) * q->norm2[0]; v2 = (v2 - q->norm2[3]) * q->norm2[1];
                if (model == 0) {
                    orbi::homography_row(0, u1, v1, u2, v2, A + (2 * j) * 9);
                    orbi::homography_row(1, u1, v1, u2, v2, A + (2 * j + 1) * 9);
                } else {
                    orbi::fundamental_row(u1, v1, u2, v2, A + j * 9);
                }
            }
            float* out1 = (model == 0 ? H21 : F21) + it * 9;
            float* vout = model == 0 ? hn : fpre;
            float* score = model == 0 ? scoreH : scoreF;
            if (bad) {
                for (int i = 0; i < 9; i++) {
                    out1[i] = 0.0f;
                    if (model == 0) H12[it * 9 + i] = 0.0f;
                    if (vout) vout[it * 9 + i] = 0.0f;
                }
                score[it] = 0.0f;
                continue;
            }
            null9(A, model == 0 ? 16 : 8, vec);
            if (vout) std::memcpy(vout + it * 9, vec, sizeof(vec));
            if (model == 0) {
                orbi::homography_chain(vec, q->norm1, q->norm2, m1, m2);
                std::memcpy(H12 + it * 9, m2, sizeof(m2));
            } else {
                double S3[9], V3[9];
                orbi::gram3(vec, S3);
                orbj::sym_eig<3>(S3, V3);
                orbi::fundamental_chain(vec, V3, orbj::smallest_eigenvalue<3>(S3), q->norm1, q->norm2, m1);
            }
            std::memcpy(out1, m1, sizeof(m1));
            float s = 0.0f;
            for (int i = 0; i < N; i++) {
                orbi::Terms t = {0.0f, 0.0f, false};
                float u1, v1, u2, v2;
                if (match_points(kps1, n1, kps2, n2, matches, i, u1, v1, u2, v2))
                    t = model == 0 ? orbi::homography_terms(m1, m2, u1, v1, u2, v2, iss) : orbi::fundamental_terms(m1, u1, v1, u2, v2, iss);
                s = s + t.t1;
                s = s + t.t2;
                cur[i] = t.in ? 1 : 0;
            }
            score[it] = s;
            if (s > S[model]) {
                S[model] = s;
                best[model] = it;
                std::memcpy(model == 0 ? inlH : inlF, cur.data(), N);
            }
        }
    return 0;
}

// orbi_check_rt on the host
int init_host_check_rt(float fx, float fy, float cx, float cy, const orbi_pose* poses, int nhyp, const orbx_keypoint* kps1, int n1,
                       const orbx_keypoint* kps2, int n2, const int32_t* matches, int nmatches, const uint8_t* flags, float th2, uint8_t* status,
                       float* x3d, float* cosp, uint8_t* good, float* v, int32_t* ngood, float* parallax) {
    std::vector<float> counted;
    for (int h = 0; h < nhyp; h++) {
        counted.clear();
        for (int i = 0; i < nmatches; i++) {
            orbi::RtOut o;
            std::memset(&o, 0, sizeof(o));
            o.status = ORBI_RT_NONE;
            if (flags[i]) {
                float u1, v1, u2, v2;
                if (match_points(kps1, n1, kps2, n2, matches, i, u1, v1, u2, v2)) orbi::check_rt_one(fx, fy, cx, cy, poses[h], u1, v1, u2, v2, th2, o);
                else o.status = ORBI_RT_SKIP_INDEX;
            }
            const size_t e = (size_t)h * nmatches + i;
            status[e] = (uint8_t)o.status;
            for (int j = 0; j < 3; j++) x3d[e * 3 + j] = o.X[j];
            cosp[e] = o.cosp;
            good[e] = o.status == ORBI_RT_GOOD;
            if (v) for (int j = 0; j < 4; j++) v[e * 4 + j] = o.v[j];
            if (o.status == ORBI_RT_GOOD || o.status == ORBI_RT_COUNTED) counted.push_back(o.cosp);
        }
        ngood[h] = (int)counted.size();
        parallax[h] = orbi::parallax_of(counted.data(), (int)counted.size());
    }
    return 0;
}

// The C ABI of include/orbi.h over the two functions above, so that code written against the library (orb_slam_amd/cpp/Initializer.cc) links against
// this file instead and runs the whole of Initialize on the host: what tests/init_dropin/harness_host and tools/bench_init.py use.  `device` is ignored.
int orbi_normalize(const orbx_keypoint* kps, int n, float* out) {
    if (!kps || !out || n < 1) return ORBX_ERR_ARG;
    orbi::normalize(kps, n, out);
    return ORBX_OK;
}

int orbi_pose_from_rt(float fx, float fy, float cx, float cy, const float* R, const float* t, orbi_pose* pose) {
    if (!R || !t || !pose) return ORBX_ERR_ARG;
    orbi::pose_from_rt(fx, fy, cx, cy, R, t, pose);
    return ORBX_OK;
}

int orbi_models(const orbi_problem* problem, const orbx_keypoint* kps1, const orbx_keypoint* kps2, const int32_t* matches, const int32_t* sets,
                float* scoreH, float* scoreF, float* H21, float* H12, float* F21, float* hn, float* fpre, int32_t* best, float* S,
                uint8_t* inlH, uint8_t* inlF, int) {
    return init_host_models(problem, kps1, kps2, matches, sets, scoreH, scoreF, H21, H12, F21, hn, fpre, best, S, inlH, inlF);
}

int orbi_check_rt(float fx, float fy, float cx, float cy, const orbi_pose* poses, int nhyp, const orbx_keypoint* kps1, int n1,
                  const orbx_keypoint* kps2, int n2, const int32_t* matches, int nmatches, const uint8_t* flags, float th2, uint8_t* status,
                  float* x3d, float* cosp, uint8_t* good, float* v, int32_t* ngood, float* parallax, int) {
    return init_host_check_rt(fx, fy, cx, cy, poses, nhyp, kps1, n1, kps2, n2, matches, nmatches, flags, th2, status, x3d, cosp, good, v, ngood, parallax);
}

}  // extern "C"
