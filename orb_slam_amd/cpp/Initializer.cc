// ORB_SLAM::Initializer over include/orbi.h: see Initializer.h.  The decompositions are this file's own statement of DecomposeE (E = U diag(1,1,0) V',
// R = U W V' or U W' V', t = the last column of U) and of Faugeras and Lustman's eight solutions for a homography (Motion and structure from motion in
// a piecewise planar environment, 1988), in double over the 3 x 3 SVD of orb_jacobi.h; the hypotheses are listed in the reference's order, because
// its acceptance rules (src/Initializer.cc:497-567, :719-729) depend on it.
#include "Initializer.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "orb_jacobi.h"
#include "orbi.h"

namespace ORB_SLAM {

namespace {

static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "cv::KeyPoint is OpenCV 2.4's 28-byte layout");

void check(int rc, const char* what) {
    if (rc != ORBX_OK) throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc));
}

// Thirdparty/DBoW2/DUtils/Random.cpp:47-50 over rand()
int RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}

void transpose3(const double* A, double* T) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[i * 3 + j] = A[j * 3 + i];
}

struct Motion { float R[9], t[3]; };

Motion motion(const double* R, const double* t, double sign) {
    const double n = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    Motion m;
    for (int i = 0; i < 9; i++) m.R[i] = (float)(sign * R[i]);
    for (int i = 0; i < 3; i++) m.t[i] = (float)(t[i] / n);
    return m;
}

// E = K' F K, then (R1, t), (R2, t), (R1, -t), (R2, -t): the order of src/Initializer.cc:492-495
void motions_from_fundamental(const double* K, const float* F21, std::vector<Motion>& out) {
    double F[9], Kt[9], FK[9], E[9], U[9], w[3], Vt[9];
    for (int i = 0; i < 9; i++) F[i] = (double)F21[i];
    transpose3(K, Kt);
    mul3(F, K, FK);
    mul3(Kt, FK, E);
    orbj::svd3(E, U, w, Vt);
    const double W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    double UW[9], R1[9], R2[9];
    mul3(U, W, UW);
    mul3(UW, Vt, R1);
    mul3(U, Wt, UW);
    mul3(UW, Vt, R2);
    const double s1 = orbj::det3(R1) < 0 ? -1.0 : 1.0, s2 = orbj::det3(R2) < 0 ? -1.0 : 1.0;
    const double t[3] = {U[2], U[5], U[8]}, tn[3] = {-U[2], -U[5], -U[8]};
    out.push_back(motion(R1, t, s1));
    out.push_back(motion(R2, t, s2));
    out.push_back(motion(R1, tn, s1));
    out.push_back(motion(R2, tn, s2));
}

// A = inv(K) H K = U diag(d1, d2, d3) V'; false when two singular values coincide (the rule of :595).  Eight solutions: for d' = d2 the
// rotation about the second axis by +-theta, for d' = -d2 the reflected one, each with the four sign choices of the plane normal (x1, 0, x3).
bool motions_from_homography(const double* K, const float* H21, std::vector<Motion>& out) {
    double H[9], Ki[9], HK[9], A[9], U[9], w[3], Vt[9];
    for (int i = 0; i < 9; i++) H[i] = (double)H21[i];
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double inv[9] = {1.0 / fx, 0, -cx / fx, 0, 1.0 / fy, -cy / fy, 0, 0, 1};
    std::memcpy(Ki, inv, sizeof(inv));
    mul3(H, K, HK);
    mul3(Ki, HK, A);
    orbj::svd3(A, U, w, Vt);
    const double s = orbj::det3(U) * orbj::det3(Vt);
    const float d1 = (float)w[0], d2 = (float)w[1], d3 = (float)w[2];
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
    const double a = w[0] * w[0], b = w[1] * w[1], c = w[2] * w[2];
    const double x1 = std::sqrt((a - b) / (a - c)), x3 = std::sqrt((b - c) / (a - c));
    const double e1[4] = {1, 1, -1, -1}, e3[4] = {1, -1, 1, -1};
    const double root = std::sqrt((a - b) * (b - c));
    for (int reflected = 0; reflected < 2; reflected++) {
        const double denom = (reflected ? w[0] - w[2] : w[0] + w[2]) * w[1];
        const double sn = root / denom, cs = reflected ? (w[0] * w[2] - b) / denom : (b + w[0] * w[2]) / denom;
        const double turn[4] = {sn, -sn, -sn, sn};
        for (int i = 0; i < 4; i++) {
            double Rp[9] = {cs, 0, -turn[i], 0, 1, 0, turn[i], 0, cs};
            if (reflected) { Rp[2] = turn[i]; Rp[4] = -1; Rp[8] = -cs; }
            double URp[9], R[9];
            mul3(U, Rp, URp);
            mul3(URp, Vt, R);
            const double scale = reflected ? w[0] + w[2] : w[0] - w[2];
            const double tp[3] = {e1[i] * x1 * scale, 0.0, (reflected ? 1.0 : -1.0) * e3[i] * x3 * scale};
            const double t[3] = {U[0] * tp[0] + U[2] * tp[2], U[3] * tp[0] + U[5] * tp[2], U[6] * tp[0] + U[8] * tp[2]};
            out.push_back(motion(R, t, s));
        }
    }
    return true;
}

}  // namespace

Initializer::Initializer(const Frame& ReferenceFrame, float sigma, int iterations) : mDevice(0) {
    mK = ReferenceFrame.mK.clone();
    mvKeys1 = ReferenceFrame.mvKeysUn;
    mSigma = sigma;
    mSigma2 = sigma * sigma;
    mMaxIterations = iterations;
    mReport = Report();
}

bool Initializer::Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                             std::vector<bool>& vbTriangulated) {
    // Reference Frame: 1, Current Frame: 2
    mvKeys2 = CurrentFrame.mvKeysUn;
    mvMatches12.clear();
    mvMatches12.reserve(mvKeys2.size());
    mvbMatched1.assign(mvKeys1.size(), false);
    for (std::size_t i = 0; i < vMatches12.size() && i < mvKeys1.size(); i++)
        if (vMatches12[i] >= 0) {
            mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
            mvbMatched1[i] = true;
        }
    const int N = (int)mvMatches12.size();
    mReport = Report();
    mReport.chosen = -1;
    mReport.bestH = mReport.bestF = -1;
    R21 = cv::Mat();
    t21 = cv::Mat();
    if (N < 8 || N > ORBI_MAX_MATCHES || mMaxIterations < 1 || mMaxIterations > ORBI_MAX_ITERS || mvKeys1.empty() || mvKeys2.empty()) return false;

    // the sets of 8 matches of every iteration: each drawn without replacement, as src/Initializer.cc:80-95
    if (!mvGivenSets.empty()) {
        mvSets = mvGivenSets;
    } else {
        mvSets.assign(mMaxIterations, std::vector<std::size_t>(8, 0));
        std::vector<std::size_t> all(N), available;
        for (int i = 0; i < N; i++) all[i] = i;
        for (int it = 0; it < mMaxIterations; it++) {
            available = all;
            for (int j = 0; j < 8; j++) {
                const int r = RandomInt(0, (int)available.size() - 1);
                mvSets[it][j] = available[r];
                available[r] = available.back();
                available.pop_back();
            }
        }
    }
    const int iters = (int)mvSets.size();
    if (iters < 1 || iters > ORBI_MAX_ITERS) return false;
    std::vector<int32_t> matches(2 * (std::size_t)N), sets(8 * (std::size_t)iters);
    for (int i = 0; i < N; i++) { matches[2 * i] = mvMatches12[i].first; matches[2 * i + 1] = mvMatches12[i].second; }
    for (int it = 0; it < iters; it++)
        for (int j = 0; j < 8; j++) sets[it * 8 + j] = j < (int)mvSets[it].size() ? (int32_t)mvSets[it][j] : -1;

    const orbx_keypoint* k1 = reinterpret_cast<const orbx_keypoint*>(mvKeys1.data());
    const orbx_keypoint* k2 = reinterpret_cast<const orbx_keypoint*>(mvKeys2.data());
    orbi_problem q;
    std::memset(&q, 0, sizeof(q));
    check(orbi_normalize(k1, (int)mvKeys1.size(), q.norm1), "orbi_normalize");
    check(orbi_normalize(k2, (int)mvKeys2.size(), q.norm2), "orbi_normalize");
    q.sigma = mSigma; q.n1 = (int)mvKeys1.size(); q.n2 = (int)mvKeys2.size(); q.nmatches = N; q.iters = iters;

    // FindHomography + FindFundamental: first synchronisation
    std::vector<float> scoreH(iters), scoreF(iters), H21((std::size_t)iters * 9), H12((std::size_t)iters * 9), F21((std::size_t)iters * 9);
    std::vector<unsigned char> inlH(N), inlF(N);
    int32_t best[2];
    float S[2];
    check(orbi_models(&q, k1, k2, matches.data(), sets.data(), scoreH.data(), scoreF.data(), H21.data(), H12.data(), F21.data(), 0, 0, best, S, inlH.data(),
                      inlF.data(), mDevice), "orbi_models");
    const float SH = S[0], SF = S[1];
    const float RH = SH / (SH + SF);
    mReport.SH = SH; mReport.SF = SF; mReport.RH = RH; mReport.bestH = best[0]; mReport.bestF = best[1];
    mMatchesFlat.swap(matches);

    // Try to reconstruct from homography or fundamental depending on the ratio (0.40-0.45)
    if (RH > 0.40) {
        if (best[0] < 0) return false;
        mReport.model = 'H';
        return Reconstruct(true, &H21[(std::size_t)best[0] * 9], inlH.data(), R21, t21, vP3D, vbTriangulated, 1.0f, 50);
    }
    if (best[1] < 0) return false;
    mReport.model = 'F';
    return Reconstruct(false, &F21[(std::size_t)best[1] * 9], inlF.data(), R21, t21, vP3D, vbTriangulated, 1.0f, 50);
}

bool Initializer::Reconstruct(bool homography, const float* M, const unsigned char* inliers, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                              std::vector<bool>& vbTriangulated, float minParallax, int minTriangulated) {
    const int Nm = (int)mvMatches12.size();
    int N = 0;
    for (int i = 0; i < Nm; i++)
        if (inliers[i]) N++;
    mReport.nInliers = N;
    const float fx = mK.at<float>(0, 0), fy = mK.at<float>(1, 1), cx = mK.at<float>(0, 2), cy = mK.at<float>(1, 2);
    const double K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
    std::vector<Motion> hyp;
    if (homography) {
        if (!motions_from_homography(K, M, hyp)) return false;
    } else {
        motions_from_fundamental(K, M, hyp);
    }
    const int nhyp = (int)hyp.size();
    std::vector<orbi_pose> poses(nhyp);
    for (int h = 0; h < nhyp; h++) check(orbi_pose_from_rt(fx, fy, cx, cy, hyp[h].R, hyp[h].t, &poses[h]), "orbi_pose_from_rt");

    // every CheckRT at once: second synchronisation
    const std::size_t HN = (std::size_t)nhyp * Nm;
    std::vector<unsigned char> status(HN), good(HN);
    std::vector<float> x3d(HN * 3), cosp(HN), parallax(nhyp);
    std::vector<int32_t> ngood(nhyp);
    check(orbi_check_rt(fx, fy, cx, cy, poses.data(), nhyp, reinterpret_cast<const orbx_keypoint*>(mvKeys1.data()), (int)mvKeys1.size(),
                        reinterpret_cast<const orbx_keypoint*>(mvKeys2.data()), (int)mvKeys2.size(), mMatchesFlat.data(), Nm, inliers, 4.0f * mSigma2,
                        status.data(), x3d.data(), cosp.data(), good.data(), 0, ngood.data(), parallax.data(), mDevice), "orbi_check_rt");
    mReport.nGood.assign(ngood.begin(), ngood.end());
    mReport.parallax = parallax;

    int chosen = -1;
    if (homography) {
        // :687-729: the best and the second best count in hypothesis order
        int bestGood = 0, secondBestGood = 0, bestIdx = -1;
        float bestParallax = -1;
        for (int i = 0; i < nhyp; i++) {
            if (ngood[i] > bestGood) { secondBestGood = bestGood; bestGood = ngood[i]; bestIdx = i; bestParallax = parallax[i]; }
            else if (ngood[i] > secondBestGood) secondBestGood = ngood[i];
        }
        if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * N) chosen = bestIdx;
    } else {
        // :497-567: a clear winner with enough points; the FIRST hypothesis that reaches the maximum is the only one asked for its parallax
        const int maxGood = *std::max_element(ngood.begin(), ngood.end());
        const int nMinGood = std::max(static_cast<int>(0.9 * N), minTriangulated);
        int nsimilar = 0;
        for (int i = 0; i < nhyp; i++)
            if (ngood[i] > 0.7 * maxGood) nsimilar++;
        if (!(maxGood < nMinGood || nsimilar > 1)) {
            int first = 0;
            while (ngood[first] != maxGood) first++;
            if (parallax[first] > minParallax) chosen = first;
        }
    }
    mReport.chosen = chosen;
    if (chosen < 0) return false;

    // vP3D and vbGood of the chosen CheckRT, by key point of frame 1 (:806-807, :886-891)
    vP3D.assign(mvKeys1.size(), cv::Point3f());
    vbTriangulated.assign(mvKeys1.size(), false);
    for (int i = 0; i < Nm; i++) {
        const std::size_t e = (std::size_t)chosen * Nm + i;
        if (status[e] != ORBI_RT_GOOD && status[e] != ORBI_RT_COUNTED) continue;
        const int k = mvMatches12[i].first;
        vP3D[k].x = x3d[e * 3]; vP3D[k].y = x3d[e * 3 + 1]; vP3D[k].z = x3d[e * 3 + 2];
        if (good[e]) vbTriangulated[k] = true;
    }
    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int i = 0; i < 9; i++) R21.at<float>(i / 3, i % 3) = hyp[chosen].R[i];
    for (int i = 0; i < 3; i++) t21.at<float>(i) = hyp[chosen].t[i];
    return true;
}

}  // namespace ORB_SLAM
