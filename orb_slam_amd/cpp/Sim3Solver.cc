// ORB_SLAM::Sim3Solver over include/orbh.h: see Sim3Solver.h.  Compile with -ffp-contract=off: the constructor's float text is pinned.
#include "Sim3Solver.h"

#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace ORB_SLAM {

namespace {

void require(int rc, const char* what) {
    if (rc != ORBX_OK) throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc));
}

// DUtils::Random::RandomInt(min, max) (Thirdparty/DBoW2/DUtils/Random.cpp)
int RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

// Rcw*X3Dw + tcw (:95, :98): a cv::Mat product accumulates `float s = 0; s += a*b` in k order
void ToCamera(const cv::Mat& Rcw, const cv::Mat& tcw, const cv::Mat& Xw, std::vector<float>& out) {
    for (int y = 0; y < 3; y++) {
        float s = 0.0f;
        for (int k = 0; k < 3; k++) s = s + Rcw.at<float>(y, k) * Xw.at<float>(k);
        out.push_back(s + tcw.at<float>(y));
    }
}

// FromCameraToImage (:400-418)
void ToImage(const std::vector<float>& X, const float* K, std::vector<float>& out) {
    out.clear();
    for (std::size_t i = 0; i + 2 < X.size(); i += 3) {
        const float invz = 1 / X[i + 2];
        const float x = X[i] * invz, y = X[i + 1] * invz;
        out.push_back(K[0] * x + K[2]);
        out.push_back(K[1] * y + K[3]);
    }
}

}  // namespace

Sim3Solver::Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12)
    : mN1((int)vpMatched12.size()), N(0), mnIterations(0), mnBestInliers(0), mBestScale(0.0f), mCached(0), mGivenUsed(0), mDevice(0) {
    std::memset(&mReport, 0, sizeof(mReport));
    std::memset(mBestT12, 0, sizeof(mBestT12));
    std::memset(mBestR, 0, sizeof(mBestR));
    std::memset(mBestt, 0, sizeof(mBestt));
    std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    const cv::Mat Rcw1 = pKF1->GetRotation(), tcw1 = pKF1->GetTranslation(), Rcw2 = pKF2->GetRotation(), tcw2 = pKF2->GetTranslation();
    std::vector<float> sigma1, sigma2;
    for (int i1 = 0; i1 < mN1; i1++) {                             // :62-103
        if (!vpMatched12[i1]) continue;
        MapPoint* pMP1 = vpKeyFrameMP1[i1];
        MapPoint* pMP2 = vpMatched12[i1];
        if (!pMP1) continue;
        if (pMP1->isBad() || pMP2->isBad()) continue;
        const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
        const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;
        const cv::KeyPoint kp1 = pKF1->GetKeyPointUn(indexKF1);
        const cv::KeyPoint kp2 = pKF2->GetKeyPointUn(indexKF2);
        sigma1.push_back(pKF1->GetSigma2(kp1.octave));
        sigma2.push_back(pKF2->GetSigma2(kp2.octave));
        mvnIndices1.push_back(i1);
        ToCamera(Rcw1, tcw1, pMP1->GetWorldPos(), mX3Dc1);
        ToCamera(Rcw2, tcw2, pMP2->GetWorldPos(), mX3Dc2);
    }
    N = (int)mvnIndices1.size();
    mMaxError1.assign(N > 0 ? N : 1, 0.0f);
    mMaxError2.assign(N > 0 ? N : 1, 0.0f);
    require(orbh_max_errors(N, sigma1.data(), mMaxError1.data()), "orbh_max_errors");
    require(orbh_max_errors(N, sigma2.data(), mMaxError2.data()), "orbh_max_errors");
    mK1[0] = pKF1->fx; mK1[1] = pKF1->fy; mK1[2] = pKF1->cx; mK1[3] = pKF1->cy;
    mK2[0] = pKF2->fx; mK2[1] = pKF2->fy; mK2[2] = pKF2->cx; mK2[3] = pKF2->cy;
    ToImage(mX3Dc1, mK1, mP1im1);
    ToImage(mX3Dc2, mK2, mP2im2);
    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    int32_t mx = 1;
    require(orbh_ransac_parameters(N, probability, minInliers, maxIterations, &mx), "orbh_ransac_parameters");
    mRansacMaxIts = mx;
    mnIterations = 0;                                              // :137 (mnBestInliers and the best keep their values, as in the source)
    mBestFlags.resize(ORBH_WORDS(N > 0 ? N : 1), 0);
    mCached = 0;
    mHyp.clear();
    mFlags.clear();
}

cv::Mat Sim3Solver::find(std::vector<bool>& vbInliers12, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

bool Sim3Solver::WantsFetch() const { return N >= 3 && N >= mRansacMinInliers && mCached < mRansacMaxIts; }

int Sim3Solver::PrepareFetch(orbh_problem& q, std::vector<int32_t>& sets) {
    int count = mRansacMaxIts - mCached;
    if (count > ORBH_MAX_ITERS) count = ORBH_MAX_ITERS;
    q = orbh_problem{mK1[0], mK1[1], mK1[2], mK1[3], mK2[0], mK2[1], mK2[2], mK2[3], N, count, mRansacMinInliers < 0 ? 0 : mRansacMinInliers, mRansacMaxIts};
    sets.resize((std::size_t)count * 3);
    std::vector<int> avail;
    for (int it = 0; it < count; it++) {
        if (mGivenUsed + 3 <= mGivenSets.size()) {
            for (int i = 0; i < 3; i++) sets[it * 3 + i] = mGivenSets[mGivenUsed + i];
            mGivenUsed += 3;
            continue;
        }
        avail.resize(N);                                           // vAvailableIndices = mvAllIndices
        for (int i = 0; i < N; i++) avail[i] = i;
        for (short i = 0; i < 3; ++i) {                            // :166-177
            const int randi = RandomInt(0, (int)avail.size() - 1);
            const int idx = avail[randi];
            sets[it * 3 + i] = idx;
            if ((std::size_t)idx < avail.size()) avail[idx] = avail.back();
            avail.pop_back();
        }
    }
    return count;
}

void Sim3Solver::TakeFetch(int count, const std::vector<orbh_hyp>& hyp, const std::vector<uint64_t>& flags) {
    mHyp.insert(mHyp.end(), hyp.begin(), hyp.begin() + count);
    mFlags.insert(mFlags.end(), flags.begin(), flags.begin() + (std::size_t)count * ORBH_WORDS(N));
    mCached += count;
}

void Sim3Solver::FetchAlone() {
    orbh_problem q;
    std::vector<int32_t> sets;
    const std::size_t given = mGivenUsed;
    const int count = PrepareFetch(q, sets);
    std::vector<orbh_hyp> hyp(count);
    std::vector<uint64_t> flags((std::size_t)count * ORBH_WORDS(N)), bf(ORBH_WORDS(N), 0), rf(ORBH_WORDS(N), 0);
    orbh_state st;                                                 // the C ABI's walk runs over a scratch state: the class walks for itself
    orbh_result res;
    std::memset(&st, 0, sizeof(st));
    const int rc = orbh_iterate(&q, mX3Dc1.data(), mX3Dc2.data(), mP1im1.data(), mP2im2.data(), mMaxError1.data(), mMaxError2.data(), sets.data(), &st,
                                bf.data(), &res, rf.data(), hyp.data(), flags.data(), mDevice);
    if (rc != ORBX_OK) mGivenUsed = given;
    require(rc, "orbh_iterate");
    TakeFetch(count, hyp, flags);
}

void Sim3Solver::Prefetch(const std::vector<Sim3Solver*>& vpSolvers) {
    std::vector<Sim3Solver*> todo;
    for (Sim3Solver* s : vpSolvers)
        if (s && s->WantsFetch()) todo.push_back(s);
    while (!todo.empty()) {
        const std::size_t P = todo.size() < ORBH_MAX_PROBLEMS ? todo.size() : ORBH_MAX_PROBLEMS;
        std::vector<orbh_problem> q(P);
        std::vector<std::vector<int32_t> > sets(P);
        std::vector<std::vector<orbh_hyp> > hyp(P);
        std::vector<std::vector<uint64_t> > flags(P), bf(P), rf(P);
        std::vector<const float*> x1(P), x2(P), u1(P), u2(P), m1(P), m2(P);
        std::vector<const int32_t*> st(P);
        std::vector<uint64_t*> pbf(P), prf(P), pfl(P);
        std::vector<orbh_hyp*> phy(P);
        std::vector<orbh_state> states(P);
        std::vector<orbh_result> results(P);
        std::vector<std::size_t> given(P);
        std::vector<int> count(P);
        std::memset(states.data(), 0, P * sizeof(orbh_state));
        for (std::size_t p = 0; p < P; p++) {
            Sim3Solver* s = todo[p];
            given[p] = s->mGivenUsed;
            count[p] = s->PrepareFetch(q[p], sets[p]);
            const std::size_t W = ORBH_WORDS(s->N);
            hyp[p].resize(count[p]); flags[p].resize(count[p] * W); bf[p].assign(W, 0); rf[p].assign(W, 0);
            x1[p] = s->mX3Dc1.data(); x2[p] = s->mX3Dc2.data(); u1[p] = s->mP1im1.data(); u2[p] = s->mP2im2.data();
            m1[p] = s->mMaxError1.data(); m2[p] = s->mMaxError2.data();
            st[p] = sets[p].data(); pbf[p] = bf[p].data(); prf[p] = rf[p].data(); pfl[p] = flags[p].data(); phy[p] = hyp[p].data();
        }
        const int rc = orbh_iterate_batch(q.data(), (int)P, x1.data(), x2.data(), u1.data(), u2.data(), m1.data(), m2.data(), st.data(), states.data(),
                                          pbf.data(), results.data(), prf.data(), phy.data(), pfl.data(), todo[0]->mDevice);
        if (rc != ORBX_OK) {                                       // every solver as it was, apart from the rand() values its draw consumed
            for (std::size_t p = 0; p < P; p++) todo[p]->mGivenUsed = given[p];
            require(rc, "orbh_iterate_batch");
        }
        std::vector<Sim3Solver*> next;
        for (std::size_t p = 0; p < P; p++) {
            todo[p]->TakeFetch(count[p], hyp[p], flags[p]);
            if (todo[p]->WantsFetch()) next.push_back(todo[p]);   // a range longer than ORBH_MAX_ITERS
        }
        next.insert(next.end(), todo.begin() + P, todo.end());
        todo.swap(next);
    }
}

cv::Mat Sim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    mReport = Report{0, 0, mnIterations, mnBestInliers, 0, mCached};
    if (N < mRansacMinInliers || N < 3) {                          // :146-150
        bNoMore = true;
        return cv::Mat();
    }
    const std::size_t W = ORBH_WORDS(N);
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {      // :158
        if (mnIterations >= mCached) {
            FetchAlone();
            mReport.deviceCalls++;
        }
        nCurrentIterations++;
        const orbh_hyp& h = mHyp[mnIterations];
        const uint64_t* fl = &mFlags[(std::size_t)mnIterations * W];
        mnIterations++;
        if (h.count >= mnBestInliers) {                            // :183-190
            mBestFlags.assign(fl, fl + W);
            mnBestInliers = h.count;
            std::memcpy(mBestT12, h.T12, sizeof(mBestT12));
            std::memcpy(mBestR, h.R, sizeof(mBestR));
            std::memcpy(mBestt, h.t, sizeof(mBestt));
            mBestScale = h.s;
            if (h.count > mRansacMinInliers) {                     // :192-199
                nInliers = h.count;
                for (int i = 0; i < N; i++)
                    if ((fl[i / 64] >> (i % 64)) & 1) vbInliers[mvnIndices1[i]] = true;
                mReport = Report{1, nCurrentIterations, mnIterations, mnBestInliers, mReport.deviceCalls, mCached};
                cv::Mat T(4, 4, CV_32F);
                for (int i = 0; i < 16; i++) T.at<float>(i) = mBestT12[i];
                return T;
            }
        }
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    mReport = Report{0, nCurrentIterations, mnIterations, mnBestInliers, mReport.deviceCalls, mCached};
    return cv::Mat();
}

cv::Mat Sim3Solver::GetEstimatedRotation() {
    cv::Mat R(3, 3, CV_32F);
    for (int i = 0; i < 9; i++) R.at<float>(i) = mBestR[i];
    return R;
}

cv::Mat Sim3Solver::GetEstimatedTranslation() {
    cv::Mat t(3, 1, CV_32F);
    for (int i = 0; i < 3; i++) t.at<float>(i) = mBestt[i];
    return t;
}

float Sim3Solver::GetEstimatedScale() { return mBestScale; }

}  // namespace ORB_SLAM
