// ORB_SLAM::PnPsolver over include/orbe.h: see PnPsolver.h.
#include "PnPsolver.h"

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

}  // namespace

PnPsolver::PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches)
    : mnKeys(vpMapPointMatches.size()), N(0), mGivenUsed(0), mDevice(0), mPending(false), mPendingIterations(0), mGivenBefore(0) {
    std::memset(&mState, 0, sizeof(mState));
    std::memset(&mReport, 0, sizeof(mReport));
    for (std::size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {          // :80-102
        MapPoint* pMP = vpMapPointMatches[i];
        if (pMP && !pMP->isBad()) {
            const cv::KeyPoint& kp = F.mvKeysUn[i];
            mP2D.push_back(kp.pt.x);
            mP2D.push_back(kp.pt.y);
            mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
            cv::Mat Pos = pMP->GetWorldPos();
            for (int j = 0; j < 3; j++) mP3D.push_back(Pos.at<float>(j));
            mvKeyPointIndices.push_back(i);
        }
    }
    fu = F.fx; fv = F.fy; uc = F.cx; vc = F.cy;
    SetRansacParameters();
}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
    N = (int)mvSigma2.size();
    mvMaxError.assign(N > 0 ? N : 1, 0.0f);
    mBestFlags.assign(N, 0);
    mRefinedFlags.assign(N, 0);
    mPending = false;
    if (N == 0) {                                                  // nothing to fit: iterate returns at once (N < mRansacMinInliers)
        mRansacMinInliers = minInliers > minSet ? minInliers : minSet;
        mRansacMaxIts = 1;
        mRansacEpsilon = epsilon;
        return;
    }
    int32_t mi = 0, mx = 0;
    require(orbe_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, th2, mvSigma2.data(), &mi, &mx, &mRansacEpsilon,
                                   mvMaxError.data()),
            "orbe_ransac_parameters");
    mRansacMinInliers = mi;
    mRansacMaxIts = mx;
}

cv::Mat PnPsolver::find(std::vector<bool>& vbInliers, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

bool PnPsolver::Prepare(int nIterations, Call& c) {
    if (N < mRansacMinInliers) return false;                       // :174-178
    const int done = mState.iterations;
    int range = (mRansacMaxIts > done + nIterations ? mRansacMaxIts : done + nIterations) - done;      // the loop condition of :183
    if (range < 1) range = 1;
    if (range > ORBE_MAX_ITERS) range = ORBE_MAX_ITERS;
    c.q = orbe_problem{fu, fv, uc, vc, N, range, mRansacMinInliers, mRansacMaxIts};
    c.sets.resize((std::size_t)range * 4);
    c.flags.assign(N, 0);
    std::vector<int> avail;
    for (int it = 0; it < range; it++) {
        if (mGivenUsed + 4 <= mGivenSets.size()) {
            for (int i = 0; i < 4; i++) c.sets[it * 4 + i] = mGivenSets[mGivenUsed + i];
            mGivenUsed += 4;
            continue;
        }
        avail.resize(N);                                           // vAvailableIndices = mvAllIndices
        for (int i = 0; i < N; i++) avail[i] = i;
        for (short i = 0; i < 4; ++i) {                            // :192-202
            const int randi = RandomInt(0, (int)avail.size() - 1);
            const int idx = avail[randi];
            c.sets[it * 4 + i] = idx;
            if ((std::size_t)idx < avail.size()) avail[idx] = avail.back();
            avail.pop_back();
        }
    }
    return true;
}

cv::Mat PnPsolver::Finish(const Call& c, bool prefetched, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    const orbe_result& r = c.result;
    mReport = Report{r.kind, r.stop, c.q.iters, mState.iterations, mState.best_inliers, prefetched};
    bNoMore = r.no_more != 0;
    if (r.kind == ORBE_KIND_NONE) return cv::Mat();
    nInliers = r.ninliers;
    vbInliers = std::vector<bool>(mnKeys, false);
    for (int i = 0; i < N; i++)
        if (c.flags[i]) vbInliers[mvKeyPointIndices[i]] = true;
    cv::Mat Tcw(4, 4, CV_32F);                                     // cv::Mat::eye with rows 0-2 from the result
    for (int i = 0; i < 12; i++) Tcw.at<float>(i) = r.tcw[i];
    Tcw.at<float>(12) = Tcw.at<float>(13) = Tcw.at<float>(14) = 0.0f;
    Tcw.at<float>(15) = 1.0f;
    return Tcw;
}

cv::Mat PnPsolver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (mPending) {
        mPending = false;
        if (mPendingIterations == nIterations) return Finish(mPendingCall, true, bNoMore, vbInliers, nInliers);
        mState = mStateBefore;                                     // another call than the one prefetched: as if Prefetch had not run
        mBestFlags = mBestBefore;
        mRefinedFlags = mRefinedBefore;
        mGivenUsed = mGivenBefore;
    }
    Call c;
    if (!Prepare(nIterations, c)) {
        bNoMore = true;
        mReport = Report{ORBE_KIND_NONE, 0, 0, mState.iterations, mState.best_inliers, false};
        return cv::Mat();
    }
    require(orbe_iterate(&c.q, mP3D.data(), mP2D.data(), mvMaxError.data(), c.sets.data(), &mState, mBestFlags.data(), mRefinedFlags.data(), &c.result,
                         c.flags.data(), mDevice),
            "orbe_iterate");
    return Finish(c, false, bNoMore, vbInliers, nInliers);
}

void PnPsolver::Prefetch(const std::vector<PnPsolver*>& vpSolvers, int nIterations) {
    std::vector<PnPsolver*> run;
    for (PnPsolver* s : vpSolvers) {
        if (!s || s->mPending || run.size() == ORBE_MAX_PROBLEMS) continue;
        s->mStateBefore = s->mState;
        s->mBestBefore = s->mBestFlags;
        s->mRefinedBefore = s->mRefinedFlags;
        s->mGivenBefore = s->mGivenUsed;
        if (s->Prepare(nIterations, s->mPendingCall)) run.push_back(s);
    }
    if (run.empty()) return;
    const std::size_t P = run.size();
    std::vector<orbe_problem> q(P);
    std::vector<const float*> p3(P), p2(P), me(P);
    std::vector<const int32_t*> st(P);
    std::vector<orbe_state> states(P);
    std::vector<orbe_result> results(P);
    std::vector<uint8_t*> bf(P), rf(P), of(P);
    for (std::size_t p = 0; p < P; p++) {
        PnPsolver* s = run[p];
        q[p] = s->mPendingCall.q;
        p3[p] = s->mP3D.data(); p2[p] = s->mP2D.data(); me[p] = s->mvMaxError.data();
        st[p] = s->mPendingCall.sets.data();
        states[p] = s->mState;
        bf[p] = s->mBestFlags.data(); rf[p] = s->mRefinedFlags.data(); of[p] = s->mPendingCall.flags.data();
    }
    const int rc = orbe_iterate_batch(q.data(), (int)P, p3.data(), p2.data(), me.data(), st.data(), states.data(), bf.data(), rf.data(), results.data(),
                                      of.data(), run[0]->mDevice);
    if (rc != ORBX_OK) {                                           // every solver as it was, apart from the rand() values its draw consumed
        for (PnPsolver* s : run) {
            s->mBestFlags = s->mBestBefore;
            s->mRefinedFlags = s->mRefinedBefore;
            s->mGivenUsed = s->mGivenBefore;
        }
        require(rc, "orbe_iterate_batch");
    }
    for (std::size_t p = 0; p < P; p++) {
        run[p]->mState = states[p];
        run[p]->mPendingCall.result = results[p];
        run[p]->mPending = true;
        run[p]->mPendingIterations = nIterations;
    }
}

}  // namespace ORB_SLAM
