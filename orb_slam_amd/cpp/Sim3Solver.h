// ORB_SLAM::Sim3Solver — the reference's loop-closing solver (include/Sim3Solver.h:36-53, src/Sim3Solver.cc) with its arithmetic on the MI355X
// (include/orbh.h): the reference's constructor, SetRansacParameters, find, iterate and the three getters.  Host C++ written against the reference's
// member names (KeyFrame::GetMapPointMatches, GetRotation, GetTranslation, GetKeyPointUn, GetSigma2, fx, fy, cx, cy; MapPoint::isBad, GetWorldPos,
// GetIndexInKeyFrame); links the C ABI only (swap Sim3Solver.h + .cc).
//   host:    the correspondences with the reference's rules (:62-103: a NULL match, a NULL pMP1, a bad point and an index < 0 are skipped; mvnIndices1
//            is kept), Rcw*X3Dw+tcw and FromCameraToImage in the float text of orbh.h, the max errors (orbh_max_errors), SetRansacParameters
//            (orbh_ransac_parameters), the draw of the sets with the reference's DUtils::Random::RandomInt expression over rand() and its
//            `vAvailableIndices[idx] = vAvailableIndices.back()` (idx, not randi; the write is made only where idx < size(), which is what every later
//            read of the source sees), the walk of iterate() over the cached hypotheses, vbInliers by index of vpMatched12;
//   device:  every hypothesis of every remaining iteration up to mRansacMaxIts in ONE call: Prefetch for all solvers of a ComputeSim3 together
//            (orbh_iterate_batch), or the first iterate() of a solver for itself.  Every later iterate() answers from the cache on the host.
// Differences from the reference, next to the unpinned steps of include/orbh.h: rand() is consumed per solver for the whole range at Prefetch, not
// interleaved five at a time across the candidates (UseSets fixes the sets instead); with fewer than three correspondences iterate returns an empty
// matrix and bNoMore where the source's draw would read past its index vector.
// There is no CPU fallback: without a usable GPU a fetch throws std::runtime_error.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbh.h"

namespace ORB_SLAM {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

    cv::Mat find(std::vector<bool>& vbInliers12, int& nInliers);

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

    cv::Mat GetEstimatedRotation();
    cv::Mat GetEstimatedTranslation();
    float GetEstimatedScale();

    // For every listed non-NULL solver: draws the sets of all its remaining iterations up to mRansacMaxIts and computes their hypotheses, all solvers
    // in one batched chain with one synchronisation (ORBH_MAX_PROBLEMS solvers and ORBH_MAX_ITERS iterations per chain; more take further chains).
    // The whole chain runs on the device of the first listed solver that takes part.  If it fails std::runtime_error is thrown and no cache changes.
    // LoopClosing::ComputeSim3: one line in front of its while loop, Sim3Solver::Prefetch(vpSim3Solvers).
    static void Prefetch(const std::vector<Sim3Solver*>& vpSolvers);

    // The sets of the next iterations instead of a draw (3 indices into the correspondences each, consumed in order): reproducible runs and tests.
    void UseSets(const std::vector<int32_t>& sets) { mGivenSets = sets; mGivenUsed = 0; }
    void SetDevice(int device) { mDevice = device; }

    // What the last iterate saw, for logs and tests.
    struct Report {
        int found;                       // a similarity was returned
        int walked;                      // iterations walked by the call
        int iterations, bestInliers;     // mnIterations, mnBestInliers after the call
        int deviceCalls;                 // device calls the call itself made (0: answered from the cache)
        int cached;                      // iterations computed so far
    };
    const Report& LastReport() const { return mReport; }
    int Correspondences() const { return N; }
    int MaxIterations() const { return mRansacMaxIts; }

private:
    bool WantsFetch() const;                                      // iterations are left that are not in the cache
    int PrepareFetch(orbh_problem& q, std::vector<int32_t>& sets);     // draws the sets of the next chunk; -> its length
    void TakeFetch(int count, const std::vector<orbh_hyp>& hyp, const std::vector<uint64_t>& flags);
    void FetchAlone();

    int mN1, N;
    std::vector<float> mX3Dc1, mX3Dc2, mP1im1, mP2im2, mMaxError1, mMaxError2;
    std::vector<std::size_t> mvnIndices1;
    float mK1[4], mK2[4];                                         // fx, fy, cx, cy
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;
    // the state of iterate()
    int mnIterations, mnBestInliers;
    std::vector<uint64_t> mBestFlags;
    float mBestT12[16], mBestR[9], mBestt[3], mBestScale;
    // the hypotheses of the iterations [0, mCached): counts and transforms, flag words
    int mCached;
    std::vector<orbh_hyp> mHyp;
    std::vector<uint64_t> mFlags;
    std::vector<int32_t> mGivenSets;
    std::size_t mGivenUsed;
    int mDevice;
    Report mReport;
};

}  // namespace ORB_SLAM
