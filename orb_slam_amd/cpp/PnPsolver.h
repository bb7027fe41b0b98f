// ORB_SLAM::PnPsolver — the reference's relocalisation solver (include/PnPsolver.h:61-72, src/PnPsolver.cc) with its arithmetic on the MI355X
// (include/orbe.h): the reference's constructor, SetRansacParameters, find and iterate.  Host C++ written against the reference's member names
// (Frame::mvKeysUn, mvLevelSigma2, fx, fy, cx, cy; MapPoint::isBad, GetWorldPos); links the C ABI only (swap PnPsolver.h + .cc).
//   host:    the correspondences (:68-111), SetRansacParameters (orbe_ransac_parameters), the draw of the sets with the reference's
//            DUtils::Random::RandomInt expression over rand() and its `vAvailableIndices[idx] = vAvailableIndices.back()` (idx, not randi; the write is
//            made only where idx < size(), which is what every later read of the source sees), vbInliers by key point;
//   device:  one orbe_iterate call per iterate(): every hypothesis of the range [mnIterations, max(mRansacMaxIts, mnIterations + nIterations)), Refine
//            of the records and the walk, one synchronisation.  Prefetch runs the next iterate() of several solvers as ONE chain.
// Differences from the reference, next to the deviation of include/orbe.h (the four-point poses are the reference's in distribution, not iteration
// by iteration): rand() is consumed for the whole range of a call even when the call returns early; UseSets fixes the sets instead.
// N < mRansacMinInliers returns an empty matrix and bNoMore without a device call, as the source does.
// There is no CPU fallback: without a usable GPU iterate throws std::runtime_error.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "Frame.h"
#include "MapPoint.h"
#include "orbe.h"

namespace ORB_SLAM {

class PnPsolver {
public:
    PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches);

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991);

    cv::Mat find(std::vector<bool>& vbInliers, int& nInliers);

    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

    // Runs the next iterate(nIterations) of every listed non-NULL solver in one batched chain with one synchronisation; each solver's next
    // iterate with that nIterations answers from the cached block (with another nIterations the cache is dropped and the call runs as usual).
    // A dropped cache restores the solver's state, flags and position in the UseSets list, not the rand() values the prefetched draw consumed: without
    // UseSets the later call draws other sets than it would have without the Prefetch.  The whole chain runs on the device of the first listed
    // solver that takes part; the other solvers' SetDevice is not looked at.  If the chain fails the solvers are put back in the same way and
    // std::runtime_error is thrown.
    // Tracking::Relocalisation: one line at the top of its while loop, PnPsolver::Prefetch(vpPnPsolvers, 5), NULL-ing discarded solvers as it does.
    static void Prefetch(const std::vector<PnPsolver*>& vpSolvers, int nIterations);

    // The sets of the next iterations instead of a draw (4 indices into the correspondences each, consumed in order): reproducible runs and tests.
    void UseSets(const std::vector<int32_t>& sets) { mGivenSets = sets; mGivenUsed = 0; }
    void SetDevice(int device) { mDevice = device; }

    // What the last iterate saw, for logs and tests.
    struct Report {
        int kind;                        // ORBE_KIND_*
        int stop, range;                 // the iteration of the range at which the call returned; the length of the range
        int iterations, bestInliers;     // mnIterations, mnBestInliers after the call
        bool prefetched;                 // answered from a Prefetch
    };
    const Report& LastReport() const { return mReport; }
    int Correspondences() const { return N; }

private:
    struct Call {                        // one prepared or finished call
        orbe_problem q;
        std::vector<int32_t> sets;
        orbe_result result;
        std::vector<uint8_t> flags;
    };
    bool Prepare(int nIterations, Call& c);                       // false: N < mRansacMinInliers
    cv::Mat Finish(const Call& c, bool prefetched, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

    std::size_t mnKeys;
    std::vector<float> mP3D, mP2D, mvSigma2, mvMaxError;
    std::vector<std::size_t> mvKeyPointIndices;
    float fu, fv, uc, vc;
    int N, mRansacMinInliers, mRansacMaxIts;
    float mRansacEpsilon;
    orbe_state mState;
    std::vector<uint8_t> mBestFlags, mRefinedFlags;
    std::vector<int32_t> mGivenSets;
    std::size_t mGivenUsed;
    int mDevice;
    Report mReport;
    // a Prefetch not yet consumed: its call, and the solver as it was before
    bool mPending;
    int mPendingIterations;
    Call mPendingCall;
    orbe_state mStateBefore;
    std::vector<uint8_t> mBestBefore, mRefinedBefore;
    std::size_t mGivenBefore;
};

}  // namespace ORB_SLAM
