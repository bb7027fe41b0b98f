// ORB_SLAM::PoseOptimizer — the reference's Optimizer::PoseOptimization (include/Optimizer.h, src/Optimizer.cc:154-285) with its arithmetic on the
// MI355X (include/orbo.h): the Levenberg iteration of g2o over one SE3 vertex, four rounds, in one launch.  Host C++ written against the
// reference's member names (Frame::mvpMapPoints, mvKeysUn, mvbOutlier, mTcw, fx, fy, cx, cy, mvLevelSigma2; MapPoint::GetWorldPos); links the C ABI
// only: a build that tracks and relocalises through this class needs neither Eigen nor g2o (add PoseOptimizer.h + .cc).
//   host:    the walk over mvpMapPoints that makes the compact edges (:191-237; vnIndexEdge stays here), mvbOutlier by key point, mTcw;
//   device:  one orbo_pose call per frame, or ONE orbo_pose_batch for a list of frames (the relocaliser's candidates), one synchronisation.
// invSigma2 is 1/mvLevelSigma2[octave] in float, which is what Frame.cc:107 stores in mvInvLevelSigma2.
// Differences from the reference: the two steps include/orbo.h does not pin to Eigen (Quaterniond(R), the dense LDLT).
// There is no CPU fallback: without a usable GPU PoseOptimization throws std::runtime_error.
#pragma once
#include <vector>

#include "Frame.h"
#include "MapPoint.h"
#include "orbo.h"

namespace ORB_SLAM {

class PoseOptimizer {
public:
    // Optimizer::PoseOptimization: sets pFrame->mvbOutlier for every key point with a map point, stores the pose in pFrame->mTcw and returns
    // nInitialCorrespondences - nBad
    static int PoseOptimization(Frame* pFrame);

    // the same for every listed non-NULL frame as one batched call; pnGood (may be NULL) receives one return value per entry, -1 for a NULL entry.
    // More than ORBO_MAX_PROBLEMS frames run as several calls.
    static void PoseOptimization(const std::vector<Frame*>& vpFrames, std::vector<int>* pnGood);

    static void SetDevice(int device) { mnDevice = device; }

    // what the last call made of its first frame (for tests and logs)
    struct Report {
        int nInitial = 0, nBad = 0, rounds = 0, iters[ORBO_ROUNDS] = {0, 0, 0, 0}, deviceCalls = 0;
    };
    static const Report& LastReport() { return mReport; }

private:
    static int mnDevice;
    static Report mReport;
};

}  // namespace ORB_SLAM
