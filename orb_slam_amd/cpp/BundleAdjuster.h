// ORB_SLAM::BundleAdjuster — the reference's Optimizer::LocalBundleAdjustment (src/Optimizer.cc:287-536), Optimizer::BundleAdjustment (:46-151) and
// Optimizer::GlobalBundleAdjustemnt (:38-43) with their arithmetic on the MI355X (include/orbb.h): g2o's optimize(n) with Levenberg over the Schur
// complement.  Host C++ written against the reference's member names; links the C ABI only, so a build that binds this class needs neither Eigen
// nor g2o for its bundle adjustments (swap the two Optimizer calls).
//   host:    the walk of :289-338 that makes lLocalKeyFrames, lLocalMapPoints and lFixedCameras with the mnBALocalForKF / mnBAFixedForKF marks, in the
//            reference's order; the point-major edges over GetObservations() of non-bad key frames (:399-447); the two loops over the flags
//            (:453-470, :497-515) with EraseMapPointMatch and EraseObservation; SetPose, SetWorldPos and UpdateNormalAndDepth.
//   device:  LocalBundleAdjustment makes TWO calls on one state, optimize(5) and optimize(10), because the reference needs the host in between:
//            a point that EraseObservation makes bad inside the first loop keeps its later flagged edges ACTIVE (`if(pMP->isBad()) continue`).
//            BundleAdjustment makes one call of nIterations.
// A key frame with mnId == 0 is a fixed vertex (:363, :72): it goes behind the free poses with the fixed cameras.
// Differences from the reference:
//   * the device call cannot be interrupted: *pbStopFlag is read before each optimize(); a raised flag makes that call run 0 iterations, which is
//     what g2o's loop does when terminate() is already true;
//   * the intermediate write-back of :472-489 is overwritten by :517-535 and is left out;
//   * the two steps include/orbb.h does not pin to Eigen (the 3 x 3 inverse, the dense LDL' in place of the sparse LLT);
//   * nIterations above ORBB_MAX_ITERS runs as several calls on the same state, each of which restarts lambda as a new optimize() does.
// There is no CPU fallback: without a usable GPU, or with more than ORBB_MAX_FREE free key frames, the calls throw std::runtime_error.
#pragma once
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbb.h"

namespace ORB_SLAM {

class Map;

class BundleAdjuster {
public:
    static void LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag = NULL);
    static void BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations = 5, bool* pbStopFlag = NULL);
    // Map::GetAllKeyFrames and GetAllMapPoints, forwarded (a template so that this header needs no Map.h)
    template <class MapT> static void GlobalBundleAdjustemnt(MapT* pMap, int nIterations = 5, bool* pbStopFlag = NULL) {
        BundleAdjustment(pMap->GetAllKeyFrames(), pMap->GetAllMapPoints(), nIterations, pbStopFlag);
    }

    static void SetDevice(int device) { mnDevice = device; }

    // what the last call did (for tests and logs)
    struct Report {
        std::vector<KeyFrame*> vLocalKeyFrames, vFixedCameras;
        std::vector<MapPoint*> vLocalMapPoints;
        int nFree = 0, nFixed = 0, nEdges = 0, deviceCalls = 0;
        int iters[2] = {0, 0}, erased[2] = {0, 0};
    };
    static const Report& LastReport() { return mReport; }

private:
    static int mnDevice;
    static Report mReport;
};

}  // namespace ORB_SLAM
