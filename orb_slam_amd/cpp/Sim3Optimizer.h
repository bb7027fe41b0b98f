// ORB_SLAM::Sim3Optimizer — the reference's Optimizer::OptimizeSim3 (include/Optimizer.h, src/Optimizer.cc:789-987) with its arithmetic on the
// MI355X (include/orbg.h): the Levenberg iteration of g2o over one Sim3 vertex with its numeric Jacobian, both phases and both inlier checks in one
// launch.  Host C++ written against the reference's member names (KeyFrame::GetCalibrationMatrix, GetRotation, GetTranslation, GetMapPointMatches,
// GetKeyPointUn, GetInvSigma2, GetSigma2; MapPoint::GetWorldPos, GetIndexInKeyFrame, isBad); links the C ABI only: a build that closes loops through
// this class needs neither Eigen nor g2o (add Sim3Optimizer.h + .cc).
//   host:    the walk of :844-923 that makes the compact pairs (the isBad and GetIndexInKeyFrame tests, vnIndexEdge, R1w*P3D1w + t1w in float as a
//            cv::Mat product accumulates it, both sigma calls as they are: GetInvSigma2 on side 1, GetSigma2 on side 2), then
//            vpMatches1[idx] = NULL from the flags;
//   device:  one orbg_sim3 call per candidate, or ONE orbg_sim3_batch for a list of candidates, one synchronisation.
// Sim3State is the g2o::Sim3 of the call without Eigen: {q (x y z w), t, s} in double.  The header-only template reads and writes a g2o::Sim3 (or
// anything with its accessors) only through rotation(), translation() and scale(), so the call at src/LoopClosing.cc:321 changes in the class name
// alone:   const int nInliers = Sim3Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10);
// On the early `return 0` (:957-958) g2oS12 stays as it was and the matches the first check cleared stay cleared, as in the reference.
// Differences from the reference: the two steps include/orbg.h does not pin to Eigen (Quaterniond(R), the dense LDLT).
// There is no CPU fallback: without a usable GPU OptimizeSim3 throws std::runtime_error.
#pragma once
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbg.h"

namespace ORB_SLAM {

// g2o::Sim3 as plain numbers
struct Sim3State {
    double q[4], t[3], s;                                              // x y z w
    // The C ABI starts from the FLOAT R, t, s of LoopClosing.cc:320 and takes Quaterniond(R) itself.  A state built by the constructor below
    // keeps those floats (start) and is passed on exactly; one that only has q, t, s (the template overload, Compose) is narrowed:
    // toRotationMatrix(q), t and s to float, which moves the start by a float ulp, not the optimum.
    float start[13];
    bool hasStart;
    Sim3State() : q{0, 0, 0, 1}, t{0, 0, 0}, s(1), start{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, hasStart(false) {}
    // g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) (LoopClosing.cc:320, sim3.h:64-67): Quaterniond(R) of the float R widened, in
    // include/orbo.h's branch form, not normalised
    Sim3State(const cv::Mat& R, const cv::Mat& t, float s);
};

class Sim3Optimizer {
public:
    // Optimizer::OptimizeSim3: clears the rejected entries of vpMatches1, stores the refined similarity in S12 (unless the early return is taken)
    // and returns nIn
    static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, Sim3State& S12, float th2 = 10);

    // the same signature as the reference's over a g2o::Sim3, through its accessors only
    template <class Sim3T>
    static int OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, Sim3T& g2oS12, float th2 = 10) {
        Sim3State S;
        S.q[0] = g2oS12.rotation().x(); S.q[1] = g2oS12.rotation().y(); S.q[2] = g2oS12.rotation().z(); S.q[3] = g2oS12.rotation().w();
        for (int i = 0; i < 3; i++) S.t[i] = g2oS12.translation()[i];
        S.s = g2oS12.scale();
        const int nIn = OptimizeSim3(pKF1, pKF2, vpMatches1, S, th2);
        g2oS12.rotation().x() = S.q[0]; g2oS12.rotation().y() = S.q[1]; g2oS12.rotation().z() = S.q[2]; g2oS12.rotation().w() = S.q[3];
        for (int i = 0; i < 3; i++) g2oS12.translation()[i] = S.t[i];
        g2oS12.scale() = S.s;
        return nIn;
    }

    // one loop candidate of the batched form (LocalMapPoints::SearchBySim3's Sim3Candidate): the other key frame, its matches, its similarity
    struct Candidate {
        KeyFrame* pKF2;
        std::vector<MapPoint*>* vpMatches1;
        Sim3State* S12;
        float th2;
        Candidate(KeyFrame* kf, std::vector<MapPoint*>* m, Sim3State* s, float th = 10) : pKF2(kf), vpMatches1(m), S12(s), th2(th) {}
    };
    // every candidate of pKF1 as ONE orbg_sim3_batch; vnInliers (may be NULL) receives one return value per candidate.  More than
    // ORBG_MAX_PROBLEMS candidates run as several calls.
    static void OptimizeSim3(KeyFrame* pKF1, const std::vector<Candidate>& vCandidates, std::vector<int>* vnInliers);

    static cv::Mat ToCvMat(const Sim3State& S);                        // Converter::toCvMat(g2o::Sim3) (Converter.cc:56-62)
    // gScm * g2o::Sim3(Rmw, tmw, 1.0) with pKFm's pose (LoopClosing.cc:328-329, sim3.h:266-272)
    static Sim3State Compose(const Sim3State& Scm, KeyFrame* pKFm);

    static void SetDevice(int device) { mnDevice = device; }

    // what the last call made of its first candidate (for tests and logs)
    struct Report {
        int nCorrespondences = 0, nBad = 0, nIn = 0, ret0 = 0, iters[2] = {0, 0}, deviceCalls = 0;
    };
    static const Report& LastReport() { return mReport; }

private:
    static int mnDevice;
    static Report mReport;
};

}  // namespace ORB_SLAM
