// ORB_SLAM::Initializer — the reference's monocular initialisation (include/Initializer.h, src/Initializer.cc) with its arithmetic on the MI355X
// (include/orbi.h): the reference's constructor and Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated).  Host C++ written against
// the reference's Frame member names (mK, mvKeysUn); links the C ABI only (swap Initializer.h + .cc).
//   host:    the match list, the RANSAC sets (the reference's DUtils::Random::RandomInt expression over rand()), Normalize twice (orbi_normalize),
//            RH = SH/(SH+SF) and the 0.40 rule, DecomposeE / the Faugeras decomposition in double (the Jacobi header of the kernels, compiled for the
//            host), the acceptance rules of src/Initializer.cc:497-567 and :719-729;
//   device:  one orbi_models call (every homography and fundamental matrix fitted and scored, the winners selected), then one orbi_check_rt call for
//            the 4 or 8 motion hypotheses.  Two synchronisations per Initialize: the host has to see the scores before it knows which model to
//            decompose.
// Deviations, next to those of include/orbi.h: the matrices are not OpenCV's to the last bit, and the decompositions are evaluated in double from the
// float winner and rounded once, so R21 / t21 may differ from an OpenCV build in their last bits; fewer than 8 matches, or no hypothesis with a
// positive score, return false (the reference would draw from an empty list, or decompose an empty matrix).
// There is no CPU fallback: without a usable GPU the call throws std::runtime_error.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "Frame.h"

namespace ORB_SLAM {

class Initializer {
    typedef std::pair<int, int> Match;

public:
    // Fix the reference frame
    Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200);

    // Fits a fundamental matrix and a homography, selects a model and tries to recover the motion and the structure from motion
    bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                    std::vector<bool>& vbTriangulated);

    // The sets of the next Initialize calls instead of a draw (iterations x 8 indices into the match list): reproducible runs and tests.
    void UseSets(const std::vector<std::vector<std::size_t> >& sets) { mvGivenSets = sets; }
    void SetDevice(int device) { mDevice = device; }

    // What the last Initialize saw, for logs and tests.
    struct Report {
        char model;                      // 'H', 'F', or 0 when no hypothesis scored
        float SH, SF, RH;
        int bestH, bestF, nInliers;
        std::vector<int> nGood;          // per motion hypothesis, in the reference's order
        std::vector<float> parallax;
        int chosen;                      // the hypothesis returned, -1 when none
    };
    const Report& LastReport() const { return mReport; }
    const std::vector<std::vector<std::size_t> >& Sets() const { return mvSets; }

private:
    bool Reconstruct(bool homography, const float* M, const unsigned char* inliers, cv::Mat& R21, cv::Mat& t21, std::vector<cv::Point3f>& vP3D,
                     std::vector<bool>& vbTriangulated, float minParallax, int minTriangulated);

    std::vector<cv::KeyPoint> mvKeys1, mvKeys2;
    std::vector<Match> mvMatches12;
    std::vector<int> mMatchesFlat;                // mvMatches12 as the int32 [N][2] the C ABI reads
    std::vector<bool> mvbMatched1;
    cv::Mat mK;
    float mSigma, mSigma2;
    int mMaxIterations;
    std::vector<std::vector<std::size_t> > mvSets, mvGivenSets;
    int mDevice;
    Report mReport;
};

}  // namespace ORB_SLAM
