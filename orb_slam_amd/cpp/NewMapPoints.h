// ORB_SLAM::TriangulateNewMapPoints — the match loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:269-353) as one
// call on the MI355X (include/orbt.h): the parallax test, the linear triangulation and the six tests in front of `new MapPoint(x3D, ...)`
// for every match ORBmatcher::SearchForTriangulation returned.  Host C++ written against the reference's KeyFrame member names; links
// the C ABI only.  The host keeps `new MapPoint`, AddObservation, AddMapPoint and what follows (:355-368).
// The null vector of the 4 x 4 system is computed in double precision, not by OpenCV's float cv::SVD: include/orbt.h, "THE ONE DEVIATION".
// There is no CPU fallback: without a usable GPU the call throws std::runtime_error.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "KeyFrame.h"

namespace ORB_SLAM {

class KeyFrame;

// one match for which the reference reaches `new MapPoint(x3D, mpCurrentKeyFrame, mpMap)`
struct NewMapPoint {
    cv::Mat x3D;                    // 3 x 1, CV_32F
    std::size_t idx1, idx2;         // vMatchedIndices[ikp]
};

// pKF1 = mpCurrentKeyFrame, pKF2 = the neighbour; the three vectors are what SearchForTriangulation filled.  Returns the accepted matches
// in the order of vMatchedIndices.  status (may be NULL) receives one ORBT_* value per match.
std::vector<NewMapPoint> TriangulateNewMapPoints(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<cv::KeyPoint>& vMatchedKeysUn1,
                                                 const std::vector<cv::KeyPoint>& vMatchedKeysUn2,
                                                 const std::vector<std::pair<std::size_t, std::size_t> >& vMatchedIndices,
                                                 std::vector<unsigned char>* status = 0, int device = 0);

}  // namespace ORB_SLAM
