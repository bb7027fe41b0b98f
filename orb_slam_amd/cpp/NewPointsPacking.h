// What LocalMapPoints::CreateNewMapPoints (LocalMapPointsNewPoints.cc) uploads per call, as plain functions: the "holds a map point" flags of a key
// frame's feature slots in the two polarities ORBmatcher::SearchForTriangulation reads them (reference src/ORBmatcher.cc:892-896, :908-912: the
// POINTER is tested, a bad point counts), and a fundamental matrix as nine floats.  No HIP, no OpenCV: tests/_probe/tri_rows_host.cpp runs it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ORB_SLAM {

// flag[i] = 1 when (v[i] != NULL) == holds, for i < min(v.size(), cap); the rest of the cap entries 0
template <class Point>
inline void PackPointFlags(const std::vector<Point*>& v, bool holds, int cap, uint8_t* flag) {
    for (int i = 0; i < cap; i++) flag[i] = (std::size_t)i < v.size() && ((v[i] != 0) == holds) ? 1 : 0;
}

// F12 (3 x 3, CV_32F) row major, `F12.at<float>(r, c)` at out[3r + c]; false for a matrix that is empty or not 3 x 3 (nothing is written)
template <class Mat>
inline bool PackF12(const Mat& F12, float* out) {
    if (F12.empty() || F12.rows != 3 || F12.cols != 3) return false;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) out[3 * r + c] = F12.template at<float>(r, c);
    return true;
}

}  // namespace ORB_SLAM
