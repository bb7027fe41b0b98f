// Stand-in ORB_SLAM::Frame: the members of the reference's include/Frame.h that Initializer.cc reads, over the stand-in OpenCV types of
// tests/mappoints_dropin/cvmini.h plus cv::Point3f.
#pragma once
#include <vector>

#include "cvmini.h"

namespace cv {
struct Point3f {
    float x, y, z;
    Point3f() : x(0), y(0), z(0) {}
    Point3f(float a, float b, float c) : x(a), y(b), z(c) {}
};
}  // namespace cv

namespace ORB_SLAM {

class Frame {
public:
    cv::Mat mK = cv::Mat(3, 3, CV_32F);          // calibration matrix
    std::vector<cv::KeyPoint> mvKeysUn;          // undistorted key points
};

}  // namespace ORB_SLAM
