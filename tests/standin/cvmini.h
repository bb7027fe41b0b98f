// The little of OpenCV that ORB_SLAM's Frame.h / KeyFrame.h / MapPoint.h expose to the drop-in classes of orb_slam_amd/cpp, for the stand-in
// headers of this directory: a matrix of floats or bytes with at<T>() / ptr<T>(), cv::KeyPoint and cv::Point3f.  A copy of a Mat shares its
// store, as OpenCV's does.
// tests/kfdb_dropin keeps its own Frame.h / KeyFrame.h: they sit on orb_slam_amd/cpp/cvcompat.h, whose cv::Mat is another type than this one.
#pragma once
#include <cstddef>
#include <memory>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

struct Point2f { float x = 0, y = 0; };

struct Point3f {
    float x, y, z;
    Point3f() : x(0), y(0), z(0) {}
    Point3f(float a, float b, float c) : x(a), y(b), z(c) {}
};

struct KeyPoint {
    Point2f pt;
    float size = 0, angle = -1, response = 0;
    int octave = 0, class_id = -1;
};

class Mat {
public:
    int rows = 0, cols = 0;
    Mat() {}
    Mat(int r, int c, int type) : rows(r), cols(c), esz_(type == CV_32F ? 4 : 1), store_(std::make_shared<std::vector<unsigned char> >((std::size_t)r * c * (type == CV_32F ? 4 : 1))) {}
    template <typename T> T& at(int i) { return reinterpret_cast<T*>(store_->data())[i]; }
    template <typename T> const T& at(int i) const { return reinterpret_cast<const T*>(store_->data())[i]; }
    template <typename T> T& at(int r, int c) { return reinterpret_cast<T*>(store_->data())[(std::size_t)r * cols + c]; }
    template <typename T> const T& at(int r, int c) const { return reinterpret_cast<const T*>(store_->data())[(std::size_t)r * cols + c]; }
    template <typename T> T* ptr(int r = 0) { return reinterpret_cast<T*>(store_->data() + (std::size_t)r * cols * esz_); }
    template <typename T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(store_->data() + (std::size_t)r * cols * esz_); }
    Mat clone() const { Mat m(*this); m.store_ = std::make_shared<std::vector<unsigned char> >(*store_); return m; }
    bool empty() const { return !store_ || rows == 0 || cols == 0; }

private:
    int esz_ = 1;
    std::shared_ptr<std::vector<unsigned char> > store_;
};

}  // namespace cv
