// ORB_SLAM::ORBextractor with the reference's class surface (reference include/ORBextractor.h:31-79),
// implemented on the MI355X C ABI (include/orbx.h).  Frame / Tracking call it unchanged:
//     (*mpORBextractor)(im, cv::Mat(), mvKeys, mDescriptors);          // reference src/Frame.cc:60
// Differences from the reference, all documented in INTEGRATION.md:
//   * device errors throw std::runtime_error (the reference cannot fail there);
//   * the mask argument is accepted and ignored — it has no effect in the reference either
//     (cellMask is built but never passed to cv::FAST, reference src/ORBextractor.cc:601-607).
#pragma once
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvcompat.h"
#include "orbx.h"

namespace ORB_SLAM {

class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    // maxBatch: frames per launch group of ExtractBatch (operator() is unaffected)
    ORBextractor(int nfeatures = 1000, float scaleFactor = 1.2f, int nlevels = 8, int scoreType = FAST_SCORE, int fastTh = 20,
                 int device = 0, int maxBatch = 1)
        : h_(nullptr), nlevels_(nlevels), scaleFactor_(scaleFactor), device_(device) {
        orbx_params p;
        orbx_default_params(&p);
        p.nfeatures = nfeatures; p.scale_factor = scaleFactor; p.nlevels = nlevels; p.score_type = scoreType; p.fast_th = fastTh;
        p.device = device;
        p.max_batch = maxBatch;
        const int rc = orbx_create(&p, &h_);
        if (rc != ORBX_OK) throw std::runtime_error("orbx_create failed (" + std::to_string(rc) + "): no usable MI355X / HIP runtime");
        cap_ = orbx_max_keypoints(h_);
    }
    ~ORBextractor() {
        freeBatch();
        orbx_destroy(h_);
    }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // Compute the ORB features and descriptors on an image (reference include/ORBextractor.h:43-45).  Written against the proxy
    // classes the way the reference's own body is (src/ORBextractor.cc:718-742: _image.empty(), _image.getMat(),
    // _descriptors.release() / create() / getMat()), so it compiles against a real OpenCV 2.4 (-DORBX_WITH_OPENCV) as well as
    // against cvcompat.h.
    void operator()(cv::InputArray _image, cv::InputArray /*_mask*/, std::vector<cv::KeyPoint>& _keypoints, cv::OutputArray _descriptors) {
        if (_image.empty()) return;                                  // reference :721-722: outputs untouched
        cv::Mat image = _image.getMat();
        kps_.resize(cap_);
        desc_.resize((size_t)cap_ * 32);
        int n = 0;
        const int rc = orbx_extract(h_, image.data, image.cols, image.rows, (ptrdiff_t)image.step,
                                    reinterpret_cast<orbx_keypoint*>(kps_.data()), desc_.data(), cap_, &n);
        if (rc == ORBX_EMPTY) return;
        if (rc != ORBX_OK) throw std::runtime_error(std::string("orbx_extract: ") + orbx_last_error(h_));
        if (n == 0) _descriptors.release();                           // reference :738-739
        else {
            _descriptors.create(n, 32, CV_8U);                        // reference :742
            cv::Mat descriptors = _descriptors.getMat();
            for (int i = 0; i < n; i++) std::memcpy(descriptors.ptr(i), desc_.data() + (size_t)i * 32, 32);
        }
        _keypoints.assign(kps_.begin(), kps_.begin() + n);            // reference :746-747,:777
    }

    // Tracking::GrabImage + the extraction of Frame::Frame in one call (reference src/Tracking.cc:185-195, src/Frame.cc:57-60): a colour
    // image (CV_8UC3 / CV_8UC4; rgb = Camera.RGB, true for R, G, B byte order, false for B, G, R) is converted to gray on the GPU
    // (cvtColor CV_RGB2GRAY / CV_BGR2GRAY; a fourth channel is ignored), a gray one (CV_8UC1) is copied, as GrabImage does.  imGray
    // receives the gray image (what Frame keeps as Frame::im); keypoints / descriptors are what operator() gives for imGray
    // (orbx_extract_color).
    void GrabImage(const cv::Mat& im, bool rgb, cv::Mat& imGray, std::vector<cv::KeyPoint>& keypoints, cv::Mat& descriptors) {
        if (im.empty()) return;                                      // reference :721-722: outputs untouched
        const int fmt = pixFormat(channelsOf(im), rgb);
        cv::Mat gray(im.rows, im.cols, CV_8UC1);
        kps_.resize(cap_);
        desc_.resize((size_t)cap_ * 32);
        int n = 0;
        const int rc = orbx_extract_color(h_, im.data, im.cols, im.rows, (ptrdiff_t)im.step, fmt, reinterpret_cast<orbx_keypoint*>(kps_.data()),
                                          desc_.data(), cap_, &n, gray.data);
        if (rc == ORBX_EMPTY) return;
        if (rc != ORBX_OK) throw std::runtime_error(std::string("orbx_extract_color: ") + orbx_last_error(h_));
        imGray = gray;
        if (n == 0) descriptors.release();                           // reference :738-739
        else {
            descriptors.create(n, 32, CV_8U);
            for (int i = 0; i < n; i++) std::memcpy(descriptors.ptr(i), desc_.data() + (size_t)i * 32, 32);
        }
        keypoints.assign(kps_.begin(), kps_.begin() + n);
    }

    // Several host images of one size, any step each, in one call (orbx_extract_batch, host form: launch groups of maxBatch frames, the
    // upload of one overlapping the kernels of the previous one).  keypoints[i] / descriptors[i] are exactly what operator() gives for
    // images[i], descriptors[i] released when it has no features.
    void ExtractBatch(const std::vector<cv::Mat>& images, std::vector<std::vector<cv::KeyPoint> >& keypoints, std::vector<cv::Mat>& descriptors) {
        extractBatch(images, ORBX_PIX_GRAY8, keypoints, descriptors);
    }
    // The same for colour images (all CV_8UC3 or all CV_8UC4; rgb as in GrabImage), converted to gray on the GPU per launch group
    // (orbx_extract_batch_color): keypoints[i] / descriptors[i] are what GrabImage gives for images[i].
    void ExtractBatch(const std::vector<cv::Mat>& images, bool rgb, std::vector<std::vector<cv::KeyPoint> >& keypoints, std::vector<cv::Mat>& descriptors) {
        const int fmt = images.empty() ? ORBX_PIX_GRAY8 : pixFormat(channelsOf(images[0]), rgb);
        for (const cv::Mat& m : images)
            if (pixFormat(channelsOf(m), rgb) != fmt) throw std::invalid_argument("ExtractBatch: images differ in channels");
        extractBatch(images, fmt, keypoints, descriptors);
    }

    int inline GetLevels() { return nlevels_; }
    float inline GetScaleFactor() { return (float)scaleFactor_; }

private:
    // CV_MAT_CN of the matrix type (read from type(): the stand-in matrices some builds of this header see have no channels())
    static int channelsOf(const cv::Mat& m) { return ((m.type() >> 3) & 511) + 1; }
    static int pixFormat(int channels, bool rgb) {
        switch (channels) {
            case 1: return ORBX_PIX_GRAY8;
            case 3: return rgb ? ORBX_PIX_RGB8 : ORBX_PIX_BGR8;
            case 4: return rgb ? ORBX_PIX_RGBA8 : ORBX_PIX_BGRA8;
            default: throw std::invalid_argument("ORBextractor: images must have 1, 3 or 4 channels");
        }
    }

    void extractBatch(const std::vector<cv::Mat>& images, int fmt, std::vector<std::vector<cv::KeyPoint> >& keypoints, std::vector<cv::Mat>& descriptors) {
        const int F = (int)images.size();
        keypoints.assign(F, std::vector<cv::KeyPoint>());
        descriptors.resize(F);
        if (F == 0) return;
        const int w = images[0].cols, hgt = images[0].rows;
        std::vector<const uint8_t*> ptrs(F);
        std::vector<ptrdiff_t> steps(F);
        for (int i = 0; i < F; i++) {
            if (images[i].cols != w || images[i].rows != hgt) throw std::invalid_argument("ExtractBatch: images differ in size");
            ptrs[i] = images[i].data;
            steps[i] = (ptrdiff_t)images[i].step;
        }
        if (w <= 0 || hgt <= 0) return;                               // reference :721-722: outputs untouched
        if (F > batchCap_) {
            freeBatch();
            if (orbx_device_alloc(device_, (size_t)F * cap_ * sizeof(orbx_keypoint), &dKps_) != ORBX_OK ||
                orbx_device_alloc(device_, (size_t)F * cap_ * 32, &dDesc_) != ORBX_OK || orbx_device_alloc(device_, (size_t)F * 8, &dN_) != ORBX_OK)
                throw std::runtime_error("ExtractBatch: device allocation failed");
            batchCap_ = F;
        }
        int32_t* dn = static_cast<int32_t*>(dN_);
        const int rc = fmt == ORBX_PIX_GRAY8
            ? orbx_extract_batch(h_, ptrs.data(), steps.data(), F, w, hgt, ORBX_FRAMES_ON_HOST, static_cast<orbx_keypoint*>(dKps_),
                                 static_cast<uint8_t*>(dDesc_), dn, cap_, dn + F, nullptr)
            : orbx_extract_batch_color(h_, ptrs.data(), steps.data(), F, w, hgt, ORBX_FRAMES_ON_HOST, fmt, static_cast<orbx_keypoint*>(dKps_),
                                       static_cast<uint8_t*>(dDesc_), dn, cap_, dn + F, nullptr);
        if (rc == ORBX_EMPTY) return;
        if (rc != ORBX_OK) throw std::runtime_error(std::string(fmt == ORBX_PIX_GRAY8 ? "orbx_extract_batch: " : "orbx_extract_batch_color: ") + orbx_last_error(h_));
        std::vector<int32_t> ns((size_t)2 * F);
        kps_.resize((size_t)F * cap_);
        desc_.resize((size_t)F * cap_ * 32);
        if (orbx_device_download(device_, ns.data(), dN_, ns.size() * 4) != ORBX_OK ||
            orbx_device_download(device_, kps_.data(), dKps_, kps_.size() * sizeof(orbx_keypoint)) != ORBX_OK ||
            orbx_device_download(device_, desc_.data(), dDesc_, desc_.size()) != ORBX_OK)
            throw std::runtime_error("ExtractBatch: device download failed");
        for (int i = 0; i < F; i++) {
            if (ns[F + i] != ORBX_OK) throw std::runtime_error("ExtractBatch: internal list capacity exceeded");
            const int n = ns[i];
            if (n == 0) descriptors[i].release();                     // reference :738-739
            else {
                descriptors[i].create(n, 32, CV_8U);
                for (int k = 0; k < n; k++) std::memcpy(descriptors[i].ptr(k), desc_.data() + ((size_t)i * cap_ + k) * 32, 32);
            }
            keypoints[i].assign(kps_.begin() + (size_t)i * cap_, kps_.begin() + (size_t)i * cap_ + n);
        }
    }

    void freeBatch() {
        orbx_device_free(device_, dKps_);
        orbx_device_free(device_, dDesc_);
        orbx_device_free(device_, dN_);
        dKps_ = dDesc_ = dN_ = nullptr;
        batchCap_ = 0;
    }

    orbx_extractor* h_;
    int nlevels_;
    double scaleFactor_;   // the reference keeps a double member initialised from the float argument
    int device_;
    int cap_;
    void *dKps_ = nullptr, *dDesc_ = nullptr, *dN_ = nullptr;     // ExtractBatch outputs on the device: batchCap_ frames (dN_: n, then status)
    int batchCap_ = 0;
    std::vector<cv::KeyPoint> kps_;
    std::vector<unsigned char> desc_;
};
static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint), "KeyPoint layout");

}  // namespace ORB_SLAM
