// ORB_SLAM::TriangulateNewMapPoints over the C ABI of include/orbt.h (see NewMapPoints.h).
#include "NewMapPoints.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "orbt.h"

namespace ORB_SLAM {

namespace {

orbt_camera camera_of(KeyFrame* pKF) {
    orbt_camera c;
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) c.Rcw[r * 3 + k] = R.at<float>(r, k);
        c.tcw[r] = t.at<float>(r);
        c.Ow[r] = O.at<float>(r);
    }
    c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy;
    return c;
}

std::vector<orbx_keypoint> keypoints_of(const std::vector<cv::KeyPoint>& v) {
    std::vector<orbx_keypoint> out(v.size());
    for (std::size_t i = 0; i < v.size(); i++) {
        out[i].x = v[i].pt.x; out[i].y = v[i].pt.y; out[i].size = v[i].size; out[i].angle = v[i].angle;
        out[i].response = v[i].response; out[i].octave = v[i].octave; out[i].class_id = v[i].class_id;
    }
    return out;
}

}  // namespace

std::vector<NewMapPoint> TriangulateNewMapPoints(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<cv::KeyPoint>& vMatchedKeysUn1,
                                                 const std::vector<cv::KeyPoint>& vMatchedKeysUn2,
                                                 const std::vector<std::pair<std::size_t, std::size_t> >& vMatchedIndices,
                                                 std::vector<unsigned char>* status, int device) {
    const std::size_t n = vMatchedIndices.size();
    if (vMatchedKeysUn1.size() != n || vMatchedKeysUn2.size() != n) throw std::invalid_argument("TriangulateNewMapPoints: the three vectors differ in length");
    std::vector<NewMapPoint> out;
    if (status) status->assign(n, ORBT_NONE);
    if (n == 0) return out;
    orbt_pair pair;
    pair.kf1 = camera_of(pKF1);
    pair.kf2 = camera_of(pKF2);
    pair.scale_factor = pKF1->GetScaleFactor();
    pair.reserved = 0;
    // the level tables of both key frames, over the levels both have
    const std::vector<float> f1 = pKF1->GetScaleFactors(), s1 = pKF1->GetVectorScaleSigma2(), f2 = pKF2->GetScaleFactors(), s2 = pKF2->GetVectorScaleSigma2();
    const std::size_t nlevels = std::min(std::min(f1.size(), s1.size()), std::min(f2.size(), s2.size()));
    // match ikp pairs key point ikp of the first list with key point ikp of the second: vMatches12 is the identity
    const std::vector<orbx_keypoint> k1 = keypoints_of(vMatchedKeysUn1), k2 = keypoints_of(vMatchedKeysUn2);
    std::vector<int32_t> match12(n), acc_idx(2 * n);
    for (std::size_t i = 0; i < n; i++) match12[i] = (int32_t)i;
    std::vector<unsigned char> st(n);
    std::vector<float> x3d(3 * n), acc_x3d(3 * n);
    int count = 0;
    const int rc = orbt_triangulate(&pair, f1.data(), s1.data(), f2.data(), s2.data(), (int)nlevels, k1.data(), (int)n, k2.data(), (int)n, match12.data(),
                                    st.data(), x3d.data(), 0, acc_idx.data(), acc_x3d.data(), (int)n, &count, device);
    if (rc != ORBX_OK) throw std::runtime_error("orbt_triangulate failed: " + std::to_string(rc));
    out.resize(count);
    for (int k = 0; k < count; k++) {
        const int ikp = acc_idx[2 * k];
        out[k].x3D = cv::Mat(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) out[k].x3D.at<float>(i) = acc_x3d[3 * k + i];
        out[k].idx1 = vMatchedIndices[ikp].first;
        out[k].idx2 = vMatchedIndices[ikp].second;
    }
    if (status) *status = st;
    return out;
}

}  // namespace ORB_SLAM
