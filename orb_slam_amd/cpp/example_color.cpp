// Colour frames through ORBextractor::GrabImage (Tracking::GrabImage + Frame::Frame, orbx_extract_color) and the colour ExtractBatch
// (orbx_extract_batch_color, host form), each checked against the gray operator() on the gray image GrabImage hands back.
// usage: example_color <w> <h> <channels> <rgb 0|1> <out file> <image.raw> <step> [<image.raw> <step> ...]
//   image.raw holds h rows of `step` bytes (the first w * channels of each row are the pixels); writes per image the gray image (w*h bytes),
//   N, keypoints (28 B each), descriptors
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ORBextractor.h"

int main(int argc, char** argv) {
    if (argc < 8 || (argc - 6) % 2) { std::fprintf(stderr, "usage: %s w h channels rgb out.bin image.raw step [image.raw step ...]\n", argv[0]); return 2; }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), ch = std::atoi(argv[3]);
    const bool rgb = std::atoi(argv[4]) != 0;
    const int F = (argc - 6) / 2;
    const int type = ch == 4 ? CV_8UC4 : ch == 3 ? CV_8UC3 : CV_8UC1;
    std::vector<std::vector<unsigned char> > bufs(F);
    std::vector<cv::Mat> images;
    for (int i = 0; i < F; i++) {
        const size_t step = (size_t)std::atol(argv[7 + 2 * i]);
        bufs[i].resize(step * h);
        FILE* f = std::fopen(argv[6 + 2 * i], "rb");
        if (!f || std::fread(bufs[i].data(), 1, bufs[i].size(), f) != bufs[i].size()) { std::fprintf(stderr, "cannot read image %d\n", i); return 2; }
        std::fclose(f);
        images.push_back(cv::Mat(h, w, type, bufs[i].data(), step));
    }

    ORB_SLAM::ORBextractor extractor(1000, 1.2f, 8, ORB_SLAM::ORBextractor::FAST_SCORE, 20, 0, /*maxBatch=*/2);
    std::vector<std::vector<cv::KeyPoint> > keys;
    std::vector<cv::Mat> descs;
    extractor.ExtractBatch(images, rgb, keys, descs);

    int same = 1;
    FILE* o = std::fopen(argv[5], "wb");
    for (int i = 0; i < F; i++) {
        // what Tracking does per frame: GrabImage, then the Frame keeps imGray and the features
        cv::Mat imGray, d0;
        std::vector<cv::KeyPoint> k0;
        extractor.GrabImage(images[i], rgb, imGray, k0, d0);
        const int N = (int)k0.size();
        std::vector<cv::KeyPoint> k1;
        cv::Mat d1;
        extractor(imGray, cv::Mat(), k1, d1);                         // the gray call on the converted frame
        same &= imGray.rows == h && imGray.cols == w && imGray.channels() == 1;
        same &= (int)k1.size() == N && (N == 0 || std::memcmp(k1.data(), k0.data(), (size_t)N * sizeof(cv::KeyPoint)) == 0);
        same &= (int)keys[i].size() == N && (N == 0 || std::memcmp(keys[i].data(), k0.data(), (size_t)N * sizeof(cv::KeyPoint)) == 0);
        for (int k = 0; k < N; k++) same &= std::memcmp(d1.ptr(k), d0.ptr(k), 32) == 0 && std::memcmp(descs[i].ptr(k), d0.ptr(k), 32) == 0;
        for (int y = 0; y < h; y++) std::fwrite(imGray.ptr(y), 1, (size_t)w, o);
        std::fwrite(&N, 4, 1, o);
        std::fwrite(k0.data(), sizeof(cv::KeyPoint), N, o);
        for (int k = 0; k < N; k++) std::fwrite(d0.ptr(k), 1, 32, o);
        std::printf("image %d: N=%d\n", i, N);
    }
    std::fclose(o);
    std::printf("same_as_gray_operator=%d\n", same);
    return same ? 0 : 1;
}
