// Several host frames through ORBextractor::ExtractBatch (orbx_extract_batch, host form), checked against the one-frame operator().
// usage: example_batch <w> <h> <out file> <image.raw> <step> [<image.raw> <step> ...]
//   image.raw holds h rows of `step` bytes (the first w of each row are the image); writes per image N, keypoints (28 B each), descriptors
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ORBextractor.h"

int main(int argc, char** argv) {
    if (argc < 6 || (argc - 4) % 2) { std::fprintf(stderr, "usage: %s w h out.bin image.raw step [image.raw step ...]\n", argv[0]); return 2; }
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
    const int F = (argc - 4) / 2;
    std::vector<std::vector<unsigned char> > bufs(F);
    std::vector<cv::Mat> images;
    for (int i = 0; i < F; i++) {
        const size_t step = (size_t)std::atol(argv[5 + 2 * i]);
        bufs[i].resize(step * h);
        FILE* f = std::fopen(argv[4 + 2 * i], "rb");
        if (!f || std::fread(bufs[i].data(), 1, bufs[i].size(), f) != bufs[i].size()) { std::fprintf(stderr, "cannot read image %d\n", i); return 2; }
        std::fclose(f);
        images.push_back(cv::Mat(h, w, CV_8UC1, bufs[i].data(), step));
    }

    ORB_SLAM::ORBextractor extractor(1000, 1.2f, 8, ORB_SLAM::ORBextractor::FAST_SCORE, 20, 0, /*maxBatch=*/2);
    std::vector<std::vector<cv::KeyPoint> > keys;
    std::vector<cv::Mat> descs;
    extractor.ExtractBatch(images, keys, descs);

    int same = 1;
    FILE* o = std::fopen(argv[3], "wb");
    for (int i = 0; i < F; i++) {
        const int N = (int)keys[i].size();
        std::vector<cv::KeyPoint> k1;
        cv::Mat d1;
        extractor(images[i], cv::Mat(), k1, d1);                      // the one-frame call on the same image
        same &= (int)k1.size() == N && (N == 0 || std::memcmp(k1.data(), keys[i].data(), (size_t)N * sizeof(cv::KeyPoint)) == 0);
        for (int k = 0; k < N; k++) same &= std::memcmp(d1.ptr(k), descs[i].ptr(k), 32) == 0;
        std::fwrite(&N, 4, 1, o);
        std::fwrite(keys[i].data(), sizeof(cv::KeyPoint), N, o);
        for (int k = 0; k < N; k++) std::fwrite(descs[i].ptr(k), 1, 32, o);
        std::printf("image %d: N=%d\n", i, N);
    }
    std::fclose(o);
    std::printf("same_as_operator=%d\n", same);
    return same ? 0 : 1;
}
