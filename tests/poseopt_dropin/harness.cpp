// Drives ORB_SLAM::PoseOptimizer (orb_slam_amd/cpp/PoseOptimizer.cc) over the stand-in Frame.h and MapPoint.h of tests/standin: harness IN OUT.
// IN (binary, little endian): int32 nframes, mode (0: the frames one by one, 1: one batched call with a NULL entry in front), nlevels;
// float fx, fy, cx, cy; float sigma2[nlevels]; per frame: float Tcw[16]; int32 nkeys; per key point: float u, v; int32 octave, has (0: a NULL map
// point); float X, Y, Z.
// OUT: per frame: int32 good, nInitial, nBad, rounds, deviceCalls; float Tcw[16]; uint8 mvbOutlier[nkeys].
// Linked against liborbx.so (harness) it runs on the GPU, against tools/libposeopt_host.so (harness_host) the same class runs on the host.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "PoseOptimizer.h"
#include "harness_io.h"

template <class T> static void rd(std::FILE* f, T* p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: harness IN OUT\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int32_t hdr[3];
    float cam[4];
    rd(f, hdr, 3);
    rd(f, cam, 4);
    const int nframes = hdr[0], mode = hdr[1], nlevels = hdr[2];
    std::vector<float> sigma2(nlevels);
    rd(f, sigma2.data(), nlevels);
    ORB_SLAM::Frame::fx = cam[0]; ORB_SLAM::Frame::fy = cam[1]; ORB_SLAM::Frame::cx = cam[2]; ORB_SLAM::Frame::cy = cam[3];
    std::vector<std::unique_ptr<ORB_SLAM::Frame> > frames;
    std::vector<std::unique_ptr<ORB_SLAM::MapPoint> > points;
    for (int s = 0; s < nframes; s++) {
        frames.emplace_back(new ORB_SLAM::Frame);
        ORB_SLAM::Frame& F = *frames.back();
        float T[16];
        int32_t nkeys;
        rd(f, T, 16);
        rd(f, &nkeys, 1);
        F.mTcw = cv::Mat(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) F.mTcw.at<float>(i) = T[i];
        F.mvLevelSigma2 = sigma2;
        F.mvKeysUn.resize(nkeys);
        F.mvpMapPoints.assign(nkeys, nullptr);
        F.mvbOutlier.assign(nkeys, true);                      // the call clears the flag of every key point with a map point, and of no other
        for (int i = 0; i < nkeys; i++) {
            float uv[2], X[3];
            int32_t w[2];
            rd(f, uv, 2); rd(f, w, 2); rd(f, X, 3);
            F.mvKeysUn[i].pt.x = uv[0]; F.mvKeysUn[i].pt.y = uv[1]; F.mvKeysUn[i].octave = w[0];
            if (w[1]) {
                points.emplace_back(new ORB_SLAM::MapPoint);
                for (int j = 0; j < 3; j++) points.back()->mWorldPos.at<float>(j) = X[j];
                F.mvpMapPoints[i] = points.back().get();
            }
        }
    }
    std::fclose(f);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::vector<int> good(nframes, -1);
    std::vector<int32_t> calls(nframes, 0);
    std::vector<ORB_SLAM::PoseOptimizer::Report> reports(nframes);
    if (mode == 1) {
        std::vector<ORB_SLAM::Frame*> list(1, nullptr);        // the relocaliser's list has discarded candidates
        for (auto& F : frames) list.push_back(F.get());
        std::vector<int> g;
        ORB_SLAM::PoseOptimizer::PoseOptimization(list, &g);
        if (g[0] != -1) { std::fprintf(stderr, "a NULL entry must report -1\n"); return 3; }
        for (int s = 0; s < nframes; s++) { good[s] = g[s + 1]; reports[s].deviceCalls = ORB_SLAM::PoseOptimizer::LastReport().deviceCalls; }
    } else {
        for (int s = 0; s < nframes; s++) {
            good[s] = ORB_SLAM::PoseOptimizer::PoseOptimization(frames[s].get());
            reports[s] = ORB_SLAM::PoseOptimizer::LastReport();
        }
    }
    for (int s = 0; s < nframes; s++) {
        const ORB_SLAM::Frame& F = *frames[s];
        int32_t head[5] = {good[s], reports[s].nInitial, reports[s].nBad, reports[s].rounds, reports[s].deviceCalls};
        float T[16];
        for (int i = 0; i < 16; i++) T[i] = F.mTcw.at<float>(i);
        std::vector<uint8_t> fl(F.mvbOutlier.size());
        for (size_t i = 0; i < fl.size(); i++) fl[i] = F.mvbOutlier[i];
        std::fwrite(head, 4, 5, o);
        std::fwrite(T, 4, 16, o);
        std::fwrite(fl.data(), 1, fl.size(), o);
    }
    std::fclose(o);
    return 0;
}
