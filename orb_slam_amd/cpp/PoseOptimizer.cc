// ORB_SLAM::PoseOptimizer (PoseOptimizer.h): the edges of Optimizer::PoseOptimization gathered on the host, the optimisation through include/orbo.h.
#include "PoseOptimizer.h"

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace ORB_SLAM {

int PoseOptimizer::mnDevice = 0;
PoseOptimizer::Report PoseOptimizer::mReport;

namespace {

// one frame's compact edges (Optimizer.cc:191-237)
struct Edges {
    orbo_problem q;
    std::vector<float> xyz, uv, invSigma2;
    std::vector<size_t> vnIndexEdge;
    std::vector<uint64_t> outlier;
    float Tcw[12];
};

void gather(Frame* pFrame, Edges& E) {
    const int N = pFrame->mvpMapPoints.size();
    for (int i = 0; i < N; i++) {
        MapPoint* pMP = pFrame->mvpMapPoints[i];
        if (!pMP) continue;
        pFrame->mvbOutlier[i] = false;
        const cv::Mat Xw = pMP->GetWorldPos();
        const cv::KeyPoint& kpUn = pFrame->mvKeysUn[i];
        for (int j = 0; j < 3; j++) E.xyz.push_back(Xw.at<float>(j));
        E.uv.push_back(kpUn.pt.x);
        E.uv.push_back(kpUn.pt.y);
        E.invSigma2.push_back(1.0f / pFrame->mvLevelSigma2[kpUn.octave]);       // Frame.cc:107: mvInvLevelSigma2
        E.vnIndexEdge.push_back(i);
    }
    E.q = orbo_problem{Frame::fx, Frame::fy, Frame::cx, Frame::cy, (int32_t)E.vnIndexEdge.size()};
    E.outlier.assign(ORBO_WORDS(E.q.n), 0);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) E.Tcw[r * 4 + c] = pFrame->mTcw.at<float>(r, c);
}

// mvbOutlier by key point, pose.copyTo(pFrame->mTcw), the return value (:252-284)
int scatter(Frame* pFrame, const Edges& E, const orbo_result& r) {
    for (size_t i = 0; i < E.vnIndexEdge.size(); i++) pFrame->mvbOutlier[E.vnIndexEdge[i]] = (E.outlier[i / 64] >> (i % 64)) & 1;
    for (int k = 0; k < 16; k++) pFrame->mTcw.at<float>(k / 4, k % 4) = r.Tcw[k];
    return r.ninitial - r.nbad;
}

}  // namespace

void PoseOptimizer::PoseOptimization(const std::vector<Frame*>& vpFrames, std::vector<int>* pnGood) {
    if (pnGood) pnGood->assign(vpFrames.size(), -1);
    std::vector<size_t> which;
    for (size_t i = 0; i < vpFrames.size(); i++)
        if (vpFrames[i]) which.push_back(i);
    mReport = Report();
    for (size_t first = 0; first < which.size(); first += ORBO_MAX_PROBLEMS) {
        const size_t P = std::min<size_t>(ORBO_MAX_PROBLEMS, which.size() - first);
        std::vector<Edges> E(P);
        std::vector<orbo_problem> q(P);
        std::vector<const float*> xyz(P), uv(P), w(P);
        std::vector<uint64_t*> fl(P);
        std::vector<float> T(P * 12);
        for (size_t p = 0; p < P; p++) {
            gather(vpFrames[which[first + p]], E[p]);
            q[p] = E[p].q;
            const bool any = q[p].n > 0;
            xyz[p] = any ? E[p].xyz.data() : nullptr;
            uv[p] = any ? E[p].uv.data() : nullptr;
            w[p] = any ? E[p].invSigma2.data() : nullptr;
            fl[p] = any ? E[p].outlier.data() : nullptr;
            std::copy(E[p].Tcw, E[p].Tcw + 12, T.begin() + p * 12);
        }
        std::vector<orbo_result> res(P);
        const int rc = orbo_pose_batch(q.data(), (int)P, xyz.data(), uv.data(), w.data(), T.data(), res.data(), fl.data(), nullptr, mnDevice);
        if (rc != ORBX_OK) throw std::runtime_error("PoseOptimizer: orbo_pose_batch failed with status " + std::to_string(rc));
        mReport.deviceCalls++;
        for (size_t p = 0; p < P; p++) {
            const int good = scatter(vpFrames[which[first + p]], E[p], res[p]);
            if (pnGood) (*pnGood)[which[first + p]] = good;
        }
        if (first == 0) {
            mReport.nInitial = res[0].ninitial;
            mReport.nBad = res[0].nbad;
            mReport.rounds = res[0].rounds;
            std::copy(res[0].iters, res[0].iters + ORBO_ROUNDS, mReport.iters);
        }
    }
}

int PoseOptimizer::PoseOptimization(Frame* pFrame) {
    std::vector<int> good;
    PoseOptimization(std::vector<Frame*>(1, pFrame), &good);
    return good[0];
}

}  // namespace ORB_SLAM
