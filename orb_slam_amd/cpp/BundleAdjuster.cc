// ORB_SLAM::BundleAdjuster (BundleAdjuster.h): the graph of the reference's bundle adjustments gathered on the host, optimize(n) through include/orbb.h.
#include "BundleAdjuster.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <stdexcept>
#include <string>

namespace ORB_SLAM {

int BundleAdjuster::mnDevice = 0;
BundleAdjuster::Report BundleAdjuster::mReport;

namespace {

// the graph of one call: poses (free first), points, point-major edges, and the state
struct Graph {
    orbb_problem q;
    std::vector<KeyFrame*> poses;
    std::vector<MapPoint*> points;
    std::vector<float> cam, uv, invSigma2;
    std::vector<int32_t> first, edgePose;
    std::vector<KeyFrame*> vpEdgeKF;                // Optimizer.cc:388
    std::vector<MapPoint*> vpMapPointEdge;          // :394
    std::vector<double> qt, xyz, chi2;
    std::vector<uint64_t> active, flags;
};

// vertices and edges as :357-447 (resp. :64-125) make them
void gather(const std::vector<KeyFrame*>& free, const std::vector<KeyFrame*>& fixed, const std::vector<MapPoint*>& points, Graph& G) {
    G.poses = free;
    G.poses.insert(G.poses.end(), fixed.begin(), fixed.end());
    G.points = points;
    std::map<KeyFrame*, int32_t> index;
    std::vector<float> Tcw, world;
    for (size_t p = 0; p < G.poses.size(); p++) {
        KeyFrame* pKF = G.poses[p];
        index[pKF] = (int32_t)p;
        const cv::Mat T = pKF->GetPose();
        for (int i = 0; i < 12; i++) Tcw.push_back(T.at<float>(i / 4, i % 4));
        const float c[4] = {pKF->fx, pKF->fy, pKF->cx, pKF->cy};
        G.cam.insert(G.cam.end(), c, c + 4);
    }
    G.first.push_back(0);
    for (MapPoint* pMP : G.points) {
        const cv::Mat X = pMP->GetWorldPos();
        for (int i = 0; i < 3; i++) world.push_back(X.at<float>(i));
        const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
        for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); mit++) {
            KeyFrame* pKFi = mit->first;
            const std::map<KeyFrame*, int32_t>::const_iterator at = index.find(pKFi);
            if (pKFi->isBad() || at == index.end()) continue;
            const cv::KeyPoint kpUn = pKFi->GetKeyPointUn(mit->second);
            G.edgePose.push_back(at->second);
            G.uv.push_back(kpUn.pt.x);
            G.uv.push_back(kpUn.pt.y);
            G.invSigma2.push_back(pKFi->GetInvSigma2(kpUn.octave));
            G.vpEdgeKF.push_back(pKFi);
            G.vpMapPointEdge.push_back(pMP);
        }
        G.first.push_back((int32_t)G.edgePose.size());
    }
    G.q = orbb_problem{(int32_t)free.size(), (int32_t)fixed.size(), (int32_t)points.size(), (int32_t)G.edgePose.size()};
    G.qt.assign(G.poses.size() * 7, 0.0);
    G.xyz.assign(points.size() * 3 + 1, 0.0);
    G.chi2.assign(G.edgePose.size() + 1, 0.0);
    G.active.assign(ORBB_WORDS(G.q.nedges) + 1, 0);
    G.flags.assign(ORBB_WORDS(G.q.nedges) + 1, 0);
    for (int e = 0; e < G.q.nedges; e++) G.active[e >> 6] |= (uint64_t)1 << (e & 63);
    const int rc = orbb_state_from_float(&G.q, Tcw.data(), world.data(), G.qt.data(), G.xyz.data());
    if (rc != ORBX_OK) throw std::runtime_error("BundleAdjuster: the graph is outside include/orbb.h's limits (status " + std::to_string(rc) + ")");
}

// optimizer.optimize(nIterations) on the graph's state; returns the outer iterations run
int optimize(Graph& G, int nIterations, bool* pbStopFlag, int device, int& deviceCalls) {
    int done = 0;
    const float thHuber = std::sqrt(5.991);
    do {
        // a raised stop flag: g2o's loop runs no iteration when terminate() is true on entry
        const int n = (pbStopFlag && *pbStopFlag) ? 0 : std::min(nIterations - done, (int)ORBB_MAX_ITERS);
        orbb_result r;
        const int rc = orbb_optimize(&G.q, G.cam.data(), G.first.data(), G.edgePose.data(), G.uv.data(), G.invSigma2.data(), thHuber, G.qt.data(), G.xyz.data(),
                                     G.active.data(), G.chi2.data(), n, &r, G.flags.data(), nullptr, nullptr, device);
        if (rc != ORBX_OK) throw std::runtime_error("BundleAdjuster: orbb_optimize failed with status " + std::to_string(rc));
        deviceCalls++;
        done += r.iters;
        if (n == 0 || r.status != ORBB_RUN_OK) break;
    } while (done < nIterations);
    return done;
}

bool flagged(const Graph& G, size_t i) { return (G.flags[i >> 6] >> (i & 63)) & 1; }

// SetPose(Converter::toCvMat(SE3quat)), SetWorldPos and UpdateNormalAndDepth from the final state
void write_back(const Graph& G, const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP) {
    std::vector<float> Tcw(G.poses.size() * 16), world(G.points.size() * 3 + 1);
    orbb_state_to_float(&G.q, G.qt.data(), G.xyz.data(), Tcw.data(), world.data());
    std::map<KeyFrame*, size_t> poseOf;
    std::map<MapPoint*, size_t> pointOf;
    for (size_t p = 0; p < G.poses.size(); p++) poseOf[G.poses[p]] = p;
    for (size_t j = 0; j < G.points.size(); j++) pointOf[G.points[j]] = j;
    for (KeyFrame* pKF : vpKFs) {
        const std::map<KeyFrame*, size_t>::const_iterator at = poseOf.find(pKF);
        if (at == poseOf.end()) continue;
        cv::Mat T(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) T.at<float>(i / 4, i % 4) = Tcw[at->second * 16 + i];
        pKF->SetPose(T);
    }
    for (MapPoint* pMP : vpMP) {
        const std::map<MapPoint*, size_t>::const_iterator at = pointOf.find(pMP);
        if (at == pointOf.end()) continue;
        cv::Mat X(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) X.at<float>(i) = world[at->second * 3 + i];
        pMP->SetWorldPos(X);
        pMP->UpdateNormalAndDepth();
    }
}

}  // namespace

void BundleAdjuster::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag) {
    // Local KeyFrames: First Breath Search from Current Keyframe (:289-302)
    std::list<KeyFrame*> lLocalKeyFrames;
    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    const std::vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (int i = 0, iend = vNeighKFs.size(); i < iend; i++) {
        KeyFrame* pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }
    // Local MapPoints seen in Local KeyFrames (:304-320)
    std::list<MapPoint*> lLocalMapPoints;
    for (std::list<KeyFrame*>::iterator lit = lLocalKeyFrames.begin(); lit != lLocalKeyFrames.end(); lit++) {
        const std::vector<MapPoint*> vpMPs = (*lit)->GetMapPointMatches();
        for (std::vector<MapPoint*>::const_iterator vit = vpMPs.begin(); vit != vpMPs.end(); vit++) {
            MapPoint* pMP = *vit;
            if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
                lLocalMapPoints.push_back(pMP);
                pMP->mnBALocalForKF = pKF->mnId;
            }
        }
    }
    // Fixed Keyframes. Keyframes that see Local MapPoints but that are not Local Keyframes (:322-338)
    std::list<KeyFrame*> lFixedCameras;
    for (std::list<MapPoint*>::iterator lit = lLocalMapPoints.begin(); lit != lLocalMapPoints.end(); lit++) {
        const std::map<KeyFrame*, size_t> observations = (*lit)->GetObservations();
        for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); mit++) {
            KeyFrame* pKFi = mit->first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    }
    mReport = Report();
    mReport.vLocalKeyFrames.assign(lLocalKeyFrames.begin(), lLocalKeyFrames.end());
    mReport.vLocalMapPoints.assign(lLocalMapPoints.begin(), lLocalMapPoints.end());
    mReport.vFixedCameras.assign(lFixedCameras.begin(), lFixedCameras.end());

    // vertices (:357-380): vSE3->setFixed(pKFi->mnId==0) puts a local key frame with id 0 among the fixed poses
    std::vector<KeyFrame*> free, fixed;
    for (KeyFrame* pKFi : mReport.vLocalKeyFrames) (pKFi->mnId == 0 ? fixed : free).push_back(pKFi);
    fixed.insert(fixed.end(), lFixedCameras.begin(), lFixedCameras.end());
    Graph G;
    gather(free, fixed, mReport.vLocalMapPoints, G);
    mReport.nFree = G.q.nfree;
    mReport.nFixed = G.q.nfixed;
    mReport.nEdges = G.q.nedges;

    mReport.iters[0] = optimize(G, 5, pbStopFlag, mnDevice, mReport.deviceCalls);             // :449-450
    // Check inlier observations (:453-470)
    for (size_t i = 0, iend = G.vpEdgeKF.size(); i < iend; i++) {
        MapPoint* pMP = G.vpMapPointEdge[i];
        if (pMP->isBad()) continue;
        if (flagged(G, i)) {
            KeyFrame* pKFi = G.vpEdgeKF[i];
            pKFi->EraseMapPointMatch(pMP);
            pMP->EraseObservation(pKFi);
            G.active[i >> 6] &= ~((uint64_t)1 << (i & 63));                                  // optimizer.removeEdge(e); vpEdges[i]=NULL
            mReport.erased[0]++;
        }
    }
    mReport.iters[1] = optimize(G, 10, pbStopFlag, mnDevice, mReport.deviceCalls);            // :493-494
    // Check inlier observations (:497-515)
    for (size_t i = 0, iend = G.vpEdgeKF.size(); i < iend; i++) {
        if (!((G.active[i >> 6] >> (i & 63)) & 1)) continue;
        MapPoint* pMP = G.vpMapPointEdge[i];
        if (pMP->isBad()) continue;
        if (flagged(G, i)) {
            KeyFrame* pKFi = G.vpEdgeKF[i];
            pKFi->EraseMapPointMatch(pMP->GetIndexInKeyFrame(pKFi));
            pMP->EraseObservation(pKFi);
            mReport.erased[1]++;
        }
    }
    write_back(G, mReport.vLocalKeyFrames, mReport.vLocalMapPoints);                          // :517-535
}

void BundleAdjuster::BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag) {
    std::vector<KeyFrame*> free, fixed;
    for (KeyFrame* pKF : vpKFs)
        if (!pKF->isBad()) (pKF->mnId == 0 ? fixed : free).push_back(pKF);                   // :64-76
    std::vector<MapPoint*> points;
    for (MapPoint* pMP : vpMP)
        if (!pMP->isBad()) points.push_back(pMP);                                            // :82-86
    mReport = Report();
    Graph G;
    gather(free, fixed, points, G);
    mReport.nFree = G.q.nfree;
    mReport.nFixed = G.q.nfixed;
    mReport.nEdges = G.q.nedges;
    mReport.iters[0] = optimize(G, nIterations, pbStopFlag, mnDevice, mReport.deviceCalls);   // :129-130
    write_back(G, vpKFs, vpMP);                                                               // :132-150
}

}  // namespace ORB_SLAM
