// The route without the device map-point table, for tools/bench_mappoints.py: Frame::isInFrustum's arithmetic (include/orbp.h) and the
// query packing of ORB_SLAM::ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>&, th) (orb_slam_amd/cpp/ORBmatcher.cc) on one
// host core, over plain arrays.  Build: g++ -O2 -ffp-contract=off -fPIC -shared (Makefile: tools/libmappoints_host.so).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbp.h"

extern "C" int host_queries(const orbp_view* V, const float* factors, int nlevels, const int32_t* list, const uint8_t* skip, int nlist,
                            const float* geom, const uint8_t* desc, const uint8_t* live, float* qxyr, int32_t* qlev, uint8_t* qdesc,
                            int32_t* qpos) {
    int nq = 0;
    for (int i = 0; i < nlist; i++) {
        if (skip && skip[i]) continue;
        const int s = list[i];
        if (!live[s]) continue;
        const float* g = geom + (size_t)s * 8;
        float Pc[3];
        for (int r = 0; r < 3; r++) {
            float a = 0.0f;
            for (int k = 0; k < 3; k++) a += V->Rcw[r * 3 + k] * g[k];
            Pc[r] = a + V->tcw[r];
        }
        if (Pc[2] < 0.0f) continue;
        const float invz = 1.0 / Pc[2];
        const float u = V->fx * Pc[0] * invz + V->cx, v = V->fy * Pc[1] * invz + V->cy;
        if (u < V->min_x || u > V->max_x || v < V->min_y || v > V->max_y || u != u || v != v) continue;
        double PO[3], s2 = 0, dot = 0;
        for (int k = 0; k < 3; k++) { PO[k] = g[k] - V->Ow[k]; s2 += PO[k] * PO[k]; }
        const float dist = std::sqrt(s2);
        if (dist < g[6] || dist > g[7]) continue;
        for (int k = 0; k < 3; k++) dot += PO[k] * g[3 + k];
        const float vc = dot / dist;
        if (vc < V->view_cos_limit) continue;
        const float ratio = dist / g[6];
        int lv = 0;
        while (lv < nlevels && factors[lv] < ratio) lv++;
        if (lv >= nlevels) lv = nlevels - 1;
        float r = vc > 0.998 ? 2.5f : 4.0f;
        if (V->th != 1.0) r *= V->th;
        qxyr[nq * 3] = u; qxyr[nq * 3 + 1] = v; qxyr[nq * 3 + 2] = r * factors[lv];
        qlev[nq * 2] = lv - 1; qlev[nq * 2 + 1] = lv;
        std::memcpy(qdesc + (size_t)nq * 32, desc + (size_t)s * 32, 32);
        qpos[nq++] = i;
    }
    return nq;
}

// every view of a batch in one call (view p writes its queries at offset p*qcap): the host loop is C++, not the caller's interpreter
extern "C" void host_queries_batch(const orbp_view* V, int nviews, const float* factors, int nlevels, const int32_t* list, int nlist, const float* geom,
                                   const uint8_t* desc, const uint8_t* live, int qcap, float* qxyr, int32_t* qlev, uint8_t* qdesc, int32_t* qpos,
                                   int32_t* nq) {
    for (int p = 0; p < nviews; p++)
        nq[p] = host_queries(V + p, factors, nlevels, list, nullptr, nlist, geom, desc, live, qxyr + (size_t)p * qcap * 3, qlev + (size_t)p * qcap * 2,
                             qdesc + (size_t)p * qcap * 32, qpos + (size_t)p * qcap);
}
