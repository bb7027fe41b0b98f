// The route without orbp_fuse, for tools/bench_fuse.py: the projection of ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>&, float th) (the
// arithmetic include/orbp.h states for ORBP_MODE_FUSE, what window_in_keyframe of orb_slam_amd/cpp/ORBmatcher.cc does per point) and the query
// packing on one host core, over plain arrays; the window search of the packed queries is orbs_window_search_batch_device with
// ORBS_RULE_FREE.  tests/test_fuse_host_route.py holds it against tests/fuse_ref.py.
// Build: g++ -O2 -ffp-contract=off -fPIC -shared (Makefile: tools/libfuse_host.so).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbp.h"

// geom: 8 floats per slot (position, normal, minDistance, maxDistance), desc: 32 bytes per slot, live: 1 byte per slot.  The queries that reach
// the window scan are packed in list order; qpos[q] is the list position of query q.  Returns their number.
extern "C" int fuse_host_queries(const orbp_view* V, const float* factors, int nlevels, const int32_t* list, const uint8_t* skip, int nlist,
                                 const float* geom, const uint8_t* desc, const uint8_t* live, int capacity, float* qxyr, int32_t* qlev, uint8_t* qdesc,
                                 int32_t* qpos) {
    int nq = 0;
    for (int i = 0; i < nlist; i++) {
        if (skip && skip[i]) continue;
        const int s = list[i];
        if (s < 0 || s >= capacity || !live[s]) continue;
        const float* g = geom + (size_t)s * 8;
        float Pc[3];
        for (int r = 0; r < 3; r++) {
            float a = 0.0f;
            for (int k = 0; k < 3; k++) a += V->Rcw[r * 3 + k] * g[k];
            Pc[r] = a + V->tcw[r];
        }
        if (Pc[2] < 0.0f) continue;
        const float invz = 1 / Pc[2];
        const float x = Pc[0] * invz, y = Pc[1] * invz;
        const float u = V->fx * x + V->cx, v = V->fy * y + V->cy;
        if (!(u >= V->min_x && u < V->max_x && v >= V->min_y && v < V->max_y)) continue;
        double PO[3], s2 = 0, dot = 0;
        for (int k = 0; k < 3; k++) { PO[k] = g[k] - V->Ow[k]; s2 += PO[k] * PO[k]; }
        const float dist = std::sqrt(s2);
        if (dist < g[6] || dist > g[7]) continue;
        for (int k = 0; k < 3; k++) dot += PO[k] * g[3 + k];
        if (dot < 0.5 * dist) continue;
        const float ratio = dist / g[6];
        int lv = 0;
        while (lv < nlevels && factors[lv] < ratio) lv++;
        if (lv >= nlevels) lv = nlevels - 1;
        qxyr[nq * 3] = u; qxyr[nq * 3 + 1] = v; qxyr[nq * 3 + 2] = V->th * factors[lv];
        qlev[nq * 2] = lv - 1; qlev[nq * 2 + 1] = lv;
        std::memcpy(qdesc + (size_t)nq * 32, desc + (size_t)s * 32, 32);
        qpos[nq++] = i;
    }
    return nq;
}
