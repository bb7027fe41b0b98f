// The route without orbp_sim3_search, for tools/bench_sim3.py: what ORB_SLAM::ORBmatcher::SearchBySim3 of orb_slam_amd/cpp/ORBmatcher.cc does per call
// on one host core: the pair arithmetic (what include/orbp.h states for orbp_sim3_from_pair), then for both directions the projection of every
// map point of the source key frame (ORBP_MODE_SIM3) and its query, packed BY FEATURE with a valid flag as that route packs them, so that the
// window search's query -> feature table is vnMatch as it stands.  The two searches are orbs_window_search_batch_device with ORBS_RULE_FREE and
// the agreement orbs_agreement_batch_device.  tests/test_sim3_host_route.py holds it against tests/sim3_ref.py.
// Build: g++ -O2 -ffp-contract=off -fPIC -shared (Makefile: tools/libsim3_host.so).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbp.h"

namespace {

// R * P + t as the cv::Mat product evaluates it
void rigid(const float* R, const float* t, const float* P, float* out) {
    for (int r = 0; r < 3; r++) {
        float a = 0.0f;
        for (int k = 0; k < 3; k++) a += R[r * 3 + k] * P[k];
        out[r] = a + t[r];
    }
}

// one direction: entry i is feature i of the source key frame, list[i] its point's slot (-1 none).  Returns the number of valid queries.
int direction(const float* Raw, const float* taw, const float* S, const float* t, const float* cam, const orbf_bounds* b, float th, const float* factors,
              int nlevels, const int32_t* list, const uint8_t* skip, int n, const float* geom, const uint8_t* desc, const uint8_t* live, int capacity,
              float* qxyr, int32_t* qlev, uint8_t* qdesc, uint8_t* qvalid) {
    int nq = 0;
    for (int i = 0; i < n; i++) {
        qvalid[i] = 0;
        if (skip && skip[i]) continue;
        const int s = list[i];
        if (s < 0 || s >= capacity || !live[s]) continue;
        const float* g = geom + (size_t)s * 8;
        float Pa[3], Pb[3];
        rigid(Raw, taw, g, Pa);
        rigid(S, t, Pa, Pb);
        if (Pb[2] < 0.0f) continue;
        const float invz = 1 / Pb[2];
        const float x = Pb[0] * invz, y = Pb[1] * invz;
        const float u = cam[0] * x + cam[2], v = cam[1] * y + cam[3];
        if (!(u >= b->min_x && u < b->max_x && v >= b->min_y && v < b->max_y)) continue;
        double s2 = 0;
        for (int k = 0; k < 3; k++) s2 += (double)Pb[k] * (double)Pb[k];
        const float dist = std::sqrt(s2);
        if (dist < g[6] || dist > g[7]) continue;
        const float ratio = dist / g[6];
        int lv = 0;
        while (lv < nlevels && factors[lv] < ratio) lv++;
        if (lv >= nlevels) lv = nlevels - 1;
        qxyr[i * 3] = u; qxyr[i * 3 + 1] = v; qxyr[i * 3 + 2] = th * factors[lv];
        qlev[i * 2] = lv - 1; qlev[i * 2 + 1] = lv;
        std::memcpy(qdesc + (size_t)i * 32, desc + (size_t)s * 32, 32);
        qvalid[i] = 1;
        nq++;
    }
    return nq;
}

}  // namespace

// geom: 8 floats per slot (position, normal, minDistance, maxDistance), desc: 32 bytes per slot, live: 1 byte per slot.  cam: fx fy cx cy.
// Direction 1 -> 2 fills the arrays with suffix 1 (n1 entries), direction 2 -> 1 those with suffix 2 (n2 entries); nq[2] the valid queries of
// each.  sim[24]: sR12, sR21 (row major), t21, and three unused floats, for the test.  Returns -1 for a scale that is zero or not finite.
extern "C" int sim3_host_queries(float s12, const float* R12, const float* t12, const float* R1w, const float* t1w, const float* R2w, const float* t2w,
                                 const float* cam, const orbf_bounds* b, float th, const float* factors, int nlevels, const int32_t* list1, const uint8_t* skip1,
                                 int n1, const int32_t* list2, const uint8_t* skip2, int n2, const float* geom, const uint8_t* desc, const uint8_t* live,
                                 int capacity, float* qxyr1, int32_t* qlev1, uint8_t* qdesc1, uint8_t* qvalid1, float* qxyr2, int32_t* qlev2, uint8_t* qdesc2,
                                 uint8_t* qvalid2, int32_t* nq, float* sim) {
    if (s12 == 0.0f || !std::isfinite(s12)) return -1;
    float sR12[9], sR21[9], t21[3];
    const double inv = 1.0 / s12;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            sR12[r * 3 + c] = (float)(R12[r * 3 + c] * (double)s12);
            sR21[r * 3 + c] = (float)(R12[c * 3 + r] * inv);
        }
    for (int r = 0; r < 3; r++) {
        float a = 0.0f;
        for (int k = 0; k < 3; k++) a += -sR21[r * 3 + k] * t12[k];
        t21[r] = a;
    }
    if (sim) { std::memcpy(sim, sR12, 36); std::memcpy(sim + 9, sR21, 36); std::memcpy(sim + 18, t21, 12); }
    nq[0] = direction(R1w, t1w, sR21, t21, cam, b, th, factors, nlevels, list1, skip1, n1, geom, desc, live, capacity, qxyr1, qlev1, qdesc1, qvalid1);
    nq[1] = direction(R2w, t2w, sR12, t12, cam, b, th, factors, nlevels, list2, skip2, n2, geom, desc, live, capacity, qxyr2, qlev2, qdesc2, qvalid2);
    return 0;
}
