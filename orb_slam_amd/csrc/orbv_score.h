// The merge walk of DBoW2/ScoringObject.cpp (:23-67 and the five sister functions), shared by orbv_score (host) and the
// key-frame database's scoring kernel (orbd_database.hip), so that the two cannot drift.  One sequential double sum in
// ascending word order; the reference's lower_bound jumps only skip keys that cannot match.  Built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "orbv.h"

namespace orbv {

// sc: ORBV_L1_NORM .. ORBV_DOT_PRODUCT.  The device path never sees ORBV_KL (orbd_create refuses it: device log need not
// equal the host's).
__host__ __device__ inline double score_walk(int sc, const uint32_t* id1, const double* val1, int n1, const uint32_t* id2,
                                             const double* val2, int n2) {
    const double log_eps = log(DBL_EPSILON);
    double s = 0;
    int i = 0, j = 0;
    while (i < n1 && j < n2) {
        if (id1[i] == id2[j]) {
            const double a = val1[i], b = val2[j];
            if (sc == ORBV_L1_NORM) s += fabs(a - b) - fabs(a) - fabs(b);
            else if (sc == ORBV_L2_NORM || sc == ORBV_DOT_PRODUCT) s += a * b;
            else if (sc == ORBV_CHI_SQUARE) { if (a + b != 0.0) s += a * b / (a + b); }
            else if (sc == ORBV_KL) { if (a != 0 && b != 0) s += a * log(a / b); }
            else s += sqrt(a * b);
            i++; j++;
        } else if (id1[i] < id2[j]) {
            if (sc == ORBV_KL) s += val1[i] * (log(val1[i]) - log_eps);
            i++;
        } else {
            j++;
        }
    }
    if (sc == ORBV_L1_NORM) return -s / 2.0;
    if (sc == ORBV_L2_NORM) return s >= 1 ? 1.0 : 1.0 - sqrt(1.0 - s);
    if (sc == ORBV_CHI_SQUARE) return 2. * s;
    if (sc == ORBV_KL) {
        for (; i < n1; i++) if (val1[i] != 0) s += val1[i] * (log(val1[i]) - log_eps);
        return s;
    }
    return s;
}

}  // namespace orbv
