// Test-only: the exact FAST score of orb_slam_amd/csrc/orb_math.h on rings, in its plain form (fast9_score on differences) and in the packed
// form the kernels run (fast9_score_pk on two ring pixels per word, host instantiation), for ctypes
// (tests/test_fast_score_pk_host.py, tests/test_gpu_fast_score_pk.py).
#include "orb_math.h"
#include <stdint.h>
extern "C" {
// centre[i], ring[16 i + k] (ring order of k_fast.hip: k = 0 at (0, +3)) -> plain[i], packed[i]: the score, or 0 where it is below tmin
void probe_score_rings(const uint8_t* centre, const uint8_t* ring, uint8_t* plain, uint8_t* packed, long cnt, int tmin) {
    for (long i = 0; i < cnt; i++) {
        const uint8_t* r = ring + 16 * i;
        const int v = centre[i];
        int d[16];
        uint32_t X[8];
        for (int k = 0; k < 16; k++) d[k] = v - r[k];
        for (int j = 0; j < 8; j++) X[j] = (uint32_t)r[j] | (uint32_t)r[j + 8] << 16;
        plain[i] = (uint8_t)orbx::fast9_score(d, tmin);
        packed[i] = (uint8_t)orbx::fast9_score_pk(X, v, tmin);
    }
}
}
