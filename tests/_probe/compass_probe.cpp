// Test-only: the FAST compass pre-test of orb_slam_amd/csrc/orb_math.h (host instantiation) for ctypes
// (tests/test_fast_compass_host.py, tests/test_gpu_fast_compass.py).
#include "orb_math.h"
#include <stdint.h>
extern "C" {
int probe_avg_u8(int a, int b, int c) { return orbx::avg_u8(a, b, c); }
int probe_compass_r(int t) { return orbx::compass_r(t); }
int probe_compass_kb(int t) { return orbx::compass_kb(t); }
int probe_compass_kd(int t) { return orbx::compass_kd(t); }
// every ring pixel x and centre v at threshold t: out[x * 256 + v] = bright flag | dark flag << 1 | (an intermediate left 0..255) << 2
void probe_compass_table(int t, uint8_t* out) {
    const int r = orbx::compass_r(t), kb = orbx::compass_kb(t), kd = orbx::compass_kd(t);
    for (int x = 0; x < 256; x++)
        for (int v = 0; v < 256; v++) {
            const int h = orbx::avg_u8(x, 255 - v, r), b = orbx::avg_u8(h, kb, 0), g = orbx::avg_u8(h, kd, 0);
            const int wide = ((unsigned)h > 255u) | ((unsigned)b > 255u) | ((unsigned)g > 255u);
            out[x * 256 + v] = (uint8_t)(((b >> 7) & 1) | ((~g >> 7) & 1) << 1 | wide << 2);
        }
}
void probe_compass4(const uint32_t* c, const uint32_t* e, const uint32_t* w, const uint32_t* n, const uint32_t* s, uint32_t* out, long cnt, int t) {
    for (long i = 0; i < cnt; i++) out[i] = orbx::compass4_flags(c[i], e[i], w[i], n[i], s[i], t);
}
}
