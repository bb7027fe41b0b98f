// Test-only: the float column pass of k_describe_od's blur (orb_slam_amd/csrc/orb_math.h blurf_*, host instantiation) for ctypes
// (tests/test_blur_f16_host.py, tests/test_gpu_blur_f16.py).
#include "orb_math.h"
#include <stdint.h>
extern "C" {
// out: tap_hi[7], tap_lo[7], start
void probe_blurf_consts(float* out) {
    for (int t = 0; t < 7; t++) { out[t] = orbx::blurf_tap_hi(t); out[7 + t] = orbx::blurf_tap_lo(t); }
    out[14] = orbx::blurf_start();
}
int probe_blur_tap(int t) { return orbx::blur_tap(t); }
int probe_blurf_lo_bias() { return orbx::blurf_lo_bias(); }
int probe_blurf_mid_start() { return orbx::blurf_mid_start(); }
int probe_blurf_hi(int mid) { return orbx::blurf_hi(mid); }
int probe_blurf_lo(int mid) { return orbx::blurf_lo(mid); }
unsigned probe_f16_bits_scaled(int v, int shift) { return orbx::f16_bits_scaled(v, shift); }
int probe_blur_round_i(int sum, int te) { return orbx::blur_round(sum, te); }
// n columns of seven Mid values -> the float the column pass leaves, and its two roundings
void probe_blurf_columns(const int32_t* mid, long n, float* v, uint8_t* up, uint8_t* even) {
    for (long i = 0; i < n; i++) {
        v[i] = orbx::blurf_column(mid + 7 * i);
        up[i] = (uint8_t)orbx::blurf_round(v[i], 0);
        even[i] = (uint8_t)orbx::blurf_round(v[i], 1);
    }
}
// one 43 x 48 window -> the 37 x 40 blurred region the taps read (window rows 3 .. 39, columns 4 .. 43), the row pass in integers as the kernel's
void probe_blurf_window(const uint8_t* win, int ties_even, uint8_t* out) {
    int32_t mid[43][40];
    for (int r = 0; r < 43; r++)
        for (int c = 0; c < 40; c++) {
            const uint8_t* p = win + r * 48 + c + 1;
            mid[r][c] = orbx::blur_taps7(p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
        }
    for (int ro = 0; ro < 37; ro++)
        for (int c = 0; c < 40; c++) {
            int m[7];
            for (int t = 0; t < 7; t++) m[t] = mid[ro + t][c];
            out[ro * 40 + c] = (uint8_t)orbx::blurf_round(orbx::blurf_column(m), ties_even);
        }
}
}
