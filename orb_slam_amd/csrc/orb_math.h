// Scalar arithmetic of the ORB front-end, written once for host and device (ORBX_HD) so the
// same expressions can be unit-tested on the CPU (tests/test_device_math.py builds this header
// with g++) and run inside the HIP kernels.  Everything here must evaluate identically under
// g++ and hipcc: no FMA contraction (-ffp-contract=off on both sides), IEEE +,-,*,/ only.
//
// Reference call sites (in /root/reference):
//   cvRound            src/ORBextractor.cc:102-103,:128,:166-167,:786  (OpenCV: round-half-to-even)
//   fastAtan2          src/ORBextractor.cc:150                         (OpenCV 2.4 mathfuncs.cpp)
//   cos/sin(float)     src/ORBextractor.cc:160                         (libm cosf/sinf)
//   cv::FAST score     src/ORBextractor.cc:607,:613                    (OpenCV fast_score.cpp cornerScore<16>)
//   cv::resize         src/ORBextractor.cc:800                         (OpenCV imgwarp.cpp, 8U fixed point)
//   cv::GaussianBlur   src/ORBextractor.cc:760                         (OpenCV smooth.cpp/filter.cpp, 8U fixed point)
//   DescriptorDistance src/ORBmatcher.cc:1794-1810
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ORBX_HD __host__ __device__ inline
#else
#define ORBX_HD inline
#endif

namespace orbx {

// cvRound(double(float v)): ties-to-even.  float->double is exact, so rintf suffices.
ORBX_HD int cv_round_f(float v) { return (int)rintf(v); }

ORBX_HD int imin(int a, int b) { return a < b ? a : b; }
ORBX_HD int imax(int a, int b) { return a > b ? a : b; }
ORBX_HD int imin3(int a, int b, int c) { return imin(imin(a, b), c); }
ORBX_HD int imax3(int a, int b, int c) { return imax(imax(a, b), c); }

// BORDER_REFLECT_101 index map (OpenCV borderInterpolate).
ORBX_HD int reflect101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        p = p < 0 ? -p : 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

// ---- cv::fastAtan2 (degrees, [0,360)) -------------------------------------------------------
// Coefficient products are formed in float exactly as the static initialisers of OpenCV do.
ORBX_HD float fast_atan2_deg(float y, float x) {
    const float k = (float)(180 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k;
    const float p5 = 0.1555786518463281f * k, p7 = -0.04432655554792128f * k;
    const float eps = 2.2204460492503131e-16f;   // (float)DBL_EPSILON
    float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + eps);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + eps);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// ---- sinf/cosf for the descriptor rotation ---------------------------------------------------
// The reference calls libm cosf/sinf (glibc).  A GPU cannot call glibc, so this is the published
// algorithm glibc >= 2.28 uses (Arm Optimized Routines sincosf: reduce by pi/2 in double, 8th/7th
// order minimax polynomials in double, one final rounding to float), written with plain double
// +,* so that host and device agree bit-for-bit.  tests/test_device_math.py measures it against
// this machine's glibc over the whole input range the path can produce ([0, 2*pi]).
// Valid for |x| < 120 (the path only produces [0, 6.2832]).
ORBX_HD void sincosf_orb(float y, float* sinp, float* cosp) {
    const double hpi_inv = 0x1.45F306DC9C883p+23;   // 2/pi * 2^24
    const double hpi = 0x1.921FB54442D18p0;         // pi/2
    const double c0 = 0x1p0, c1 = -0x1.ffffffd0c621cp-2, c2 = 0x1.55553e1068f19p-5;
    const double c3 = -0x1.6c087e89a359dp-10, c4 = 0x1.99343027bf8c3p-16;
    const double s1 = -0x1.555545995a603p-3, s2 = 0x1.1107605230bc4p-7, s3 = -0x1.994eb3774cf24p-13;
    double x = (double)y;
    int n = 0;
    const float ay = fabsf(y);
    if (!(ay < 0x1.921fb6p-1f)) {            // |y| >= pi/4 : reduce
        double r = x * hpi_inv;
        n = ((int32_t)r + 0x800000) >> 24;
        x = x - (double)n * hpi;
    }
    const double x2 = x * x;
    // sine polynomial (odd) and cosine polynomial (even) on the reduced argument
    double ps, pc;
    {
        double x3 = x * x2;
        double t1 = s2 + x2 * s3;
        double x7 = x3 * x2;
        double s = x + x3 * s1;
        ps = s + x7 * t1;
    }
    {
        double x4 = x2 * x2;
        double t2 = c3 + x2 * c4;
        double t1 = c0 + x2 * c1;
        double x6 = x4 * x2;
        double c = t1 + x4 * c2;
        pc = c + x6 * t2;
    }
    // quadrant: n&1 swaps, signs by n&2 / (n+1)&2
    double sv = (n & 1) ? pc : ps;
    double cv = (n & 1) ? ps : pc;
    if (n & 2) sv = -sv;
    if ((n + 1) & 2) cv = -cv;
    if (n == 0 && ay < 0x1p-12f) sv = (double)y;     // glibc returns y itself for tiny |y|
    *sinp = (float)sv;
    *cosp = (float)cv;
}

// ---- cv::FAST 9/16 corner score --------------------------------------------------------------
// d[k] = v - ring[k], k = 0..15 around the Bresenham circle.  Returns the OpenCV corner score
//   max over the 16 nine-pixel arcs of min(arc of d) (darker) / min(arc of -d) (brighter), minus 1,
// i.e. the largest threshold at which the pixel is still a FAST-9 corner, or 0 when that is < tmin
// (not a corner at threshold tmin).  corner@t <=> score >= t, independent of t.
// Window-9 circular min/max built from two rounds of 3-input min/max.
ORBX_HD int fast9_score(const int d[16], int tmin) {
    int lo3[16], hi3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        lo3[k] = imin3(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
        hi3[k] = imax3(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
    }
    int dark = -1000, bright = 1000;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        int lo9 = imin3(lo3[k], lo3[(k + 3) & 15], lo3[(k + 6) & 15]);
        int hi9 = imax3(hi3[k], hi3[(k + 3) & 15], hi3[(k + 6) & 15]);
        dark = imax(dark, lo9);
        bright = imin(bright, hi9);
    }
    int s = imax(dark, -bright) - 1;
    return s >= tmin ? s : 0;
}

// ---- the same score on packed halves (k_fast.hip phase B: fast_score_pk) ------------------------
// Two ring positions per 32-bit word: X[j] = x[j] | x[j + 8] << 16, j = 0..7, x the ring PIXELS (not differences).  Ring position i of any of
// the three levels (pixels, windows of 3, windows of 9) is R(i) = word i for i < 8 and word i - 8 WITH ITS HALVES SWAPPED for 8 <= i < 16, so
// that step j works on positions j (low half) and j + 8 (high half) at once:
//   hi3[j] = max3(R(j), R(j + 1), R(j + 2))       8 steps, halves (hi3[j], hi3[j + 8])
//   hi9[j] = max3(H3(j), H3(j + 3), H3(j + 6))    8 steps, halves (hi9[j], hi9[j + 8])
//   min over the 16 hi9: 8 words -> 3 -> 1 by min3 (4 steps), then the word against itself with swapped halves (1 step)
// and the same with min and max exchanged: 42 three-input steps where fast9_score takes 80.  The sources of a step are in rising position, so
// only three swap patterns occur: none, the third source, the second and third (PK_PLAIN / PK_SWAP_C / PK_SWAP_BC).
// OPS supplies max3 / min3 of three words per half with those patterns.  PkHalvesInt below does it with integer compares on the halves (the
// definition; tests/test_fast_score_pk_host.py holds fast9_score_pk against fast9_score); the kernel's PkHalvesF16 does each in one
// v_pk_maximum3_f16 / v_pk_minimum3_f16, the swaps by op_sel: a half 0x00XX is a positive f16 denormal, positive f16 order is integer order,
// and the kernels keep denormals (float_denorm_mode_16_64 = 3), so the instruction returns one of its inputs unchanged.
// d = v - x turns a max over pixels into a min over differences: in fast9_score's terms dark = max_k lo9(d) = v - min_k hi9(x) and
// bright = min_k hi9(d) = v - max_k lo9(x), so the score max(dark, -bright) - 1 is max(v - min_k hi9(x), max_k lo9(x) - v) - 1.
enum { PK_PLAIN = 0, PK_SWAP_C = 1, PK_SWAP_BC = 2 };
ORBX_HD uint32_t pk_swap(uint32_t a) { return a >> 16 | a << 16; }
struct PkHalvesInt {
    static ORBX_HD uint32_t each(uint32_t a, uint32_t b, uint32_t c, int form, bool want_max) {
        if (form >= PK_SWAP_C) c = pk_swap(c);
        if (form == PK_SWAP_BC) b = pk_swap(b);
        uint32_t o = 0;
        for (int h = 0; h < 32; h += 16) {
            const int x = (int)((a >> h) & 0xFFFFu), y = (int)((b >> h) & 0xFFFFu), z = (int)((c >> h) & 0xFFFFu);
            o |= (uint32_t)(want_max ? imax3(x, y, z) : imin3(x, y, z)) << h;
        }
        return o;
    }
    static ORBX_HD uint32_t max3(uint32_t a, uint32_t b, uint32_t c, int form) { return each(a, b, c, form, true); }
    static ORBX_HD uint32_t min3(uint32_t a, uint32_t b, uint32_t c, int form) { return each(a, b, c, form, false); }
};
// swap pattern of a step whose second / third source sit at ring positions ib <= ic (the first is always below 8)
ORBX_HD constexpr int pk_form(int ib, int ic) { return ib >= 8 ? PK_SWAP_BC : ic >= 8 ? PK_SWAP_C : PK_PLAIN; }
// min over k of hi9[k] (low half of the result) from the pixel words; MAXW = false: max over k of lo9[k]
template <class OPS, bool MAXW>
ORBX_HD uint32_t fast9_window_pk(const uint32_t X[8]) {
    uint32_t W3[8], W9[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int f = pk_form(j + 1, j + 2);
        W3[j] = MAXW ? OPS::max3(X[j], X[(j + 1) & 7], X[(j + 2) & 7], f) : OPS::min3(X[j], X[(j + 1) & 7], X[(j + 2) & 7], f);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int f = pk_form(j + 3, j + 6);
        W9[j] = MAXW ? OPS::max3(W3[j], W3[(j + 3) & 7], W3[(j + 6) & 7], f) : OPS::min3(W3[j], W3[(j + 3) & 7], W3[(j + 6) & 7], f);
    }
    // the other way round: the min of the window maxima
    auto red = [](uint32_t a, uint32_t b, uint32_t c, int f) { return MAXW ? OPS::min3(a, b, c, f) : OPS::max3(a, b, c, f); };
    const uint32_t m = red(red(W9[0], W9[1], W9[2], PK_PLAIN), red(W9[3], W9[4], W9[5], PK_PLAIN), red(W9[6], W9[7], W9[7], PK_PLAIN), PK_PLAIN);
    return red(m, m, m, PK_SWAP_BC) & 0xFFFFu;      // each half against the other
}
template <class OPS>
ORBX_HD int fast9_score_pk_with(const uint32_t X[8], int v, int tmin) {
    const int min_hi9 = (int)fast9_window_pk<OPS, true>(X), max_lo9 = (int)fast9_window_pk<OPS, false>(X);
    const int s = imax(v - min_hi9, max_lo9 - v) - 1;
    return s >= tmin ? s : 0;
}
// X[j] = ring[j] | ring[j + 8] << 16 (pixels 0..255), v the centre: == fast9_score of d[k] = v - ring[k]
ORBX_HD int fast9_score_pk(const uint32_t X[8], int v, int tmin) { return fast9_score_pk_with<PkHalvesInt>(X, v, tmin); }

// ---- FAST compass pre-test by byte averages (k_fast.hip phase A1) ------------------------------
// avg_u8 is one byte of v_lerp_u8: (a + b + (c & 1)) >> 1, the sum nine bits wide.  With x a ring pixel, v the centre, d = x - v,
// t the threshold and r = t & 1 (so that t + r is even):
//   h = avg_u8(x, 255 - v, r) = (255 + d + r) >> 1              in 0..255, monotone in d
//   bright:  bit 7 of avg_u8(h, compass_kb(t), 0)  is SET   <=>  h >= 128 + (t + r) / 2      <=>  d >  t      (exact)
//   dark:    bit 7 of avg_u8(h, compass_kd(t), 0)  is CLEAR <=>  h <= (254 + r - t) / 2      <=>  d <= -t     (d < -t, and d == -t)
// The dark side admits the one extra difference d == -t (253 + r - t is always odd, so no constant cuts h between -t and -t - 1: h
// was rounded with the bright side's r).  The test is a filter in front of the exact score, so a superset changes no result.
// Valid for 0 <= t <= 254; a larger t is clamped to 254: the filter then passes d = 255 and d <= -254 although nothing is a corner
// at such a threshold, and the exact score (fast_score_pk: s >= tmin) rejects those pixels as it rejects every other false flag.
// tests/test_fast_compass_host.py runs every (x, v, t).
ORBX_HD int avg_u8(int a, int b, int c) { return (a + b + (c & 1)) >> 1; }
ORBX_HD int compass_t(int t) { return t < 0 ? 0 : t > 254 ? 254 : t; }
ORBX_HD int compass_r(int t) { return compass_t(t) & 1; }
ORBX_HD int compass_kb(int t) { return 128 - (compass_t(t) + compass_r(t)) / 2; }
ORBX_HD int compass_kd(int t) { return 255 - (254 + compass_r(t) - compass_t(t)) / 2; }
// the same on four packed pixels (host form of the kernel's compass4; on the device each avg4_u8 is one v_lerp_u8): the flag of pixel j
// is bit 8 j + 7.  C: centres, E / W: pixels x + 3 / x - 3, N / S: rows y - 3 / y + 3; R, KB, KD: r, kb, kd in every byte.
ORBX_HD uint32_t avg4_u8(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t o = 0;
    for (int j = 0; j < 4; j++) o |= (uint32_t)avg_u8((int)((a >> (8 * j)) & 255u), (int)((b >> (8 * j)) & 255u), (int)((c >> (8 * j)) & 1u)) << (8 * j);
    return o;
}
ORBX_HD uint32_t compass4_flags(uint32_t C, uint32_t E, uint32_t W, uint32_t N, uint32_t S, int t) {
    const uint32_t R = (uint32_t)compass_r(t) * 0x01010101u, KB = (uint32_t)compass_kb(t) * 0x01010101u, KD = (uint32_t)compass_kd(t) * 0x01010101u;
    const uint32_t nc = ~C;
    const uint32_t hN = avg4_u8(N, nc, R), hS = avg4_u8(S, nc, R), hE = avg4_u8(E, nc, R), hW = avg4_u8(W, nc, R);
    const uint32_t br = (avg4_u8(hN, KB, 0) | avg4_u8(hS, KB, 0)) & (avg4_u8(hE, KB, 0) | avg4_u8(hW, KB, 0));
    const uint32_t dk = (avg4_u8(hN, KD, 0) & avg4_u8(hS, KD, 0)) | (avg4_u8(hE, KD, 0) & avg4_u8(hW, KD, 0));
    return (br | ~dk) & 0x80808080u;
}

// ---- cv::resize INTER_LINEAR 8U, one output pixel ----------------------------------------------
// s00,s01: source row sy0 at sx, sx+1; s10,s11: row sy1.  a0,a1 / b0,b1: 11-bit fixed-point weights.
ORBX_HD int resize_px(int s00, int s01, int s10, int s11, int a0, int a1, int b0, int b1) {
    int d0 = s00 * a0 + s01 * a1;
    int d1 = s10 * a0 + s11 * a1;
    return (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
}

// ---- GaussianBlur 7x7 sigma 2, 8U: fixed-point taps and final rounding --------------------------
// Taps x256: [18,34,49,55,49,34,18] (sum 257, not renormalised; KAT in tests/test_oracle_kat.py).
#define ORBX_G0 18
#define ORBX_G1 34
#define ORBX_G2 49
#define ORBX_G3 55
ORBX_HD int blur_taps7(int a, int b, int c, int d, int e, int f, int g) {
    return ORBX_G0 * (a + g) + ORBX_G1 * (b + f) + ORBX_G2 * (c + e) + ORBX_G3 * d;
}
// sum has 16 fractional bits.  ties_even = 1 for the columns OpenCV's SSE2 column filter handles
// (float accumulate + cvtps2dq), 0 for its scalar tail / non-SIMD build (half-up).  SURVEY.md A.5.
ORBX_HD int blur_round(int sum, int ties_even) {
    // half-up: (sum + 0x8000) >> 16;  ties-to-even: add 0x7FFF plus the parity of the integer part
    int q = (sum + 0x7FFF + (ties_even ? ((sum >> 16) & 1) : 1)) >> 16;
    return q > 255 ? 255 : q;
}

// ---- the blur's column pass as a float matrix product (k_describe_od.hip: v_mfma_f32_16x16x32_f16) -----------------
// The row pass leaves Mid = S_row = sum of tap * pixel, 0 .. 65535 (the taps sum to 257).  The column sum S = sum of tap * Mid has up to 25 bits
// and the int8 matrix product cannot carry the x 256 between Mid's two bytes; a float product can.  Per Mid element two f16 operands:
//   HI = Mid >> 8                 0 .. 255, exact in f16; it meets the tap scaled by 2^-8
//   LO = 1024 + (Mid & 255)       exact in f16 too, and its bit pattern is 0x6400 | (Mid & 255): a byte move, no conversion; tap scaled by 2^-16
// The 1024 of every LO slot is taken off again by the accumulator's start value, -1024 * 257 / 65536 (each output meets every tap once).
// Every product is an integer multiple of 2^-16 and every partial sum, in ANY order of the slots, lies in [start, S / 65536]: below 256 such
// a number has at most 24 significant bits, so float accumulation is exact and the result IS S / 65536 whenever that is below 256.  From
// 256 on (S up to 257 * 65535: 256.996) a sum may round to a multiple of 2^-15, and stays >= 255.5 because 255.5 is one: the output
// saturates either way.  blur_round's two modes are then round-to-nearest-even of that float, or floor(v + 0.5) (v + 0.5 is exact below 256),
// saturated.  tests/test_blur_f16_host.py runs structured, random and constructed-tie columns in random slot orders.
ORBX_HD constexpr int blur_tap(int t) { return t == 0 || t == 6 ? ORBX_G0 : t == 1 || t == 5 ? ORBX_G1 : t == 2 || t == 4 ? ORBX_G2 : t == 3 ? ORBX_G3 : 0; }
ORBX_HD constexpr int blur_tap_sum() { return blur_tap(0) + blur_tap(1) + blur_tap(2) + blur_tap(3) + blur_tap(4) + blur_tap(5) + blur_tap(6); }
ORBX_HD constexpr int blurf_lo_bias() { return 1024; }                                   // f16 1024.0 = 0x6400, ulp 1 up to 2047
ORBX_HD constexpr int blurf_hi(int mid) { return mid >> 8; }
ORBX_HD constexpr int blurf_lo(int mid) { return blurf_lo_bias() + (mid & 255); }
ORBX_HD constexpr float blurf_tap_hi(int t) { return (float)blur_tap(t) / 256.f; }
ORBX_HD constexpr float blurf_tap_lo(int t) { return (float)blur_tap(t) / 65536.f; }
ORBX_HD constexpr float blurf_start() { return -(float)(blurf_lo_bias() * blur_tap_sum()) / 65536.f; }
// the row pass's accumulator start that makes its int32 result 0x0064HHLL: pixels go in centred (p - 128), and byte 2 is the high byte of
// every f16 operand whose low byte is LL or HH (0x64HH = 1024 + HI: the kernel takes the 1024 off again with one packed f16 add)
ORBX_HD constexpr int blurf_mid_start() { return 128 * blur_tap_sum() + (0x64 << 16); }
// bit pattern of the f16 value v * 2^-shift for an integer 0 <= v < 2048 whose scaled value is a normal f16 number (0 for v = 0)
ORBX_HD constexpr uint32_t f16_bits_scaled(int v, int shift) {
    if (v <= 0) return 0u;
    int p = 0;
    while ((v >> p) > 1) p++;
    return (uint32_t)(p - shift + 15) << 10 | (((uint32_t)v << (10 - p)) & 0x3FFu);
}
// one output: mid[t] = the seven Mid values under the taps; the float the matrix product leaves (HI slots first here; any order gives the same)
ORBX_HD float blurf_column(const int mid[7]) {
    float acc = blurf_start();
    for (int t = 0; t < 7; t++) acc = acc + (float)blurf_hi(mid[t]) * blurf_tap_hi(t);
    for (int t = 0; t < 7; t++) acc = acc + (float)blurf_lo(mid[t]) * blurf_tap_lo(t);
    return acc;
}
ORBX_HD int blurf_round(float v, int ties_even) {
    const float r = ties_even ? rintf(v) : floorf(v + 0.5f);
    return r > 255.f ? 255 : r < 0.f ? 0 : (int)r;
}

// ---- 256-bit Hamming distance (host form; kernels use v_bcnt directly) -------------------------
ORBX_HD int hamming256_words(const uint32_t* a, const uint32_t* b) {
    int dist = 0;
    for (int i = 0; i < 8; i++) {
        dist += __builtin_popcount(a[i] ^ b[i]);
    }
    return dist;
}

}  // namespace orbx
