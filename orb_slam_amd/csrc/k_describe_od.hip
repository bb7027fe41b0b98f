// k_describe_od — orientation + rBRIEF with the GaussianBlur computed ON DEMAND, per keypoint, on the matrix cores (round 6).
//
// reference: IC_Angle src/ORBextractor.cc:124-151, GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) :760, computeOrbDescriptor :154-194,
//            scaling / output :769-775.
//
// k_describe reads two things per keypoint: the 31 x 31 patch of the PLAIN level (IC_Angle) and the 37 x 37 window of the BLURRED level
// the rotated pattern can reach — the only consumer the blurred plane has.  Here a wave stages ONE 43 x 48-byte window of the plain
// level per keypoint (rows y-21 .. y+21, 48 bytes from the 4-byte aligned column at or left of x-22: the patch AND everything the 7 x 7
// filter needs around the 37 x 37 tap window), computes IC_Angle from it, then blurs it IN PLACE with exact matrix products (the row pass
// on v_mfma_i32_16x16x64_i8, the arithmetic of k_blur_mfma on window-shaped operands; the column pass on v_mfma_f32_16x16x32_f16, exact as
// well: orb_math.h blurf_*) and takes the 512 taps from the result.  The blurred
// plane, the blur kernel (VGA: 0.49 ms and 2.2 GB per 1024 frames; 1080p: 0.80 ms per 256 frames on the VALU) and the second gather
// of every keypoint disappear; the windows of a frame cover 1.4 x the pyramid's pixels at VGA / 1000 and 0.58 x at 1080p / 2000.
//
//   window      row r <-> level row y-21+r, reflected (BORDER_REFLECT_101) by the loader's row index; byte c <-> level column xs+c with
//               xs = (x-22) & ~3 (window column cx = x-xs in 22..25 is the keypoint).  Loaded by 16-byte LDS-DMA, three chunks per row:
//               129 chunks = three wave instructions per keypoint (one of them a single lane).  Chunks that would leave the row's readable
//               bytes are fetched from a clamped start and put right afterwards, together with the reflected columns of windows that
//               reach over the level's left / right edge, by LDS-to-LDS byte moves (border keypoints only, a few % of a frame).
//               The window is then the level's reflect-101 extension at DISTINCT positions: every window takes the same arithmetic.
//   row pass    Mid[r][c'] = sum_t tap[t] * In[r][c'+1+t]  (c' <-> window column c'+4: outputs start on a dword): per 16-column tile
//               ct and 16-row tile t one MFMA, A = the window rows (a lane's 16 bytes are one ds_read_b128), B = the banded tap matrix
//               (a lane constant).  Pixels go in centred (p - 128) and the accumulator starts at blurf_mid_start(), so the 32-bit result
//               is 0x0064HHLL with HHLL = S_row: a v_perm_b32 per two elements makes the f16 pair (1024 + LL) of the column pass's LO
//               operand, another the pair (1024 + HH), which one v_pk_add_f16 turns into the HI operand (orb_math.h blurf_hi / blurf_lo).
//   column pass Out[ro][c'] = sum_t tap[t] * Mid[ro+t][c'] as a float product: the row pass leaves lane (c' % 16, g) with Mid rows
//               16t+4g+i of column c' (i = 0 .. 3), whose four register pairs LO01 HI01 LO23 HI23 ARE an A operand of
//               v_mfma_f32_16x16x32_f16 (lane (m, g) holds K = 8g .. 8g+7) for row tile t: no data moves between the passes.  The tap
//               matrix (x 2^-8 in the HI slots, x 2^-16 in the LO slots, a lane constant) is numbered to match.  An output row needs two
//               row tiles, i.e. two chained products per 16 x 16 tile; the accumulator starts at blurf_start() and ends at S / 65536, exactly.
//               The result has four consecutive COLUMNS of one output row per lane: one aligned ds_write_b32 into the window, in place.
//   rounding    (S + 0x8000) >> 16 half-up or ties-to-even by ABSOLUTE column (x < w & ~3: OpenCV's SSE2 column filter), saturated —
//               orb_math.h blur_round, as k_blur / k_blur_mfma: here round-to-nearest-even resp. floor(v + 0.5) of the float
//               (blurf_round), then v_cvt_pk_u8_f32, which saturates and puts the byte into the output dword.
//   H4          taps up to 2 px outside the level read the UNBLURRED reflect-101 border in the reference.  Outputs at
//               out-of-level positions are simply not written: the window keeps the plain reflected pixel there.
//   tiles       two 16-wide tiles per axis per window; the last 8 columns and 5 rows of two windows share one tile (see the blur below).
// 20 MFMAs (7.5 int8, 12.5 f16) and ~87 VALU instructions per keypoint for the blur (listing, fast epilogue: 170 per pair + 8 for the corner);
// a wave owns four keypoints.
#include <algorithm>
#include <type_traits>

#include "orbx_device.h"
#include "orbx_launch.h"

namespace orbx {

constexpr int OD_KPW = 4;                                        // keypoints per wave (16 lanes each for IC_Angle and the taps)
constexpr int OD_PITCH = 48, OD_ROWS = 43;
constexpr int OD_WIN_BYTES = OD_PITCH * OD_ROWS;                 // 2064 (a multiple of 16)
constexpr int OD_CHUNKS = OD_ROWS * 3;                           // 129 16-byte chunks
constexpr int OD_WAVES = DESC_WAVES;
constexpr int OD_TAIL = 512;                                     // the operand reads of row tile 2 run 5 rows past a window (garbage in, unused out)

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int float_bits(float v) { return __builtin_bit_cast(int, v); }
typedef const void __attribute__((address_space(1))) * gptr_t;
typedef void __attribute__((address_space(3))) * lptr_t;

// Everything the kernel's lanes need that does not depend on the key point, computed by the COMPILER (constant memory, one load each instead of
// ~170 VALU instructions per wave): the circle masks of the IC_Angle patch, the BRIEF pattern as floats, and the tap operands of the two passes.
constexpr int od_tap(int t) { return t >= 0 && t <= 6 ? (int)((0x12223137312212ull >> (8 * t)) & 255ull) : 0; }      // [18, 34, 49, 55, 49, 34, 18][t], 0 outside
constexpr uint32_t od_taps4(int t0) { return (uint32_t)od_tap(t0) | (uint32_t)od_tap(t0 + 1) << 8 | (uint32_t)od_tap(t0 + 2) << 16 | (uint32_t)od_tap(t0 + 3) << 24; }
struct OdTables {
    uint32_t mask[256];            // circle byte masks of the 31 x 8 patch dwords (umax[] of reference :495-510; slots 248.. = 0)
    float pat[256][4];             // test t: x0, y0, x1, y1
    uint32_t trow[3][64][4];       // row pass, lane: K = 16 g + 4 v + byte; [ct < 2]: window column K, output column c' = 16 ct + n;
                                   // [2] (PCOL): K block 2 = the first window's columns 32 .. 47 -> c' = 32 + n (n < 8), block 3 = the second's -> c' = 24 + n (n >= 8)
    uint32_t tcol[4][64][4];       // column pass (f16 pairs), lane (n, g), register v, half h: K = 8 g + 2 v + h <-> LO (v even) / HI (v odd) of Mid row
                                   // 16 t + 4 g + 2 (v / 2) + h of the product's row tile t; output row ro = 16 rt + n: [0] t = rt, [1] t = rt + 1;
                                   // (PROW, CORNER) ro = 32 + (n & 7), t = 2: [2] the first window's (n < 5), [3] the second's (8 <= n < 13)
};
constexpr uint32_t c_pattern_host[256] = {
#include "orb_pattern_packed.inc"
};
constexpr OdTables make_od_tables() {
    OdTables T{};
    for (int t = 0; t < 256; t++) {
        const int r = t >> 3, c = t & 7;
        const int v = r - HALF_PATCH, av = v < 0 ? -v : v;
        const int um = r < 31 ? (int)((UMAX_NIBBLES >> (4 * (av & 15))) & 15ull) : -1;
        uint32_t mask = 0;
        for (int kk = 0; kk < 4; kk++) {
            const int u = 4 * c + kk - HALF_PATCH;
            if ((u < 0 ? -u : u) <= um) mask |= 0xFFu << (8 * kk);
        }
        T.mask[t] = mask;
        const uint32_t pk = c_pattern_host[t];
        for (int e = 0; e < 4; e++) T.pat[t][e] = (float)(int)(int8_t)(uint8_t)(pk >> (8 * e));
    }
    for (int c = 0; c < 3; c++)
        for (int l = 0; l < 64; l++)
            for (int v = 0; v < 4; v++) {
                const int n = l & 15, g = l >> 4;
                if (c < 2) T.trow[c][l][v] = od_taps4(16 * g + 4 * v - (16 * c + n) - 1);
                else T.trow[c][l][v] = g == 2 && n < 8 ? od_taps4(4 * v - n - 1) : g == 3 && n >= 8 ? od_taps4(4 * v - (n - 8) - 1) : 0u;
            }
    for (int c = 0; c < 4; c++)
        for (int l = 0; l < 64; l++)
            for (int v = 0; v < 4; v++) {
                const int n = l & 15, g = l >> 4;
                uint32_t word = 0;
                for (int h = 0; h < 2; h++) {
                    const int row = 4 * g + 2 * (v >> 1) + h;                   // Mid row inside the product's row tile
                    const int t = c == 0 ? row - n : c == 1 ? 16 + row - n : c == 2 ? (n < 5 ? row - n : -1) : (n >= 8 && n < 13 ? row - (n - 8) : -1);
                    word |= f16_bits_scaled(blur_tap(t), (v & 1) ? 8 : 16) << (16 * h);      // blurf_tap_hi / blurf_tap_lo
                }
                T.tcol[c][l][v] = word;
            }
    return T;
}
static __device__ __constant__ OdTables c_od = make_od_tables();

typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
// v_cvt_pk_u8_f32 rounds to nearest even and saturates to 0 .. 255 (profiles/describe_od_f16_probe.txt (c)); were it otherwise, a v_rndne_f32 goes in front
constexpr bool OD_CVT_RNE = true;
constexpr int OD_GEN = 0, OD_EVEN = 1, OD_UP = 2;           // the epilogue's forms: per-lane tie mode and H4 merge; ties to even everywhere; half up everywhere

// ---- the blur of a wave's four windows in place, two windows (a pair: slots 2 p, 2 p + 1) at a time, the whole wave on each.
// win0: the wave's OD_KPW windows (+ OD_TAIL readable bytes behind the last); nlive: 1 .. 4 of them are in use (wave-uniform); per window
// (wave-uniform) w0 .. w3: xs / yq = level column of its byte 0 / level row of its row 21, tw = its tie mode where that is uniform (1: ties to even),
// gen = it takes the per-lane epilogue — an edge window (H4 merge against Lw x Lh), or one whose outputs straddle Lwvec (ties-to-even
// columns x < Lwvec, half up beyond).  Trow / Tcol: the lane's rows of c_od.trow / c_od.tcol[0 .. 1]; tprow: the lane's row of c_od.tcol[2] in
// LDS, that of c_od.tcol[3] 64 entries behind it (five uses per wave: read where they are used, they would cost the kernel its fourth wave per SIMD).
// Output column c' <-> window column c' + 4, output row ro <-> window row ro + 3; the taps read c' <= 39, ro <= 36.  Tiles:
//   OWN     c' 16 ct .. +15, ro 16 rt .. +15 (ct, rt < 2) of one window: 4 per window; the column pass's two products take the row pass's row
//           tiles rt and rt + 1
//   PROW    c' 16 ct .. +15, ro 32 .. 36 of BOTH windows of a pair: the first product takes the first window's row tile 2 (Mid rows 32 .. 47)
//           with taps on N < 5 <-> its row 32 + N, the second the second window's with taps on N = 8 .. 12 <-> its row 32 + N - 8
//           (N = 5 .. 7, 13 .. 15: zero taps, stored to rows 37 .. 39, which nothing reads once the pair's operands are in registers)
//   PCOL    c' 32 .. 39 of both windows of a pair, ro 16 rt .. +15: the row pass's K block 2 is the first window's bytes 32 .. 47 (as
//           always) and block 3 the second window's (the first window's operand read fetches them there; the column tiles of one
//           window have zero taps on block 3); M < 8 <-> the first window's column 32 + M, M >= 8 <-> the second's column 32 + M - 8
//   CORNER  c' 32 .. 39, ro 32 .. 36 of all four windows: PROW's two products on PCOL's row tile 2 of pair 1 and of pair 0
// Per four windows 30 row-pass and 50 column-pass MFMAs and 25 epilogues instead of 36, 72 and 36 (three 16 x 16 tiles per axis, the third
// overlapping the second).  Every output the taps read is written exactly once; per pair, both windows' operands are read before the first store.
struct OdWin { int xs, yq; uint32_t tw; bool gen; };      // (scalars, not arrays: an array reference indexed by a lane value would live in scratch)
__device__ __forceinline__ void od_blur_windows(uint8_t* win0, int lane, int nlive, OdWin w0, OdWin w1, OdWin w2, OdWin w3, int Lw, int Lh, int Lwvec, const v4i (&Trow)[3], const v4i (&Tcol)[2], const v4i* tprow) {
    const int n16 = lane & 15, g4 = lane >> 4;               // the MFMA's view of the lane: row / column lane % 16, K block lane / 16
    const unsigned a_off = (unsigned)(n16 * OD_PITCH + 16 * g4);                                             // the lane's 16 operand bytes in a row tile
    const unsigned a_offp = g4 == 3 ? (unsigned)(OD_WIN_BYTES + n16 * OD_PITCH + 32) : a_off;               // (first window of a pair) block 3: the second's bytes 32 ..
    const unsigned o_own = (unsigned)((n16 + 3) * OD_PITCH + 4 + 4 * g4);                                    // OWN (0, 0)
    const unsigned o_prow = (unsigned)((n16 >= 8 ? OD_WIN_BYTES : 0) + ((n16 & 7) + 35) * OD_PITCH + 4 + 4 * g4);          // PROW of column tile 0
    const unsigned o_pcol = (unsigned)((g4 >= 2 ? OD_WIN_BYTES : 0) + (n16 + 3) * OD_PITCH + 36 + 4 * (g4 & 1));          // PCOL of row tile 0
    const unsigned o_corner = (unsigned)((n16 < 8 ? 2 : 0) * OD_WIN_BYTES + (g4 >= 2 ? OD_WIN_BYTES : 0) + ((n16 & 7) + 35) * OD_PITCH + 36 + 4 * (g4 & 1));
    const v4i cmid = {blurf_mid_start(), blurf_mid_start(), blurf_mid_start(), blurf_mid_start()};
    const h2v unbias = {(_Float16)-blurf_lo_bias(), (_Float16)-blurf_lo_bias()};
    // row pass of one column tile: z[t] = 0x0064HHLL for Mid rows 16 t + 4 g + i, made into the column pass's operand of row tile t: the f16 pairs
    // LO01, HI01, LO23, HI23 (LO = 0x64LL = 1024 + LL as it stands, HI = 0x64HH - 1024)
    auto row_pass = [&](const v4i (&A)[3], const v4i& T, v4i (&M)[3]) {
        v4i z[3];
#pragma unroll
        for (int t = 0; t < 3; t++) z[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t], T, cmid, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t z0 = (uint32_t)z[t][2 * h], z1 = (uint32_t)z[t][2 * h + 1];
                M[t][2 * h] = (int)__builtin_amdgcn_perm(z1, z0, 0x06040200u);                                // LL0 64 LL1 64
                M[t][2 * h + 1] = __builtin_bit_cast(int, __builtin_bit_cast(h2v, __builtin_amdgcn_perm(z1, z0, 0x06050201u)) + unbias);      // HH0 64 HH1 64, - 1024 each
            }
    };
    // column pass of one tile (row tiles Ma, Mb against the tap operands Ta, Tb) + rounding + saturation + the aligned store.  The lane's dword is
    // output columns cb .. cb + 3 of output row ro of the window at column xs_l / row yq_l (GEN only: per-lane tie mode and H4 merge; otherwise the
    // pair's uniform tie mode, whose half-up form starts the accumulator 0.5 higher and floors).  MODE: OD_GEN, OD_EVEN, OD_UP.
    auto epilogue = [&](auto MODE, const v4i& Ma, const v4i& Mb, const v4i& Ta, const v4i& Tb, uint8_t* dst, int xs_l, int yq_l, int cb, int ro) {
        constexpr bool gen = decltype(MODE)::value == OD_GEN, twu = decltype(MODE)::value == OD_EVEN;
        constexpr float st = (gen || twu) ? blurf_start() : blurf_start() + 0.5f;
        f4v acc = {st, st, st, st};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8v, Ma), __builtin_bit_cast(h8v, Ta), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8v, Mb), __builtin_bit_cast(h8v, Tb), acc, 0, 0, 0);
        float v[4] = {acc[0], acc[1], acc[2], acc[3]};
        uint32_t keep = 0;
        if (gen) {
            const int X0 = xs_l + 4 + cb;                    // level column of the lane's first output byte (a multiple of 4)
            const bool te = X0 < Lwvec;
            uint32_t keepc = 0;                              // bytes whose column lies outside the level
#pragma unroll
            for (int bb = 0; bb < 4; bb++) keepc |= ((unsigned)(X0 + bb) < (unsigned)Lw ? 0u : 0xFFu) << (8 * bb);
            keep = (unsigned)(yq_l - 18 + ro) < (unsigned)Lh ? keepc : 0xFFFFFFFFu;
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = te ? __builtin_rintf(v[i]) : __builtin_floorf(v[i] + 0.5f);       // (blurf_round)
        } else if (!twu) {
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = __builtin_floorf(v[i]);
        } else if (!OD_CVT_RNE) {
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = __builtin_rintf(v[i]);
        }
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) o = __builtin_amdgcn_cvt_pk_u8_f32(v[i], (uint32_t)i, o);      // rounds (an integer stays), saturates, packs byte i
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        if (gen) o = (o & ~keep) | (*d & keep);              // out-of-level positions keep the plain reflected pixel (H4)
        *d = o;
    };
    v4i mc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};                // the corner's operands: row tile 2 of each pair's PCOL row pass (Mid rows 32 .. 47)
    // (the pair's wave-uniform values come in as scalars: the per-window arrays stay unindexed by the loop counter, i.e. out of scratch)
    auto blur_pair = [&](auto GEN, int p, int xs0, int yq0, int xs1, int yq1) {
        uint8_t* W = win0 + 2 * p * OD_WIN_BYTES;
        v4i A0[3], A1[3];
        {
            const unsigned r0 = (unsigned)(uintptr_t)(lptr_t)(W + a_offp), r1 = (unsigned)(uintptr_t)(lptr_t)(W + OD_WIN_BYTES + a_off);
            asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %6 offset:768\n\tds_read_b128 %2, %6 offset:1536\n\t"
                         "ds_read_b128 %3, %7\n\tds_read_b128 %4, %7 offset:768\n\tds_read_b128 %5, %7 offset:1536\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(A0[0]), "=&v"(A0[1]), "=&v"(A0[2]), "=&v"(A1[0]), "=&v"(A1[1]), "=&v"(A1[2]) : "v"(r0), "v"(r1) : "memory");
        }
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int e = 0; e < 4; e++) { A0[t][e] = (int)((uint32_t)A0[t][e] ^ 0x80808080u); A1[t][e] = (int)((uint32_t)A1[t][e] ^ 0x80808080u); }
        const int xs_r = n16 >= 8 ? xs1 : xs0, yq_r = n16 >= 8 ? yq1 : yq0;       // (GEN) PROW lanes' window
        const int xs_c = g4 >= 2 ? xs1 : xs0, yq_c = g4 >= 2 ? yq1 : yq0;         // (GEN) PCOL lanes' window
        {
            v4i MP[3];
            row_pass(A0, Trow[2], MP);
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
                epilogue(GEN, MP[rt], MP[rt + 1], Tcol[0], Tcol[1], W + o_pcol + 16 * rt * OD_PITCH, xs_c, yq_c, 32 + 4 * (g4 & 1), 16 * rt + n16);
            if (p == 0) { mc[0] = MP[2]; mc[1] = MP[2]; }    // (pair 1 idle: its corner lanes get pair 0's rows)
            else mc[1] = MP[2];
        }
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
            v4i M0[3], M1[3];                                // (one window after the other: only row tile 2 of the first outlives its own epilogues)
            row_pass(A0, Trow[ct], M0);
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
                epilogue(GEN, M0[rt], M0[rt + 1], Tcol[0], Tcol[1], W + o_own + (16 * rt * OD_PITCH + 16 * ct), xs0, yq0, 16 * ct + 4 * g4, 16 * rt + n16);
            row_pass(A1, Trow[ct], M1);
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
                epilogue(GEN, M1[rt], M1[rt + 1], Tcol[0], Tcol[1], W + OD_WIN_BYTES + o_own + (16 * rt * OD_PITCH + 16 * ct), xs1, yq1, 16 * ct + 4 * g4, 16 * rt + n16);
            epilogue(GEN, M0[2], M1[2], tprow[0], tprow[64], W + o_prow + 16 * ct, xs_r, yq_r, 16 * ct + 4 * g4, 32 + (n16 & 7));
        }
    };
#pragma unroll 1
    for (int p = 0; p < 2; p++) {
        if (p > 0 && nlive <= 2) continue;                   // wave-uniform
        const int xs0 = p ? w2.xs : w0.xs, yq0 = p ? w2.yq : w0.yq, xs1 = p ? w3.xs : w1.xs, yq1 = p ? w3.yq : w1.yq;
        const uint32_t tw0 = p ? w2.tw : w0.tw, tw1 = p ? w3.tw : w1.tw;
        if ((p ? w2.gen || w3.gen : w0.gen || w1.gen) || tw0 != tw1) blur_pair(std::integral_constant<int, OD_GEN>{}, p, xs0, yq0, xs1, yq1);
        else if (tw0) blur_pair(std::integral_constant<int, OD_EVEN>{}, p, xs0, yq0, xs1, yq1);
        else blur_pair(std::integral_constant<int, OD_UP>{}, p, xs0, yq0, xs1, yq1);
    }
    {
        const bool gen = w0.gen || w1.gen || w2.gen || w3.gen || w0.tw != w1.tw || w0.tw != w2.tw || w0.tw != w3.tw;
        const int wsc = (n16 < 8 ? 2 : 0) + (g4 >= 2 ? 1 : 0);
        const int xs_k = wsc == 0 ? w0.xs : wsc == 1 ? w1.xs : wsc == 2 ? w2.xs : w3.xs;
        const int yq_k = wsc == 0 ? w0.yq : wsc == 1 ? w1.yq : wsc == 2 ? w2.yq : w3.yq;
        if (gen) epilogue(std::integral_constant<int, OD_GEN>{}, mc[1], mc[0], tprow[0], tprow[64], win0 + o_corner, xs_k, yq_k, 32 + 4 * (g4 & 1), 32 + (n16 & 7));
        else if (w0.tw) epilogue(std::integral_constant<int, OD_EVEN>{}, mc[1], mc[0], tprow[0], tprow[64], win0 + o_corner, xs_k, yq_k, 32 + 4 * (g4 & 1), 32 + (n16 & 7));
        else epilogue(std::integral_constant<int, OD_UP>{}, mc[1], mc[0], tprow[0], tprow[64], win0 + o_corner, xs_k, yq_k, 32 + 4 * (g4 & 1), 32 + (n16 & 7));
    }
}

template <bool FMA, bool GATHER>
__device__ __forceinline__ void k_describe_od_body(const Batch& b) {
    __shared__ __attribute__((aligned(16))) float s_pat[256 * 4];       // test t: x0, y0, x1, y1 as floats (one ds_read_b128 = the two points as register pairs)
    __shared__ __attribute__((aligned(16))) uint32_t s_mask[256];       // circle byte masks of the 31 x 8 patch dwords (slots 248.. = 0)
    __shared__ __attribute__((aligned(16))) uint8_t s_win[OD_WAVES * OD_KPW * OD_WIN_BYTES + OD_TAIL];
    __shared__ __attribute__((aligned(16))) v4i s_tprow[2 * 64];        // c_od.tcol[2 .. 3] (with it 40,704 bytes: four workgroups per CU still fit 160 KB)
    const DevGeom& g = b.g;
    int frame, wgi;
    if (!frame_item(b, blockIdx.x, (g.nquads + OD_WAVES - 1) / OD_WAVES, frame, wgi)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int grp = lane >> 4, li = lane & 15;
    const float4 pat_first = *reinterpret_cast<const float4*>(c_od.pat[tid & 255]);      // requested first: loads return in order, the tables are built while the key points are on their way
    const uint32_t mask_first = c_od.mask[tid & 255];
    const uint2 tprow_first = reinterpret_cast<const uint2*>(c_od.tcol[2])[tid & 255];
    const int32_t* counts = b.level_count + frame * MAX_LEVELS;
    const int quad = wgi * OD_WAVES + wave_id();
    const bool live = quad < g.nquads;
    const int level = __builtin_amdgcn_readfirstlane(find_level(g.quad_bases, live ? quad : 0));
    const LevelGeom& LG = g.lv[level];
    struct { int w, h, stride, plane_off, sel_base, quad_base, wvec; float scale, kp_size; } L = {
        __builtin_amdgcn_readfirstlane(LG.w), __builtin_amdgcn_readfirstlane(LG.h), __builtin_amdgcn_readfirstlane(LG.stride),
        __builtin_amdgcn_readfirstlane(LG.plane_off), __builtin_amdgcn_readfirstlane(LG.sel_base), __builtin_amdgcn_readfirstlane(LG.quad_base),
        __builtin_amdgcn_readfirstlane(LG.blur_wvec),
        __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, LG.scale))),
        __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, LG.kp_size)))};
    // the wave's four keypoints, the per-level counts and the frame status: wave-uniform data by scalar loads (as k_describe)
    const int k0 = (quad - L.quad_base) * OD_KPW;
    Cand kp;
    typedef int v8i_s __attribute__((ext_vector_type(8)));
    v8i_s s_cnt0, s_cnt1;
    int st0;
    {
        const int sel_cap = __builtin_amdgcn_readfirstlane(LG.sel_cap);
        const int ks = __builtin_amdgcn_readfirstlane(max(min(k0, sel_cap - OD_KPW), 0));        // (the sel block carries 4 slots of padding)
        const Cand* kp4 = b.sel + ((long long)frame * g.frame_sel + L.sel_base + ks);
        const int32_t* stp = b.status + frame;
        // REQUIRES of Batch::sel: 4 readable Cand slots behind every level's list (the 32-byte load below may start up to 3 entries in front of the list's
        // last slot: ensure_geometry pads d_sel by DESC_KPW entries) and level_count rows of MAX_LEVELS >= 16 ints (two x8 loads).
        static_assert(MAX_LEVELS >= 16, "the per-level counts are fetched as two s_load_dwordx8");
        v8i_s kq;
        int sst;
        asm volatile("s_load_dwordx8 %0, %4, 0x0\n\ts_load_dwordx8 %1, %5, 0x0\n\ts_load_dwordx8 %2, %5, 0x20\n\ts_load_dword %3, %6, 0x0\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(kq), "=&s"(s_cnt0), "=&s"(s_cnt1), "=&s"(sst) : "s"(kp4), "s"(counts), "s"(stp) : "memory");
        st0 = sst;
        const int e = min(max(k0 + grp, 0), sel_cap - 1) - ks;       // 0 .. 3
        kp.pos = (uint32_t)(e == 0 ? kq[0] : e == 1 ? kq[2] : e == 2 ? kq[4] : kq[6]);
        kp.resp = __builtin_bit_cast(float, e == 0 ? kq[1] : e == 1 ? kq[3] : e == 2 ? kq[5] : kq[7]);
    }
    static_assert(OD_WAVES * 64 == 256, "one table entry per thread");
    reinterpret_cast<float4*>(s_pat)[tid] = pat_first;
    s_mask[tid] = mask_first;
    reinterpret_cast<uint2*>(s_tprow)[tid] = tprow_first;
    int out_base = 0, total = 0, cnt = 0;
    for (int l = 0; l < g.nlevels; l++) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) { if (l == i) c = s_cnt0[i]; if (l == 8 + i) c = s_cnt1[i]; }
        if (l < level) out_base += c;
        if (l == level) cnt = c;
        total += c;
    }
    const bool work = live && k0 < cnt && total <= b.cap && __builtin_amdgcn_readfirstlane(st0) == ORBX_OK;
    const bool valid = work && k0 + grp < cnt;
    const int k = valid ? k0 + grp : (work ? k0 : 0);       // idle groups shadow the wave's first keypoint (results dropped)
    if (!valid) {
        kp.pos = (uint32_t)__builtin_amdgcn_readlane((int)kp.pos, 0);
        kp.resp = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, kp.resp), 0));
    }
    if (quad == 0 && lane == 0) {
        int st = st0, tot = total;
        if (tot > b.cap) { st = ORBX_ERR_CAPACITY; tot = 0; }
        b.out_n[frame] = st == ORBX_OK ? tot : 0;
        if (b.out_status) b.out_status[frame] = st;
    }
    if (!work) return;
    const int x = kp.pos & 0xFFFF, y = kp.pos >> 16;
    const uint8_t* plain;
    unsigned pstride;                                        // rows < 2^24 bytes, planes < 2^31 bytes (host-checked)
    int wlim;                                                // bytes of a row that may be read (>= w and >= 64: host-checked)
    if (level == 0) {
        if constexpr (GATHER) {
            long long s0;
            plain = level0_src(b, frame, s0);
            pstride = (unsigned)s0;
        } else { pstride = (unsigned)b.img_row_stride; plain = b.img + (long long)frame * b.img_frame_stride; }
        wlim = (int)min((long long)pstride, (long long)((L.w + 15) & ~15));               // include/orbx.h: what a pitched caller buffer promises (any value: the 16-byte DMA takes byte-aligned sources)
    } else { pstride = (unsigned)L.stride; plain = b.pyr + (long long)frame * g.frame_plane_bytes + L.plane_off; wlim = L.stride; }
    uint8_t* const win0 = s_win + wave_id() * OD_KPW * OD_WIN_BYTES;

    // ---- the four windows by LDS-DMA: chunk e = 64 n + lane <-> row e / 3, chunk e % 3 of the row
    int erow[3], ecol[3];
    unsigned eoff[3];                                        // the chunk's offset from the window's first byte in the level
#pragma unroll
    for (int n = 0; n < 3; n++) {
        const int e = 64 * n + lane;
        erow[n] = (e * 171) >> 9;                            // e / 3 for e < 193
        ecol[n] = 16 * (e - 3 * erow[n]);
        eoff[n] = __umul24((unsigned)erow[n], pstride) + (unsigned)ecol[n];
    }
    uint32_t fixmask = 0;                                    // (wave-uniform) bit q: window q has columns to put right; bit 4 + q: it reaches outside the level
#pragma unroll
    for (int q = 0; q < OD_KPW; q++) {
        if (q > 0 && k0 + q >= cnt) continue;                // wave-uniform
        const unsigned posq = (unsigned)__builtin_amdgcn_readlane((int)kp.pos, 16 * q);
        const int xq = posq & 0xFFFF, yq = posq >> 16;
        const int xs = (xq - 22) & ~3;
        if (xs < 0 || xs + 48 > wlim || xq + 21 >= L.w) fixmask |= 1u << q;
        if (xq < 18 || xq + 18 >= L.w || yq < 18 || yq + 21 >= L.h) fixmask |= 16u << q;
        if (xs >= 0 && xs + 48 <= wlim && yq >= 21 && yq + 21 < L.h) {       // (wave-uniform) the whole window lies inside the level's readable rows:
            const uint8_t* srcq = plain + (__umul24((unsigned)(yq - 21), pstride) + (unsigned)xs);      // one scalar base, the lanes' constant offsets
#pragma unroll
            for (int n = 0; n < 3; n++)
                if (n < 2 || lane < OD_CHUNKS - 128)
                    __builtin_amdgcn_global_load_lds((gptr_t)(srcq + eoff[n]), (lptr_t)(win0 + q * OD_WIN_BYTES + 1024 * n), 16, 0, 0);
            continue;
        }
#pragma unroll
        for (int n = 0; n < 3; n++) {
            if (n == 2 && lane >= OD_CHUNKS - 128) continue;
            int Y = yq - 21 + erow[n];
            Y = Y < 0 ? -Y : Y;
            Y = Y >= L.h ? 2 * L.h - 2 - Y : Y;
            Y = min(max(Y, 0), L.h - 1);
            const int X = min(max(xs + ecol[n], 0), wlim - 16);
            __builtin_amdgcn_global_load_lds((gptr_t)(plain + (__umul24((unsigned)Y, pstride) + (unsigned)X)), (lptr_t)(win0 + q * OD_WIN_BYTES + 1024 * n), 16, 0, 0);
        }
    }
    fixmask = (uint32_t)__builtin_amdgcn_readfirstlane((int)fixmask);
    // the tables' barrier behind the DMA issue (only the LDS writes above have to be complete; a wave that returned has left the barrier count)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // ---- lane constants of the two passes (independent of the keypoint)
    // [0], [1]: the 16-wide column / row tiles of one window; [2]: the paired tiles of the last 8 columns / 5 rows (blur below)
    v4i Trow[3], Tcol[2];
#pragma unroll
    for (int c = 0; c < 3; c++) Trow[c] = *reinterpret_cast<const v4i*>(c_od.trow[c][lane]);
#pragma unroll
    for (int c = 0; c < 2; c++) Tcol[c] = *reinterpret_cast<const v4i*>(c_od.tcol[c][lane]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the windows have landed
    wave_lds_fence();

    // ---- border windows: put the clamped chunks and the reflected columns right (LDS to LDS; chunk 1 is never affected: x <= w - 17)
    if (fixmask & 15u) {
#pragma unroll 1
        for (int q = 0; q < OD_KPW; q++) {
            if (!((fixmask >> q) & 1u)) continue;
            const unsigned posq = (unsigned)__builtin_amdgcn_readlane((int)kp.pos, 16 * q);
            const int xq = posq & 0xFFFF;
            const int xs = (xq - 22) & ~3;
            uint8_t* W = win0 + q * OD_WIN_BYTES;
#pragma unroll 1
            for (int j = 0; j < 3; j += 2) {
                const int X0 = xs + 16 * j, Xc = min(max(X0, 0), wlim - 16);
                if (X0 >= 0 && X0 + 16 <= wlim && X0 + 15 < L.w) continue;          // this chunk is what it should be
                // item = (row, dword of the chunk): 172 items, <= 3 per lane; every byte read first, then every dword written
                uint32_t nv[3];
#pragma unroll
                for (int it = 0; it < 3; it++) {
                    const int item = 64 * it + lane;
                    const int r = item >> 2, d = item & 3;
                    uint32_t v = 0;
                    if (item < 4 * OD_ROWS) {
#pragma unroll
                        for (int bb = 0; bb < 4; bb++) {
                            const int X = X0 + 4 * d + bb;
                            int Xr = X < 0 ? -X : (X >= L.w ? 2 * L.w - 2 - X : X);
                            Xr = min(max(Xr, 0), L.w - 1);
                            const int src = (Xr >= Xc && Xr < Xc + 16) ? 16 * j + (Xr - Xc) : min(max(Xr - xs, 0), OD_PITCH - 1);
                            v |= (uint32_t)W[r * OD_PITCH + src] << (8 * bb);
                        }
                    }
                    nv[it] = v;
                }
                wave_lds_fence();
#pragma unroll
                for (int it = 0; it < 3; it++) {
                    const int item = 64 * it + lane;
                    if (item < 4 * OD_ROWS) *reinterpret_cast<uint32_t*>(W + (item >> 2) * OD_PITCH + 16 * j + 4 * (item & 3)) = nv[it];
                }
                wave_lds_fence();
            }
        }
    }

    // ---- IC_Angle on the plain window (reference :124-151; the group's own window, rows 6 .. 36, columns cx-15 .. cx+15)
    const int xs_own = (x - 22) & ~3, cx = x - xs_own;
    const uint8_t* Wown = win0 + grp * OD_WIN_BYTES;
    int m10, m01;
    {
        const int rsub = li >> 1, hf = li & 1;
        const int boff = cx - HALF_PATCH + 16 * hf;          // first byte of the lane's 16 in its row
        const int sh = boff & 3;
        const uint32_t* rowp = reinterpret_cast<const uint32_t*>(Wown + (6 + rsub) * OD_PITCH + (boff & ~3));
        uint32_t uw[4];
#pragma unroll
        for (int d = 0; d < 4; d++) uw[d] = (uint32_t)(16 * hf + 4 * d) * 0x01010101u + 0x03020100u;      // u + 15 of the dword's four pixels
        uint32_t a_su = 0, a_si = 0, a_r = 0;
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const uint32_t* p = rowp + (8 * n) * (OD_PITCH / 4);     // row 31 (n = 3, rsub = 7) is masked, still inside the window
            uint32_t dw[5];
#pragma unroll
            for (int d = 0; d < 5; d++) dw[d] = p[d];
            const uint4 mk = *reinterpret_cast<const uint4*>(s_mask + (8 * (8 * n + rsub) + 4 * hf));
            const uint32_t mm[4] = {mk.x, mk.y, mk.z, mk.w};
            uint32_t srow = 0;
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const uint32_t Im = __builtin_amdgcn_alignbyte(dw[d + 1], dw[d], (uint32_t)sh) & mm[d];
                srow = __builtin_amdgcn_udot4(Im, 0x01010101u, srow, false);
                a_su = __builtin_amdgcn_udot4(Im, uw[d], a_su, false);
            }
            a_si += srow;
            a_r = __umul24(srow, (uint32_t)(8 * n)) + a_r;     // sum of (row - rsub) * rowsum
        }
        const int p10 = (int)a_su - HALF_PATCH * (int)a_si;
        const int p01 = (rsub - HALF_PATCH) * (int)a_si + (int)a_r;
        m10 = row16_sum(p10); m01 = row16_sum(p01);
    }
    const float angle = fast_atan2_deg((float)m01, (float)m10);
    wave_lds_fence();                                          // every patch read is done before the windows are overwritten

    // ---- the blur of the wave's windows (od_blur_windows)
    // per window (wave-uniform): where it lies, and whether its tiles take the per-lane epilogue — an edge window (H4 merge), or one whose
    // outputs straddle blur_wvec (ties-to-even columns x < wvec, half up beyond).  Idle slots copy the tie mode of the slot before them.
    int xsw[OD_KPW], yqw[OD_KPW];
    uint32_t tww[OD_KPW];
    bool genw[OD_KPW];
#pragma unroll
    for (int q = 0; q < OD_KPW; q++) {
        const unsigned posq = (unsigned)__builtin_amdgcn_readlane((int)kp.pos, 16 * q);
        xsw[q] = ((int)(posq & 0xFFFF) - 22) & ~3;
        yqw[q] = (int)(posq >> 16);
        const bool lo = xsw[q] + 4 < L.wvec, hi = xsw[q] + 40 < L.wvec;
        const bool liveq = q == 0 || k0 + q < cnt;
        tww[q] = liveq ? (lo ? 1u : 0u) : tww[q > 0 ? q - 1 : 0];
        genw[q] = liveq && (((fixmask >> (4 + q)) & 1u) || lo != hi);
    }
    od_blur_windows(win0, lane, min(cnt - k0, OD_KPW), OdWin{xsw[0], yqw[0], tww[0], genw[0]}, OdWin{xsw[1], yqw[1], tww[1], genw[1]},
                    OdWin{xsw[2], yqw[2], tww[2], genw[2]}, OdWin{xsw[3], yqw[3], tww[3], genw[3]}, L.w, L.h, L.wvec, Trow, Tcol, s_tprow + lane);
    wave_lds_fence();

    // ---- rotated BRIEF on the blurred window (:154-194)
    const float factorPI = (float)(3.14159265358979323846 / 180.f);
    float sn, cs;
    sincosf_orb(angle * factorPI, &sn, &cs);
    const float4* pat = reinterpret_cast<const float4*>(s_pat) + li;
    uint32_t mybits = 0;                                        // bit j: test li + 16 j
    {
        // Both coordinates of a point in ONE packed-fp32 instruction each step (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: IEEE single
        // precision per half, the same roundings as the scalar forms):  (x sn, x cs), (y cs, y sn), then (x sn + y cs, x cs - y sn).
        const uint8_t* ctr = Wown + 21 * OD_PITCH + cx;
        const f2v SC = {sn, cs};
        auto rotate = [&](f2v pt) -> f2v {                      // (x, y) -> (row offset, column offset), unrounded
            f2v m1, r;
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(m1) : "v"(pt), "v"(SC));                  // (y cs, y sn)
            if (FMA) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(pt), "v"(SC), "v"(m1));   // fma(x, sn, y cs), fma(x, cs, -(y sn))
            else {
                f2v m0;
                asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(m0) : "v"(pt), "v"(SC));              // (x sn, x cs)
                asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(m0), "v"(m1));                               // (x sn + y cs, x cs - y sn)
            }
            return r;
        };
        // cvRound (ties to even) by the magic constant: for |f| < 2^22, f + 1.5 * 2^23 rounds to the integer nearest f (ties to even, the
        // default mode) and its bit pattern is 0x4B400000 + that integer.  iy * pitch + ix is then ONE 24-bit multiply-add on the bit patterns
        // (the low 24 bits of the first are 0x400000 + iy); the constant it drags along is taken off the base address once.
        f2v MAGIC = {12582912.0f, 12582912.0f};
        asm("" : "+v"(MAGIC));                                  // in a VGPR pair: as an SGPR pair with op_sel_hi:[1,0] (what hipcc 7.2 emits for the splat) the packed add gave wrong sums
        const uint32_t ctr_a = (uint32_t)(uintptr_t)(lptr_t)ctr - (uint32_t)(OD_PITCH * 0x400000 + 0x4B400000);
        typedef const uint8_t __attribute__((address_space(3))) * lbyte_t;
#pragma unroll
        for (int j = 15; j >= 0; j--) {                       // downwards: the bits are shifted in from the bottom, test li + 16 j ends at bit j
            const float4 P = pat[16 * j];
            f2v r0 = rotate((f2v){P.x, P.y}), r1 = rotate((f2v){P.z, P.w});
            r0 = r0 + MAGIC;                                    // (v_pk_add_f32)
            r1 = r1 + MAGIC;
            // (the elements go through scalar temporaries: hipcc 7.2 folds __builtin_bit_cast(int, vec.y) of a vector ELEMENT expression to element 0 —
            //  `mad24(bits(r.x), 48, bits(r.x))` came out of the direct form; tools/microbench/bitcast_vector_element.hip)
            const float r0y = r0.x, r0x = r0.y, r1y = r1.x, r1x = r1.y;
            const uint32_t o0 = (uint32_t)(__mul24(float_bits(r0y), OD_PITCH) + float_bits(r0x));
            const uint32_t o1 = (uint32_t)(__mul24(float_bits(r1y), OD_PITCH) + float_bits(r1x));
            const uint32_t v0 = *(lbyte_t)(uintptr_t)(ctr_a + o0), v1 = *(lbyte_t)(uintptr_t)(ctr_a + o1);
            // mybits = 2 mybits + (v0 < v1): the comparison's carry straight into the add (two instructions instead of compare, select, or)
            asm("v_cmp_lt_u32_e32 vcc, %1, %2\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(mybits) : "v"(v0), "v"(v1) : "vcc");
        }
    }
    // 16 x 16 bit-matrix transpose inside the group (ds_swizzle butterflies, as k_describe)
    uint32_t half = mybits;
    auto stage = [&](auto S) {
        constexpr int s = decltype(S)::value;
        constexpr uint32_t M0 = s == 8 ? 0x00FFu : s == 4 ? 0x0F0Fu : s == 2 ? 0x3333u : 0x5555u;
        const bool hi = (li & s) != 0;
        const uint32_t yv = (uint32_t)__builtin_amdgcn_ds_swizzle((int)half, (s << 10) | 0x1F);        // lane ^ s
        const uint32_t ysh = hi ? (yv >> s) : (yv << s);
        const uint32_t mk = hi ? (~M0 & 0xFFFFu) : M0;
        half = (half & mk) | (ysh & ~mk & 0xFFFFu);
    };
    stage(std::integral_constant<int, 8>{}); stage(std::integral_constant<int, 4>{});
    stage(std::integral_constant<int, 2>{}); stage(std::integral_constant<int, 1>{});
    if (!valid) return;
    const int out_idx = out_base + k;
    reinterpret_cast<uint16_t*>(b.out_desc + ((long long)frame * b.cap + out_idx) * 32)[li] = (uint16_t)half;   // lane li stores halfword li
    if (li == 0) {
        orbx_keypoint o;
        o.x = (float)x; o.y = (float)y;
        if (level != 0) { o.x = o.x * L.scale; o.y = o.y * L.scale; }   // :769-775
        o.size = L.kp_size;
        o.angle = angle;
        o.response = kp.resp;
        o.octave = level;
        o.class_id = -1;
        b.out_kps[(long long)frame * b.cap + out_idx] = o;
    }
}
// four waves per SIMD (four workgroups per CU: what the LDS allows) need <= 128 VGPRs; without the bound the paired blur's scheduler takes 130
template <bool FMA>
__global__ __launch_bounds__(OD_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void k_describe_od(Batch b) { k_describe_od_body<FMA, false>(b); }
template <bool FMA>
__global__ __launch_bounds__(OD_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4))) void k_describe_od_gather(Batch b) { k_describe_od_body<FMA, true>(b); }

// every level must offer 48 readable bytes per row and be at least 64 px wide (the border fix-up's case analysis), rows single-reflect
bool describe_od_supported(const Batch& b, const HostGeom& hg) {
    const DevGeom& g = hg.g;
    for (int l = 0; l < g.nlevels; l++)
        if (g.lv[l].w < 64 || g.lv[l].h < 44) return false;
    const long long wlim0 = std::min<long long>(level0_min_stride(b), (g.lv[0].w + 15) & ~15);     // (gather form: the narrowest frame)
    return wlim0 >= 64 && wlim0 >= g.lv[0].w;
}

// (launch_describe's on-demand half: `variant` is its DV_OD | ... choice)
int launch_describe_od(const Batch& b, const HostGeom& hg, hipStream_t stream, int variant) {
    const DevGeom& g = hg.g;
    const dim3 grid(frame_item_blocks(b, (g.nquads + OD_WAVES - 1) / OD_WAVES)), block(OD_WAVES * 64);
    switch (variant) {
        case DV_OD: hipLaunchKernelGGL(k_describe_od<false>, grid, block, 0, stream, b); break;
        case DV_OD | DV_FMA: hipLaunchKernelGGL(k_describe_od<true>, grid, block, 0, stream, b); break;
        case DV_OD | DV_GATHER: hipLaunchKernelGGL(k_describe_od_gather<false>, grid, block, 0, stream, b); break;
        case DV_OD | DV_GATHER | DV_FMA: hipLaunchKernelGGL(k_describe_od_gather<true>, grid, block, 0, stream, b); break;
        default: return ORBX_ERR_ARG;
    }
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

// orbx_debug_eval_blur_window: od_blur_windows on caller-supplied windows, four per wave as in the kernel.  The windows lie at level column 0 /
// row 18 of a level far larger than they are: nothing is outside it, and the general (per-lane) epilogue sees the one tie mode everywhere.
__global__ __launch_bounds__(64) void k_eval_blur_window(const uint32_t* win, uint8_t* out, int n, int ties_even, int general) {
    __shared__ __attribute__((aligned(16))) uint32_t s_w[(OD_KPW * OD_WIN_BYTES + OD_TAIL) / 4];
    const int lane = threadIdx.x, q0 = blockIdx.x * OD_KPW, nlive = min(n - q0, OD_KPW);
    for (int i = lane; i < (OD_KPW * OD_WIN_BYTES + OD_TAIL) / 4; i += 64)
        s_w[i] = i < nlive * (OD_WIN_BYTES / 4) ? win[(size_t)q0 * (OD_WIN_BYTES / 4) + i] : 0u;
    __shared__ __attribute__((aligned(16))) v4i s_tprow[2 * 64];
    v4i Trow[3], Tcol[2];
#pragma unroll
    for (int c = 0; c < 3; c++) Trow[c] = *reinterpret_cast<const v4i*>(c_od.trow[c][lane]);
#pragma unroll
    for (int c = 0; c < 2; c++) { Tcol[c] = *reinterpret_cast<const v4i*>(c_od.tcol[c][lane]); s_tprow[64 * c + lane] = *reinterpret_cast<const v4i*>(c_od.tcol[2 + c][lane]); }
    wave_lds_fence();
    const int big = 1 << 20;
    const OdWin w = {0, 18, ties_even ? 1u : 0u, general != 0};
    uint8_t* W = reinterpret_cast<uint8_t*>(s_w);
    od_blur_windows(W, lane, nlive, w, w, w, w, big, big, ties_even ? big : 0, Trow, Tcol, s_tprow + lane);
    wave_lds_fence();
    for (int i = lane; i < nlive * (37 * 40); i += 64) {
        const int q = i / (37 * 40), r = (i - q * (37 * 40)) / 40, c = i % 40;
        out[(size_t)q0 * (37 * 40) + i] = W[q * OD_WIN_BYTES + (r + 3) * OD_PITCH + c + 4];
    }
}
int launch_eval_blur_window(const uint8_t* win, uint8_t* out, int n, int ties_even, int general) {
    static_assert(OD_WIN_BYTES % 4 == 0 && OD_TAIL % 4 == 0, "the windows are copied by dwords");
    hipLaunchKernelGGL(k_eval_blur_window, dim3((n + OD_KPW - 1) / OD_KPW), dim3(64), 0, 0, reinterpret_cast<const uint32_t*>(win), out, n, ties_even, general);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

}  // namespace orbx
