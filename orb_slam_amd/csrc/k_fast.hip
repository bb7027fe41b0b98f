// FAST-9 + cell-local NMS + raster-ordered cell lists for gfx950 (cv::FAST(cell, th, true) per grid cell with the threshold-7 fallback,
// reference src/ORBextractor.cc:599-614): k_fast_cells (one workgroup per row band of a grid cell) and k_fast_blur (the same beside the blur's
// strips in one launch: launch groups too small to fill the chip).
#include <algorithm>
#include <type_traits>

#include "orbx_device.h"
#include "orbx_launch.h"
#include "k_blur_strip.h"

namespace orbx {

__device__ __forceinline__ int fast_pair_test(const uint8_t* c, int S, int v, int t) {
    // ring offsets k=0..15 (dx,dy): (0,3)(1,3)(2,2)(3,1)(3,0)(3,-1)(2,-2)(1,-3)(0,-3)(-1,-3)(-2,-2)(-3,-1)(-3,0)(-3,1)(-2,2)(-1,3)
    const int x0 = c[3 * S], x1 = c[3 * S + 1], x2 = c[2 * S + 2], x3 = c[S + 3], x4 = c[3], x5 = c[-S + 3], x6 = c[-2 * S + 2], x7 = c[-3 * S + 1];
    const int x8 = c[-3 * S], x9 = c[-3 * S - 1], x10 = c[-2 * S - 2], x11 = c[-S - 3], x12 = c[-3], x13 = c[S - 3], x14 = c[2 * S - 2], x15 = c[3 * S - 1];
    // a dark 9-arc contains one pixel of every opposite pair, so max_k min(pair) < v - t is necessary (bright: mirrored)
    const int a = imax3(imax3(imin(x0, x8), imin(x1, x9), imin(x2, x10)), imax3(imin(x3, x11), imin(x4, x12), imin(x5, x13)), imax(imin(x6, x14), imin(x7, x15)));
    const int bq = imin3(imin3(imax(x0, x8), imax(x1, x9), imax(x2, x10)), imin3(imax(x3, x11), imax(x4, x12), imax(x5, x13)), imin(imax(x6, x14), imax(x7, x15)));
    return (int)(v - a > t) | (int)(bq - v > t);
}

// B's arithmetic: the exact score on packed halves (orb_math.h: fast9_score_pk_with, which fixes the pairing and the swap pattern of every
// step).  Word j holds ring pixels j and j + 8 in its 16-bit halves; a byte in a half is the f16 denormal 0x00XX, positive f16 order is integer
// order and the kernels keep f16 denormals, so one v_pk_maximum3_f16 / v_pk_minimum3_f16 is the integer max3 / min3 of two ring positions
// at once, and op_sel supplies the swapped halves the circular indexing needs: 42 three-input instructions per pass where the unpacked
// form (rounds 1-7: v_max3_u32 / v_min3_u32 on one position each) took 80.  tools/microbench/valu_rate2.hip checks that the two opcodes return
// byte-valued halves bit for bit (all 2^24 triples per half and swap pattern) and prices them; tests/test_gpu_fast_score_pk.py holds this
// against fast9_score through orbx_debug_eval_score.
struct PkHalvesF16 {
#define ORBX_PK3(OPC, SEL) asm(OPC " %0, %1, %2, %3" SEL : "=v"(o) : "v"(a), "v"(b), "v"(c))
    static __device__ __forceinline__ uint32_t max3(uint32_t a, uint32_t b, uint32_t c, int form) {
        uint32_t o;
        if (form == PK_SWAP_BC) ORBX_PK3("v_pk_maximum3_f16", " op_sel:[0,1,1] op_sel_hi:[1,0,0]");
        else if (form == PK_SWAP_C) ORBX_PK3("v_pk_maximum3_f16", " op_sel:[0,0,1] op_sel_hi:[1,1,0]");
        else ORBX_PK3("v_pk_maximum3_f16", "");
        return o;
    }
    static __device__ __forceinline__ uint32_t min3(uint32_t a, uint32_t b, uint32_t c, int form) {
        uint32_t o;
        if (form == PK_SWAP_BC) ORBX_PK3("v_pk_minimum3_f16", " op_sel:[0,1,1] op_sel_hi:[1,0,0]");
        else if (form == PK_SWAP_C) ORBX_PK3("v_pk_minimum3_f16", " op_sel:[0,0,1] op_sel_hi:[1,1,0]");
        else ORBX_PK3("v_pk_minimum3_f16", "");
        return o;
    }
#undef ORBX_PK3
};
// the ring of the pixel at c as packed words: X[j] = ring j | ring (j + 8) << 16 (ring offsets: fast_pair_test above)
__device__ __forceinline__ void fast_ring_pk(const uint8_t* c, int S, uint32_t X[8]) {
    // all sixteen reads first, in the order the words are put together, then the words: left to itself the scheduler puts the first word
    // together after four reads, behind a full wait, and the pass pays two LDS round trips (the barrier pins the order, not the waits)
    const uint32_t x0 = c[3 * S], x8 = c[-3 * S], x1 = c[3 * S + 1], x9 = c[-3 * S - 1], x2 = c[2 * S + 2], x10 = c[-2 * S - 2], x3 = c[S + 3], x11 = c[-S - 3];
    const uint32_t x4 = c[3], x12 = c[-3], x5 = c[-S + 3], x13 = c[S - 3], x6 = c[-2 * S + 2], x14 = c[2 * S - 2], x7 = c[-3 * S + 1], x15 = c[3 * S - 1];
    __builtin_amdgcn_sched_barrier(0);
    X[0] = x0 | x8 << 16; X[1] = x1 | x9 << 16; X[2] = x2 | x10 << 16; X[3] = x3 | x11 << 16;
    X[4] = x4 | x12 << 16; X[5] = x5 | x13 << 16; X[6] = x6 | x14 << 16; X[7] = x7 | x15 << 16;
}
__device__ __forceinline__ int fast_score_pk(const uint8_t* c, int S, int v, int tmin) {
    uint32_t X[8];
    fast_ring_pk(c, S, X);
    return fast9_score_pk_with<PkHalvesF16>(X, v, tmin);   // == OpenCV cornerScore for every corner
}

// ------------------------------------------------------------------------------------ FAST + NMS + cell lists
// One workgroup = one grid cell of one level of one frame (or one row band of a big cell) — the unit the reference
// calls cv::FAST on (src/ORBextractor.cc:599-614).  Because the NMS of cv::FAST never looks outside the cell view, a
// cell-native workgroup needs no score halo towards other cells, no survivor plane in HBM and no compaction pass.
// One score pass at min(fastTh, 7) serves the normal threshold and the reference's threshold-7 fallback (score >= t <=> corner at t).
// Phases: stage the band (+3 halo) in LDS -> A1 dense compass test -> A2 opposite-pair test (sparse) -> B exact score (sparse)
// -> N 3x3 strict NMS -> raster-ordered list with its counts at fastTh and at 7.  (Round 2 form; the round-1 kernel — flat pixel
// index per lane, block-wide queues with a barrier per phase — took 1.51 ms per 1024 VGA frames, this one 1.11.)
//   * everything is addressed by the pixel's BYTE OFFSET q inside the staged LDS image (pitch S): the score plane has the
//     image's layout, so ring / neighbour addresses are q +- dy*S + dx with no division anywhere in the dense or sparse phases;
//   * A1 is SWAR: a lane tests 4 horizontally adjacent pixels (one aligned dword) per step, on the bytes as they lie, with
//     v_lerp_u8 (four byte averages (a + b + (c & 1)) >> 1 per instruction, nothing carries between bytes): h = avg(x, ~v, t & 1)
//     is (255 + x - v + (t & 1)) >> 1, and bit 7 of avg(h, K) against two constants of the threshold says "x > v + t" and
//     "x <= v - t" (compass4_dev below; rounds 2-6 unpacked the bytes into 16-bit fields and compared by biased adds: 47
//     instructions per step against 18).  Rule: a 9-arc of the 16-ring contains ring 0 or 8 AND ring 4 or 12, so a corner needs
//     (N | S) & (E | W) beyond the threshold with one polarity — a necessary condition, and the filter is a superset of it by the
//     one difference v - x == t.  (gfx950 serves unaligned ds_read_b32, but slowly: reading the E / W dwords that way instead
//     of two v_alignbyte cost +44 % on the kernel);
//   * flagged dwords are queued per WAVE (ballot + mbcnt, no atomics), expanded to pixels, pair-tested and scored by the same
//     wave in full-wave slices: no workgroup barrier between staging and the NMS;
//   * every wave remembers the pixels it gave a score; the NMS visits those (a dense sweep over the score plane only where a
//     wave's list overflowed: noise-like bands), survivors set bits in a q-space bitmask, the raster-ordered list comes from
//     the same chunk scan as before.
// Round 3 (1.12 -> 0.99 ms per 1024 VGA frames).  Cut short phase by phase the kernel costs staging 0.33 + dense phase 0.34 + drain
// 0.28 + NMS 0.06 + list 0.07 ms, and with its dynamic LDS padded 1.06 / 1.15 / 1.30 / 1.56 ms at 6 / 5 / 4 / 3 workgroups per CU: it is
// bound by latency at the occupancy its LDS allows, not by instruction issue alone.  Hence: the queues are as small as their
// invariants allow (7 workgroups per CU on VGA grids), the staging moves 16 bytes per lane, the drain scores both remainders in
// one pass without the pair test, the list output scans with DPP adds instead of ds_bpermute and counts by ballot.  (NOTES.md 8.2b;
// what did NOT help: pooling the waves' remainders behind extra barriers, an L2 prefetch of a later band, smaller bands.)
// The exact score (phase B) runs on packed halves: two ring positions per word, one v_pk_maximum3_f16 / v_pk_minimum3_f16 per step, 42 steps
// plus 8 v_lshl_or_b32 where the unpacked form took 80 (fast_score_pk above; NOTES.md 8.2e).  Every wave runs it at least once, in the
// drain.  What it gains depends on how close to its issue limit the kernel runs on the box at hand: -5.8 % of the kernel where the parent
// took 0.786 ms per 1024 VGA frames, nothing where it took 0.726.  (What did NOT help: assembling the halves by ds_read_u8_d16 / _d16_hi,
// which do not keep the other half on this device; seven reads at byte addresses in place of the sixteen byte reads, +29 %.)
struct FastHdr { int n_hi, n_lo, overflow, pad1; int wsum[8]; int pad2[4]; };
static_assert(sizeof(FastHdr) == 64, "LDS carve");

__device__ __forceinline__ int lane_rank(unsigned long long m) {   // number of set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// A1's arithmetic: the compass test of four packed pixels by byte averages (orb_math.h: avg_u8, compass_kb / compass_kd; one v_lerp_u8
// per avg4_u8 of the host form compass4_flags, which tests/test_gpu_fast_compass.py holds this against): 1 v_not + 12 v_lerp_u8 + 5
// logic ops per dword-step where the 16-bit SWAR form of rounds 2-6 took 47.  The dark side passes the one extra difference
// v - x == t (orb_math.h says why).  The exact form (four more first-level averages with the other rounding bit, 16 v_lerp_u8) was
// measured beside this one and lost on the headline and every stream but S-lowtex (NOTES.md 8.2d): the extra flags cost less than
// the four instructions.
struct CompassK { uint32_t R, KB, KD; };      // r, kb, kd in every byte (wave-uniform)
__device__ __forceinline__ CompassK compass_consts(int t) {      // (t > 254: the filter of 254, see orb_math.h; the exact score rejects what it passes)
    CompassK k;
    k.R = (uint32_t)compass_r(t) * 0x01010101u;
    k.KB = (uint32_t)compass_kb(t) * 0x01010101u;
    k.KD = (uint32_t)compass_kd(t) * 0x01010101u;
    return k;
}
__device__ __forceinline__ uint32_t compass4_dev(uint32_t C, uint32_t E, uint32_t W, uint32_t Nn, uint32_t Ss, const CompassK& k) {
    const uint32_t nc = ~C;
    const uint32_t hN = __builtin_amdgcn_lerp(Nn, nc, k.R), hS = __builtin_amdgcn_lerp(Ss, nc, k.R);
    const uint32_t hE = __builtin_amdgcn_lerp(E, nc, k.R), hW = __builtin_amdgcn_lerp(W, nc, k.R);
    const uint32_t br = (__builtin_amdgcn_lerp(hN, k.KB, 0u) | __builtin_amdgcn_lerp(hS, k.KB, 0u)) &
                        (__builtin_amdgcn_lerp(hE, k.KB, 0u) | __builtin_amdgcn_lerp(hW, k.KB, 0u));
    const uint32_t dN = __builtin_amdgcn_lerp(hN, k.KD, 0u), dS = __builtin_amdgcn_lerp(hS, k.KD, 0u);
    const uint32_t dE = __builtin_amdgcn_lerp(hE, k.KD, 0u), dW = __builtin_amdgcn_lerp(hW, k.KD, 0u);
    return (br | ~((dN & dS) | (dE & dW))) & 0x80808080u;
}
// (diagnostics, beside k_eval_math: the device compass test on caller-supplied dwords)
__global__ void k_eval_compass(const uint32_t* c, const uint32_t* e, const uint32_t* w, const uint32_t* nn, const uint32_t* ss, uint32_t* out, int n, int t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = compass4_dev(c[i], e[i], w[i], nn[i], ss[i], compass_consts(t));
}
int launch_eval_compass(const uint32_t* c, const uint32_t* e, const uint32_t* w, const uint32_t* nn, const uint32_t* ss, uint32_t* out, int n, int t) {
    hipLaunchKernelGGL(k_eval_compass, dim3((n + 255) / 256), dim3(256), 0, 0, c, e, w, nn, ss, out, n, t);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

// (diagnostics: the kernels' exact score and pair test on caller-supplied rings.  Every lane lays its ring out as a 7 x 7 patch of pitch 8 in
// LDS and calls fast_score_pk / fast_pair_test on it as phases B and A2 do on the staged band, ring reads included.)
__global__ __launch_bounds__(256) void k_eval_score(const uint8_t* centre, const uint8_t* ring16, uint8_t* score, uint8_t* pair, int n, int tmin) {
    constexpr int PS = 8, PATCH = 7 * PS;
    constexpr int RDX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1}, RDY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    __shared__ uint8_t s_patch[256 * PATCH];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint8_t* c = s_patch + threadIdx.x * PATCH + 3 * PS + 3;
    c[0] = centre[i];
#pragma unroll
    for (int k = 0; k < 16; k++) c[RDY[k] * PS + RDX[k]] = ring16[16ll * i + k];
    score[i] = (uint8_t)fast_score_pk(c, PS, c[0], tmin);      // (a lane reads its own patch only: no barrier)
    pair[i] = (uint8_t)fast_pair_test(c, PS, c[0], tmin);
}
int launch_eval_score(const uint8_t* centre, const uint8_t* ring16, uint8_t* score, uint8_t* pair, int n, int tmin) {
    hipLaunchKernelGGL(k_eval_score, dim3((n + 255) / 256), dim3(256), 0, 0, centre, ring16, score, pair, n, tmin);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

template <bool ALIGNED, int NT, int PPT, bool GATHER = false>
__device__ __forceinline__ void fast_band_task(const Batch& b, int frame, int item, uint8_t* smem) {
    constexpr int NW = NT / 64;
    static_assert((NW & (NW - 1)) == 0, "wave roles rotate modulo NW");
    constexpr int Q0CAP = fast_q0cap(PPT), Q1CAP = FAST_Q1CAP, Q2CAP = FAST_Q2CAP, Q3CAP = FAST_Q3CAP;
    constexpr int WQ_BYTES = fast_wave_queue_bytes(PPT);
    const DevGeom& g = b.g;
    const BandGeom bg = b.bands[item];
    const int level = bg.level;
    const LevelGeom& L = g.lv[level];
    // Wave roles rotate with the band index.  The tails of the task are wave-0 heavy (a VGA cell's survivor list is <= 70 chunks: wave 0
    // writes all of it; tid 0 closes the band), and the waves of a 4-wave workgroup land on the CU's four SIMDs in order, so without
    // the rotation one SIMD of every CU carried all of that.  Every use of wave / tid below is work assignment only.
    const int lane = threadIdx.x & 63, wave = ORBX_FAST_ROTATE ? (wave_id() + item) & (NW - 1) : wave_id(), tid = wave * 64 + lane;
    const int cw = bg.x1 - bg.x0 + 1, ch = bg.ey1 - bg.ey0 + 1;      // scored rectangle: own rows + halo rows towards sibling bands
    CellState* cst = b.cstate + (long long)frame * g.nbands_total + item;
    // Fallback hint (round 6: per FRAME SLOT): how many launch groups in a row THIS band of THIS slot of the launch group ended with <= 3
    // survivors@fastTh.  It lives in the upper bits of CellState::thr, which the same work item of the previous launch group left behind: one
    // load in front of the band, no store of its own (round 5 kept one table per handle, written by frame 0 and read by every frame: a launch
    // group that mixes streams — several cameras, a handle reused across sequences — inherited frame 0's texture class).
    const int hint = b.fallback_hint ? (int)((uint32_t)cst->thr >> 8) : 0;
    if (cw <= 0 || ch <= 0) {
        if (tid == 0) { CellState st; st.n_all = 0; st.n_hi = 0; st.n_lo = 0; st.thr = g.tmin; *cst = st; }
        return;
    }
    const int own_lo = bg.y0 - bg.ey0, own_hi = bg.y1 - bg.ey0;
    // staged image: rows ey0-3 .. ey1+3, columns from the dword-aligned start at or left of x0-3; pixel (x, y) of the band
    // (relative to (x0, ey0)) lives at byte offset q = (y + 3) * S + x + xoff + 3
    const int gxb = (bg.x0 - 3) & ~3;
    const int xoff = (bg.x0 - 3) - gxb;
    const int nd = fast_row_dwords(xoff, cw);
    const int S = nd * 4;
    const int x_first = xoff + 3;
    const int nrows = ch + 6;
    // LDS carve: header | survivor bit masks | per-wave queues | image | scores (image layout)
    FastHdr* hdr = reinterpret_cast<FastHdr*>(smem);
    unsigned long long* cmask = reinterpret_cast<unsigned long long*>(smem + sizeof(FastHdr));
    uint8_t* wq = smem + sizeof(FastHdr) + g.fast_max_chunks * 8 + wave * WQ_BYTES;
    uint32_t* q0 = reinterpret_cast<uint32_t*>(wq);
    uint16_t* q1 = reinterpret_cast<uint16_t*>(wq + Q0CAP * 4);
    uint16_t* q2 = q1 + Q1CAP;
    uint16_t* q3 = q2 + Q2CAP;
    uint8_t* s_img = smem + sizeof(FastHdr) + g.fast_max_chunks * 8 + NW * WQ_BYTES;
    uint8_t* s_sc = s_img + g.fast_max_img;
    const int q_own_lo = (3 + own_lo) * S, q_own_hi = (3 + own_hi + 1) * S;      // byte offsets of the band's own rows
    const int nchunks = (q_own_hi - q_own_lo + 63) >> 6;
    long long stride64;
    const uint8_t* src = plain_plane<GATHER>(b, L, level, frame, stride64);
    auto clear_lds = [&]() {
        for (int i = tid; i < ((nrows * S + 15) >> 4); i += NT) reinterpret_cast<uint4*>(s_sc)[i] = make_uint4(0, 0, 0, 0);
        if (tid < (int)(sizeof(FastHdr) / 4)) reinterpret_cast<int*>(hdr)[tid] = 0;
        for (int i = tid; i < nchunks; i += NT) cmask[i] = 0ull;
    };
    if (ALIGNED) {
        // LDS-DMA staging (global_load_lds_dwordx4: lane i's 16 bytes land at M0 + 16 i).  No VGPRs for the data, no ds_write; a wave
        // issues its few instructions back to back and waits once.  (Round 2 moved a dword per lane, one instruction per row piece:
        // 17 instructions per wave for a VGA band against 3 now, 1.00 -> 0.97 ms per 1024 frames.)
        typedef const void __attribute__((address_space(1))) * gptr_t;
        typedef void __attribute__((address_space(3))) * lptr_t;
        const uint8_t* src0 = src + (long long)(bg.ey0 - 3) * stride64 + gxb;
        clear_lds();      // first: the compiler orders every LDS write behind outstanding LDS-DMA loads (vmcnt(0)), so behind them it would wait for the band
        // The band's rows are nd / 4 chunks of 16 bytes each, the chunks of all rows one flat list q (LDS offset 16 q, row q / cpr,
        // chunk q % cpr); a wave instruction moves 64 consecutive chunks, i.e. several whole rows of a VGA-class band.  Global
        // addresses are dword-aligned only (the band starts at the dword at or left of x0 - 3), which the x4 load accepts.
        {
            const int cpr = nd >> 2, nchunks16 = nrows * cpr;
            const float inv_cpr = bg.inv_cpr;
            for (int q0 = 64 * wave; q0 < nchunks16; q0 += 64 * NW) {
                const int q = q0 + lane;
                int r, c;
                split_px(imin(q, nchunks16 - 1), cpr, inv_cpr, r, c);
                const uint8_t* ga = src0 + (long long)r * stride64 + 16 * c;
                if (q < nchunks16) __builtin_amdgcn_global_load_lds((gptr_t)ga, (lptr_t)(s_img + 16 * q0), 16, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the DMA writes of THIS wave have landed; the barrier below covers the others
    } else {
        // unaligned frames (level 0 only): flattened (row, dword) items assembled from byte loads, 8 in flight per lane
        const int total = nrows * nd;
        const float inv_nd0 = bg.inv_nd;
        const uint8_t* src0 = src + (long long)(bg.ey0 - 3) * stride64 + gxb;
        const int xm = L.w - 1 - gxb;   // never read past the row end
        for (int i0 = 0; i0 < total; i0 += NT * 8) {
            uint32_t v4[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = i0 + k * NT + tid;
                v4[k] = 0;
                if (i < total) {
                    int r, d;
                    split_px(i, nd, inv_nd0, r, d);
                    const uint8_t* row = src0 + (long long)r * stride64;
                    v4[k] = (uint32_t)row[imin(4 * d, xm)] | (uint32_t)row[imin(4 * d + 1, xm)] << 8 | (uint32_t)row[imin(4 * d + 2, xm)] << 16 |
                            (uint32_t)row[imin(4 * d + 3, xm)] << 24;
                }
            }
            if (i0 == 0) clear_lds();
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = i0 + k * NT + tid;
                if (i < total) reinterpret_cast<uint32_t*>(s_img)[i] = v4[k];
            }
        }
    }
    __syncthreads();

    // Threshold of the current pass (round 4).  The band is first scored at fastTh: survivors@fastTh = survivors@7 intersected with
    // {score >= fastTh} (a neighbour scoring below fastTh can never block a pixel scoring at least fastTh), so a band that keeps
    // more than 3 of them proves that its cell has more than 3 and never takes the reference's threshold-7 fallback (:609-614): its
    // list at fastTh is all the later stages read.  Only a band with <= 3 survivors@fastTh is scored again at 7 (below).  On textured
    // input (corners@7 several times corners@fastTh) the pair test, score, NMS and list phases shrink by that factor; on the S-blocks
    // stream 3 % of the bands take the second pass.  fastTh <= 7: one pass at fastTh serves both (g.tmin = fastTh).
    // Fallback hint (round 5; per frame slot since round 6, see above): a band that needed the second pass in FAST_HINT_RUN launch groups in a row starts at 7
    // (low-texture streams: every band would otherwise run twice, S-lowtex +35 % on this kernel).  A wrong hint costs one pass at 7
    // instead of one at fastTh, never a wrong result: CellState::thr tells the later stages what the list was made at.
    constexpr int FAST_HINT_RUN = 6;
    int tmin = ORBX_FAST_TWO_PASS ? (hint >= FAST_HINT_RUN && g.fast_th > 7 ? 7 : g.fast_th) : g.tmin;
    const float inv_nd = bg.inv_nd;                // (1 / nd, 1 / S, 1 / cpr come with the band: BandGeom)
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;          // fill of this wave's queues (wave-uniform)

    // B: exact FAST score of <= 64 queued pixels (`on` lanes hold one each); scored corners are remembered in q3
    auto score_vals = [&](bool on, int p) {
        int sc = 0;
        if (on) {
            const uint8_t* c = s_img + p;
            sc = fast_score_pk(c, S, c[0], tmin);
            s_sc[p] = (uint8_t)sc;
        }
        const unsigned long long mk = __ballot(sc != 0);
        if (mk) {
            const int add = __popcll(mk);
            if (n3 + add <= Q3CAP) { if (sc) q3[n3 + lane_rank(mk)] = (uint16_t)p; }
            n3 += add;                              // beyond Q3CAP: the band takes the dense NMS sweep
        }
    };
    auto score_step = [&](const uint16_t* q, int m) { score_vals(lane < m, lane < m ? (int)q[lane] : 0); };
    // A2: OpenCV's opposite-pair pre-test of m <= 64 queued pixels; survivors go to q2, which is scored whenever it holds a full wave
    auto pair_step = [&](const uint16_t* q, int m) {
        int pass = 0, p = 0;
        if (lane < m) {
            p = q[lane];
            const uint8_t* c = s_img + p;
            pass = fast_pair_test(c, S, c[0], tmin);
        }
        const unsigned long long mk = __ballot(pass);
        if (mk) {
            if (pass) q2[n2 + lane_rank(mk)] = (uint16_t)p;
            n2 += __popcll(mk);
            if (n2 >= 64) { n2 -= 64; score_step(q2 + n2, 64); }
        }
    };
    // expansion of m <= 64 flagged dwords into pixel offsets (pixels of the alignment / halo columns are dropped here)
    auto expand_step = [&](const uint32_t* q, int m) {
        uint32_t e = 0;
        if (lane < m) e = q[lane];
        const int idx = (int)((e & 0x7Fu) | ((e >> 1) & 0x3F80u));          // the 14-bit dword index lies around flag bit 7 (see the push in `round`)
        int r, d;
        split_px(idx, nd, inv_nd, r, d);
        const int col0 = 4 * d - x_first;                                   // band column of the dword's first pixel
        // flag bits: pixel j -> bit 8 j + 7
        const int f[4] = {(int)((e >> 7) & 1u) & (int)((unsigned)col0 < (unsigned)cw), (int)((e >> 15) & 1u) & (int)((unsigned)(col0 + 1) < (unsigned)cw),
                          (int)((e >> 23) & 1u) & (int)((unsigned)(col0 + 2) < (unsigned)cw), (int)((e >> 31) & 1u) & (int)((unsigned)(col0 + 3) < (unsigned)cw)};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned long long mk = __ballot(f[j]);
            if (mk) {
                if (f[j]) q1[n1 + lane_rank(mk)] = (uint16_t)(4 * idx + j);
                n1 += __popcll(mk);
            }
            if (j & 1) while (n1 >= 64) { n1 -= 64; pair_step(q1 + n1, 64); }      // after two pixels per dword: q1 never holds more than 63 + 128
        }
    };

    // A1: compass test by byte averages, 4 pixels per lane and step (see the header of this section; constants: orb_math.h)
    CompassK K = compass_consts(tmin);
    auto compass4 = [&](uint32_t C, uint32_t E, uint32_t W, uint32_t Nn, uint32_t Ss) -> uint32_t { return compass4_dev(C, E, W, Nn, Ss, K); };
    const int i_begin = 3 * nd, i_end = (ch + 3) * nd;          // dwords of the scored rows (all columns of the staged image)
    constexpr int RG = NW * 64 * PPT;                            // dwords per round of the workgroup
    auto round = [&](auto full_c, int base) {
        constexpr bool FULL = decltype(full_c)::value;          // every lane's PPT dwords lie below i_end: constant LDS offsets, no masking
        const int i0 = base + wave * 64 + lane;
        uint32_t C[PPT], E[PPT], W[PPT], Nn[PPT], Ss[PPT];
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const int ik = FULL ? i0 + k * NW * 64 : imin(i0 + k * NW * 64, i_end - 1);
            const uint8_t* pk = s_img + 4 * ik;
            C[k] = *reinterpret_cast<const uint32_t*>(pk);
            E[k] = __builtin_amdgcn_alignbyte(*reinterpret_cast<const uint32_t*>(pk + 4), C[k], 3);   // pixels x+3 .. x+6
            W[k] = __builtin_amdgcn_alignbyte(C[k], *reinterpret_cast<const uint32_t*>(pk - 4), 1);   // pixels x-3 .. x
            Nn[k] = *reinterpret_cast<const uint32_t*>(pk - 3 * S);
            Ss[k] = *reinterpret_cast<const uint32_t*>(pk + 3 * S);
        }
#pragma unroll
        for (int k = 0; k < PPT; k++) {
            const int i = i0 + k * NW * 64;
            uint32_t Q = compass4(C[k], E[k], W[k], Nn[k], Ss[k]);
            if (!FULL && i >= i_end) Q = 0;
            const unsigned long long mk = __ballot(Q != 0);
            if (mk) {
                if (Q) q0[n0 + lane_rank(mk)] = Q | (uint32_t)(i + (i & ~0x7F));      // flags at bits 7 / 15 / 23 / 31, the index (< 2^14) in bits 0-6 and 8-14
                n0 += __popcll(mk);
                if (n0 >= 64) { n0 -= 64; expand_step(q0 + n0, 64); }          // q0 never holds more than 63 + 64
            }
        }
    };
    for (;;) {      // one pass at fastTh; a second one at 7 for a band with <= 3 survivors@fastTh
    {
        int base = i_begin;
        for (; base + RG <= i_end; base += RG) round(std::true_type{}, base);
        if (base < i_end) round(std::false_type{}, base);
    }
    // Drain this wave's queues.  The remainders (< 64 each) run with a fraction of the lanes whatever is done, and this tail is a chain
    // of dependent LDS round trips (measured by cutting the kernel short: the drain costs 0.28 of the 1.08 ms per 1024 VGA frames,
    // the whole dense phase 0.34).  So the pair test is skipped here: it is only a filter (a pixel that fails it scores below tmin,
    // i.e. 0) and costs a queue round trip plus the same 16 ring reads the score needs; the pixel remainder and the pair-tested
    // remainder are scored together in one pass (two when they exceed a wave).
    if (n0) expand_step(q0, n0);
    for (int base = 0; base < n1 + n2; base += 64) {
        const int i = base + lane;
        const bool on = i < n1 + n2;
        score_vals(on, on ? (int)(i < n1 ? q1[i] : q2[i - n1]) : 0);
    }
    if (n3 > Q3CAP && lane == 0) hdr->overflow = 1;
    __syncthreads();

    // N: 3x3 strict NMS of the scored pixels of the band's own rows.  Scores of the halo columns / rows and of every non-corner
    // are 0, which is what cv::FAST's NMS sees outside the cell view.
    auto nms_test = [&](int p, int s) -> bool {       // strict maximum of its 3 x 3 neighbourhood: the survivor's bit is set
        const uint8_t* sp = s_sc + p;
        const int mx = imax3(imax3(sp[-1], sp[1], sp[-S]), imax3(sp[S], sp[-S - 1], sp[-S + 1]), imax(sp[S - 1], sp[S + 1]));
        if (s > mx) {
            const int bit = p - q_own_lo;
            atomicOr(&cmask[bit >> 6], 1ull << (bit & 63));
        }
        return s > mx;
    };
    auto nms_px = [&](int p, int s) {                 // ... counted per lane (the dense sweep's lanes are out of step)
        if (nms_test(p, s)) {
            if (s >= g.fast_th) atomicAdd(&hdr->n_hi, 1);
            if (s >= 7) atomicAdd(&hdr->n_lo, 1);
        }
    };
    if (!hdr->overflow) {
        int c_hi = 0, c_lo = 0;                       // counted per wave: two ballots per pass instead of two LDS atomics per survivor
        for (int i0 = 0; i0 < n3; i0 += 64) {
            const int i = i0 + lane;
            int s = 0;
            bool keep = false;
            if (i < n3) {
                const int p = q3[i];
                s = s_sc[p];
                keep = p >= q_own_lo && p < q_own_hi && nms_test(p, s);
            }
            c_hi += __popcll(__ballot(keep && s >= g.fast_th));
            c_lo += __popcll(__ballot(keep && s >= 7));
        }
        if (lane == 0 && (c_hi | c_lo)) { atomicAdd(&hdr->n_hi, c_hi); atomicAdd(&hdr->n_lo, c_lo); }      // (fastTh < 7: scores of 5 and 6 count in n_hi only)
    } else {
        const int d_lo = q_own_lo >> 2, d_hi = q_own_hi >> 2;
        for (int i = d_lo + tid; i < d_hi; i += NT) {
            uint32_t sc4 = reinterpret_cast<const uint32_t*>(s_sc)[i];
            while (sc4) {
                const int j = (__ffs((int)sc4) - 1) >> 3;
                const int s = (int)((sc4 >> (8 * j)) & 255u);
                sc4 &= ~(255u << (8 * j));
                nms_px(4 * i + j, s);
            }
        }
    }
    __syncthreads();
    if (tmin <= 7 || __builtin_amdgcn_readfirstlane(hdr->n_hi) > 3) break;          // workgroup-uniform
    // second pass at the fallback threshold: score plane, survivor masks and counts start over (the staged image stays)
    __syncthreads();                                 // every wave has read n_hi
    clear_lds();
    tmin = 7;
    K = compass_consts(7);
    n0 = n1 = n2 = n3 = 0;
    __syncthreads();
    }
    // the band's keypoint list in raster order (cv::FAST's order): one lane per 64-byte chunk of the survivor bitmask
    Cand* out = b.cand + (long long)frame * g.frame_cands + L.cand_base + bg.cand_off;
    const float inv_S = bg.inv_s;
    int run_base = 0;
    for (int c0 = 0; c0 < nchunks; c0 += NT) {
        // a wave whose 64 chunks lie beyond the band (waves 2 and 3 of a VGA level-0 band: 81 chunks) only keeps the barriers company:
        // it reports a count of 0 and skips the scan, the count exchange and the output loop (wave 0 is never idle: it carries run_base)
        const bool busy = c0 + 64 * wave < nchunks;
        unsigned long long m = 0ull;
        int cnt = 0, incl = 0;
        if (busy) {
            if (c0 + tid < nchunks) m = cmask[c0 + tid];
            cnt = __popcll(m);
            incl = wave_scan_inclusive(cnt);
        }
        if (NW > 1) {
            if (lane == 63) hdr->wsum[wave] = incl;
            __syncthreads();
        }
        int run = run_base + incl - cnt, total = NW > 1 ? 0 : __builtin_amdgcn_readlane(incl, 63);
        if (NW > 1 && busy) {
#pragma unroll
            for (int wv = 0; wv < NW; wv++) { const int t = hdr->wsum[wv]; if (wv < wave) run += t; total += t; }
        }
        while (m) {
            const int bit = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int p = q_own_lo + (c0 + tid) * 64 + bit;
            int r, xr;
            split_px(p, S, inv_S, r, xr);
            Cand e;
            e.pos = (uint32_t)(bg.x0 + xr - x_first) | ((uint32_t)(bg.ey0 + r - 3) << 16);
            e.resp = (float)s_sc[p];
            out[run++] = e;
        }
        run_base += total;
        if (NW > 1 && c0 + NT < nchunks) __syncthreads();
    }
    if (tid == 0) {
        CellState st;
        st.n_all = run_base; st.n_hi = hdr->n_hi; st.n_lo = hdr->n_lo;
        st.thr = tmin | ((st.n_hi <= 3 && g.fast_th > 7 ? imin(hint + 1, FAST_HINT_RUN) : 0) << 8);      // list threshold | the slot's run of fallbacks
        *cst = st;
    }
}

// (round 5: workgroups walking 2 / 4 / 16 bands grid-stride — one launch of long-lived workgroups instead of 729 k short ones — took
//  1.02 / 1.02 / 1.05 ms against 0.845 per 1024 VGA frames: the dispatcher's interleaving of fresh workgroups is what hides a band's
//  serial phases, a resident workgroup exposes them)
template <bool ALIGNED, int NT, int PPT, bool GATHER>
__device__ __forceinline__ void k_fast_cells_body(const Batch& b) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int frame, item;
    if (!frame_item_magic(b, blockIdx.x, (unsigned)b.g.nbands_total, b.g.nbands_magic, frame, item)) return;
    fast_band_task<ALIGNED, NT, PPT, GATHER>(b, frame, item, smem);
}
template <bool ALIGNED, int NT, int PPT>
__global__ __launch_bounds__(NT) void k_fast_cells(Batch b) { k_fast_cells_body<ALIGNED, NT, PPT, false>(b); }
template <bool ALIGNED, int NT, int PPT>
__global__ __launch_bounds__(NT) void k_fast_cells_gather(Batch b) { k_fast_cells_body<ALIGNED, NT, PPT, true>(b); }

// FAST and the blur both depend on the pyramid only.  A launch group that cannot fill the chip (the one-frame drop-in call) runs
// them side by side in ONE launch: the first blocks of a frame blur short strips (4 waves = 4 strips), the rest are cell bands.
// (Two streams would do the same for a full batch - launch_extract forks there - but a fork / join across hardware queues costs
// ~8 us each way, as much as either kernel takes on one frame.)
template <bool ALIGNED, bool SMALL, bool GATHER>
__device__ __forceinline__ void k_fast_blur_body(const Batch& b) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr FastShape A = SMALL ? FAST_SMALL : FAST_LARGE;
    constexpr int NW = A.threads / 64;
    const DevGeom& g = b.g;
    const int nblur = (g.nbtiles_total_s + NW - 1) / NW;
    const int per_frame = nblur + g.nbands_total;
    const int frame = blockIdx.x / per_frame, item = blockIdx.x - frame * per_frame;
    if (item < nblur) {
        const int t = item * NW + wave_id();
        if (t < g.nbtiles_total_s) blur_strip<ALIGNED, BLUR_ROWS_SMALL, GATHER>(b, frame, t);
    } else fast_band_task<ALIGNED, A.threads, A.ppt, GATHER>(b, frame, item - nblur, smem);
}
template <bool ALIGNED, bool SMALL>
__global__ __launch_bounds__(SMALL ? FAST_SMALL.threads : FAST_LARGE.threads) void k_fast_blur(Batch b) { k_fast_blur_body<ALIGNED, SMALL, false>(b); }
template <bool ALIGNED, bool SMALL>
__global__ __launch_bounds__(SMALL ? FAST_SMALL.threads : FAST_LARGE.threads) void k_fast_blur_gather(Batch b) { k_fast_blur_body<ALIGNED, SMALL, true>(b); }


// launch_extract's FAST stage: which of the sixteen entry points (orbx_launch.h: FastVariant), then the launch that switches on it.
// fuse_blur: the blur's short strips ride in the same launch
StagePlan plan_fast(const Batch& b, const HostGeom& hg, bool fuse_blur) {
    const DevGeom& g = hg.g;
    const bool aligned = (level0_bits(b) & 3) == 0;
    return stage_plan((aligned ? FV_ALIGNED : 0) | (g.fast_small ? FV_SMALL : 0) | (b.img_tab ? FV_GATHER : 0) | (fuse_blur ? FV_BLUR : 0),
                      (g.fast_lds_bytes > 64 * 1024 ? ORBX_VF_LDS_OVER_64K : 0u) | (fuse_blur ? ORBX_VF_FUSE_BLUR : 0u));
}
const char* fast_variant_name(int id) {
    static const char* const names[FV_COUNT] = {
        "k_fast_cells<false, FAST_LARGE>", "k_fast_cells<true, FAST_LARGE>", "k_fast_cells<false, FAST_SMALL>", "k_fast_cells<true, FAST_SMALL>",
        "k_fast_cells_gather<false, FAST_LARGE>", "k_fast_cells_gather<true, FAST_LARGE>", "k_fast_cells_gather<false, FAST_SMALL>", "k_fast_cells_gather<true, FAST_SMALL>",
        "k_fast_blur<false, false>", "k_fast_blur<true, false>", "k_fast_blur<false, true>", "k_fast_blur<true, true>",
        "k_fast_blur_gather<false, false>", "k_fast_blur_gather<true, false>", "k_fast_blur_gather<false, true>", "k_fast_blur_gather<true, true>"};
    return id >= 0 && id < FV_COUNT ? names[id] : "?";
}

int launch_fast(const Batch& b, const HostGeom& hg, hipStream_t stream, const StagePlan& plan) {
    const DevGeom& g = hg.g;
    const int F = b.nframes;
    const size_t lds = (size_t)g.fast_lds_bytes;
    const bool big_lds = (plan.flags & ORBX_VF_LDS_OVER_64K) != 0;
    auto launch = [&](auto kern, int threads) -> bool {
        if (big_lds && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
        hipLaunchKernelGGL(kern, dim3(frame_item_blocks(b, g.nbands_total)), dim3(threads), lds, stream, b);
        return true;
    };
    constexpr FastShape A = FAST_SMALL, B = FAST_LARGE;
    const int threads = (plan.id & FV_SMALL) ? A.threads : B.threads;
    const int per_frame = (g.nbtiles_total_s + threads / 64 - 1) / (threads / 64) + g.nbands_total;
    auto launch2 = [&](auto kern) -> bool {       // the blur's short strips ride in front of every frame's bands
        if (big_lds && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
        hipLaunchKernelGGL(kern, dim3(F * per_frame), dim3(threads), lds, stream, b);
        return true;
    };
    bool ok;
    switch (plan.id) {
        case 0: ok = launch(k_fast_cells<false, B.threads, B.ppt>, B.threads); break;
        case FV_ALIGNED: ok = launch(k_fast_cells<true, B.threads, B.ppt>, B.threads); break;
        case FV_SMALL: ok = launch(k_fast_cells<false, A.threads, A.ppt>, A.threads); break;
        case FV_SMALL | FV_ALIGNED: ok = launch(k_fast_cells<true, A.threads, A.ppt>, A.threads); break;
        case FV_GATHER: ok = launch(k_fast_cells_gather<false, B.threads, B.ppt>, B.threads); break;
        case FV_GATHER | FV_ALIGNED: ok = launch(k_fast_cells_gather<true, B.threads, B.ppt>, B.threads); break;
        case FV_GATHER | FV_SMALL: ok = launch(k_fast_cells_gather<false, A.threads, A.ppt>, A.threads); break;
        case FV_GATHER | FV_SMALL | FV_ALIGNED: ok = launch(k_fast_cells_gather<true, A.threads, A.ppt>, A.threads); break;
        case FV_BLUR: ok = launch2(k_fast_blur<false, false>); break;
        case FV_BLUR | FV_ALIGNED: ok = launch2(k_fast_blur<true, false>); break;
        case FV_BLUR | FV_SMALL: ok = launch2(k_fast_blur<false, true>); break;
        case FV_BLUR | FV_SMALL | FV_ALIGNED: ok = launch2(k_fast_blur<true, true>); break;
        case FV_BLUR | FV_GATHER: ok = launch2(k_fast_blur_gather<false, false>); break;
        case FV_BLUR | FV_GATHER | FV_ALIGNED: ok = launch2(k_fast_blur_gather<true, false>); break;
        case FV_BLUR | FV_GATHER | FV_SMALL: ok = launch2(k_fast_blur_gather<false, true>); break;
        case FV_BLUR | FV_GATHER | FV_SMALL | FV_ALIGNED: ok = launch2(k_fast_blur_gather<true, true>); break;
        default: return ORBX_ERR_ARG;
    }
    if (!ok) return ORBX_ERR_DEVICE;
    ORBX_LAUNCH_CHECK();
    return ORBX_OK;
}

}  // namespace orbx
