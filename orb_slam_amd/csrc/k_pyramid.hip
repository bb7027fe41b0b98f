// Pyramid kernels of the ORB extractor for gfx950 (ComputePyramid, reference src/ORBextractor.cc:781-822: cv::resize INTER_LINEAR 8U level after level):
// k_resize (one launch per level: full launch groups) and k_pyramid (cones of levels in one launch: launch groups too small to fill the chip).
#include <algorithm>
#include <type_traits>

#include "k_resize_strip.h"
#include "orbx_device.h"
#include "orbx_launch.h"

namespace orbx {

// ------------------------------------------------------------------------------------ pyramid
// cv::resize INTER_LINEAR 8U, level-1 -> level.  A workgroup produces a 256 x RZ_ROWS output tile: the source rectangle it
// needs (<= ~60 rows x ~310 px at scale 1.2) is staged in LDS (LDS-DMA for aligned planes), each lane then produces 4 horizontally
// adjacent output pixels per row of its wave's RZ_ROWS / 4 consecutive rows and stores one dword per row.
// (Byte gathers straight from global memory made this kernel texture-addresser bound.)
// LDS source tile: L.rz_rows x L.rz_pitch bytes, the exact maximum over the level's tiles (a fixed worst-case array for scale
// 2.5 capped the kernel's occupancy)

template <bool ALIGNED, bool WINDOW, bool GATHER>
__device__ __forceinline__ void k_resize_body(Batch b, int level) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_src[];
    const DevGeom& g = b.g;
    const LevelGeom& L = g.lv[level];
    const int RZ_SRC_W = L.rz_pitch;
    const LevelGeom& P = g.lv[level - 1];
    const int tiles_x = (L.w + 255) / 256, tiles_y = (L.h + RZ_ROWS - 1) / RZ_ROWS;
    int frame, tile;
    if (!frame_item(b, blockIdx.x, tiles_x * tiles_y, frame, tile)) return;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int bx0 = tile_x * 256, by0 = tile_y * RZ_ROWS;
    const int bx1 = min(bx0 + 255, L.w - 1), by1 = min(by0 + RZ_ROWS - 1, L.h - 1);
    long long sstride;
    const uint8_t* src = plain_plane<GATHER>(b, P, level - 1, frame, sstride);
    const ResizeX* tx = b.tabx + L.tabx_off;
    const ResizeY* ty = b.taby + L.taby_off;
    // this lane's 4 output columns (independent of the staging below: issued first)
    const int dx0 = bx0 + lane * 4;
    ResizeX rx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) rx[k] = tx[min(dx0 + k, L.w - 1)];
    // the row-table entries of this wave's output rows, one per lane, fetched before the staging: read inside the row loop they
    // were a global-load round trip per output row (a uniform address, but not provably read-only, so no scalar load), and that
    // chain of dependent loads - not the VALU work - set the kernel's pace
    constexpr int RPW = RZ_ROWS / 4;                               // consecutive output rows per wave (windowed form)
    const uint2 ryl = *reinterpret_cast<const uint2*>(ty + min(by0 + wave * RPW + min(lane, RPW - 1), L.h - 1));
    // source rectangle of this tile (tables are monotone)
    const int r0 = ty[by0].sy0, r1 = ty[by1].sy1;
    const int c0 = tx[bx0].sx & ~3, c1 = tx[bx1].sx1;
    const int nd = ((c1 - c0) >> 2) + 1, nr = r1 - r0 + 1;
    if (ALIGNED) {
        // LDS-DMA staging (as in k_fast_cells): one global_load_lds_dword per (row, 64-dword piece), lane i's dword lands at
        // M0 + 4 i.  Row bases are scalars, so the staging costs a wave ~2 instructions per row instead of ~20 VALU instructions
        // per dword (flattened index -> row / column, bounds, address, ds_write): that loop was 45 % of this kernel's instructions.
        typedef const void __attribute__((address_space(1))) * gptr_t;
        typedef void __attribute__((address_space(3))) * lptr_t;
        const uint8_t* base = src + (long long)r0 * sstride + c0;
        for (int p0 = 0; p0 < nd; p0 += 64) {
            const bool on = p0 + lane < nd;
            for (int r = wave; r < nr; r += 4) {
                const uint8_t* grow = base + (long long)r * sstride + 4 * p0;     // wave-uniform
                if (on) __builtin_amdgcn_global_load_lds((gptr_t)(grow + 4 * lane), (lptr_t)(s_src + r * RZ_SRC_W + 4 * p0), 4, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA writes have landed; the barrier below covers the other waves
    } else {
        // unaligned frames (level 0 -> 1 only): flattened (row, dword) items, 8 independent loads in flight per lane
        const int total = nr * nd;
        const float inv_nd = 1.0f / (float)nd;
        const uint8_t* base = src + (long long)r0 * sstride + c0;
        const int xm = P.w - 1 - c0;
        for (int i0 = 0; i0 < total; i0 += 256 * 8) {
            uint32_t v4[8];
            int off[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = i0 + k * 256 + tid;
                v4[k] = 0;
                off[k] = -1;
                if (i < total) {
                    int r, d;
                    split_px(i, nd, inv_nd, r, d);
                    const uint8_t* row = base + (long long)r * sstride;
                    off[k] = r * RZ_SRC_W + 4 * d;
                    if (ALIGNED) v4[k] = *reinterpret_cast<const uint32_t*>(row + 4 * d);
                    else v4[k] = (uint32_t)row[min(4 * d, xm)] | (uint32_t)row[min(4 * d + 1, xm)] << 8 | (uint32_t)row[min(4 * d + 2, xm)] << 16 |
                                 (uint32_t)row[min(4 * d + 3, xm)] << 24;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (off[k] >= 0) *reinterpret_cast<uint32_t*>(s_src + off[k]) = v4[k];
        }
    }
    __syncthreads();
    if (dx0 >= L.w) return;
    uint8_t* dplane = b.pyr + (long long)frame * g.frame_plane_bytes + L.plane_off;
    if (WINDOW) {
        // Windowed form (scale factors up to ~1.7): the lane's 8 source bytes of a row lie within 8 bytes from its first tap.  Three
        // aligned LDS dwords + two v_alignbyte bring that window into a register pair; a per-lane v_perm selector (row-invariant)
        // builds (s[sx] | s[sx1] << 16) of each output pixel and v_dot2_u32_u16 with (a0 | a1 << 16) is the horizontal pass
        // (D = S[sx]*a0 + S[sx+1]*a1).  A wave works on CONSECUTIVE output rows, so the lower source row of one output row is
        // usually the upper one of the next and its horizontal results are reused (1.2 instead of 2 source rows per output row).
        const int w0 = rx[0].sx - c0;                              // the lane's first tap inside the staged row
        const int wa = w0 & ~3, sh = w0 & 3;
        uint32_t sel[4], apair[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            sel[k] = (uint32_t)(rx[k].sx - c0 - w0) | 0x0C000C00u | ((uint32_t)(rx[k].sx1 - c0 - w0) << 16);     // bytes: s[sx], 0, s[sx1], 0
            apair[k] = (uint32_t)(uint16_t)rx[k].a0 | ((uint32_t)(uint16_t)rx[k].a1 << 16);
        }
        // hrow leaves the horizontal results already shifted (D >> 4, the form the vertical pass consumes: once per source row, not
        // once per use).  Vertical pass: (b * (D >> 4)) >> 16 is v_mul_hi_u32 with the weight pre-shifted to the high half (a scalar
        // per row) - one instruction instead of multiply + shift; the result is < 256 by construction (weights sum to 2048), so the
        // four pixels are packed with shift-or, no masks.
        auto hrow = [&](int sy, uint32_t (&d)[4]) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(s_src + (sy - r0) * RZ_SRC_W + wa);
            const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
            const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)sh), hi = __builtin_amdgcn_alignbyte(d2, d1, (uint32_t)sh);
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = __builtin_amdgcn_udot2(as_us2v(__builtin_amdgcn_perm(hi, lo, sel[k])), as_us2v(apair[k]), 0u, false) >> 4;
        };
        int have = -1;
        uint32_t dprev[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < RPW; j++) {
            const int dy = by0 + wave * RPW + j;
            if (dy >= L.h) break;
            const uint32_t ry_rows = (uint32_t)__builtin_amdgcn_readlane((int)ryl.x, j), ry_w = (uint32_t)__builtin_amdgcn_readlane((int)ryl.y, j);
            const int sy0 = (int16_t)(ry_rows & 0xffffu), sy1 = (int16_t)(ry_rows >> 16);
            const uint32_t b0s = ry_w << 16, b1s = ry_w & 0xffff0000u;      // the weights (0 .. 2048) in the high halves
            uint32_t da[4], db[4];
            if (sy0 == have) {
#pragma unroll
                for (int k = 0; k < 4; k++) da[k] = dprev[k];
            } else hrow(sy0, da);
            if (sy1 == sy0) {
#pragma unroll
                for (int k = 0; k < 4; k++) db[k] = da[k];
            } else hrow(sy1, db);
            have = sy1;
            uint32_t packed = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                dprev[k] = db[k];
                const uint32_t px = (__umulhi(da[k], b0s) + __umulhi(db[k], b1s) + 2u) >> 2;
                packed |= px << (8 * k);
            }
            // columns past L.w (dx0+k clamped above) land in the row padding: stride is a multiple of 64
            *reinterpret_cast<uint32_t*>(dplane + (long long)dy * L.stride + dx0) = packed;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < RZ_ROWS / 4; j++) {
        const int dy = by0 + wave + 4 * j;
        if (dy >= L.h) break;
        const ResizeY ry = ty[dy];
        const uint8_t* q0 = s_src + (ry.sy0 - r0) * RZ_SRC_W - c0;
        const uint8_t* q1 = s_src + (ry.sy1 - r0) * RZ_SRC_W - c0;
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int px = resize_px(q0[rx[k].sx], q0[rx[k].sx1], q1[rx[k].sx], q1[rx[k].sx1], rx[k].a0, rx[k].a1, ry.b0, ry.b1);
            packed |= (uint32_t)(px & 255) << (8 * k);
        }
        // columns past L.w (dx0+k clamped above) land in the row padding: stride is a multiple of 64
        *reinterpret_cast<uint32_t*>(dplane + (long long)dy * L.stride + dx0) = packed;
    }
}
template <bool ALIGNED, bool WINDOW>
__global__ __launch_bounds__(256) void k_resize(Batch b, int level) { k_resize_body<ALIGNED, WINDOW, false>(b, level); }
template <bool ALIGNED, bool WINDOW>
__global__ __launch_bounds__(256) void k_resize_gather(Batch b, int level) { k_resize_body<ALIGNED, WINDOW, true>(b, level); }

// Strip form of the per-level resize, k_resize_strip (k_resize_strip.h): a workgroup produces rows_out consecutive output rows across the WHOLE width of
// the level.  The source rows of such a strip are one contiguous byte range of the plane below, so the staging is a flat list of 16-byte
// LDS-DMA chunks with no row / column split at all (k_resize's 256-px tile columns need one 4-byte DMA instruction per row and 64-dword
// piece, each with its own address arithmetic: ~300 per level-1 tile), and there are no narrow tail tiles whose four waves walk their rows
// with a few live lanes.  The arithmetic is k_resize's windowed form, bit for bit: the same tables, v_dot2, >> 4, v_mul_hi, + 2 >> 2.
// Wave v owns rows_out / 4 consecutive output rows (scalar row weights, the lower source row's horizontal results reused) and walks the
// level's groups of 64 dword columns; a last group of at most RZS_ROWPAR_MAX columns is row-parallel instead: lanes hold (column, row) pairs
// with per-lane row weights and source-row offsets, and always compute both source rows.
// NG: the level's groups when they are few enough to keep every group's column constants in registers (fetched before the staging wait);
// 0: any number, fetched group by group.
struct RzsCols {
    uint32_t sel[4], apair[4];     // v_perm selectors and weight pairs of the lane's four output pixels (row-invariant)
    int wa, sh;                    // first tap of the lane: aligned byte column of its three-dword window, byte shift inside it
};
__device__ __forceinline__ void rzs_load_cols(const ResizeX* tx, int w, int dcol, RzsCols& c) {
    ResizeX rx[4];
#pragma unroll
    for (int k = 0; k < 4; k++) rx[k] = tx[min(4 * dcol + k, w - 1)];
    const int w0 = rx[0].sx;
    c.wa = w0 & ~3;
    c.sh = w0 & 3;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        c.sel[k] = (uint32_t)(rx[k].sx - w0) | 0x0C000C00u | ((uint32_t)(rx[k].sx1 - w0) << 16);     // bytes: s[sx], 0, s[sx1], 0
        c.apair[k] = (uint32_t)(uint16_t)rx[k].a0 | ((uint32_t)(uint16_t)rx[k].a1 << 16);
    }
}
// horizontal pass of one source row (LDS byte offset `off` of the lane's aligned window): D >> 4 of the lane's four pixels
__device__ __forceinline__ void rzs_hrow(const uint8_t* s_src, int off, const RzsCols& c, uint32_t (&d)[4]) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(s_src + off);
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
    const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)c.sh), hi = __builtin_amdgcn_alignbyte(d2, d1, (uint32_t)c.sh);
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] = __builtin_amdgcn_udot2(as_us2v(__builtin_amdgcn_perm(hi, lo, c.sel[k])), as_us2v(c.apair[k]), 0u, false) >> 4;
}
__device__ __forceinline__ uint32_t rzs_vpack(const uint32_t (&da)[4], const uint32_t (&db)[4], uint32_t b0s, uint32_t b1s) {
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) packed |= ((__umulhi(da[k], b0s) + __umulhi(db[k], b1s) + 2u) >> 2) << (8 * k);
    return packed;
}

template <bool GATHER, int NG>
__device__ __forceinline__ void k_resize_strip_body(Batch b, int level, int rows_out, int nstrips, unsigned magic) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_src[];
    const DevGeom& g = b.g;
    const LevelGeom& L = g.lv[level];
    const LevelGeom& P = g.lv[level - 1];
    int frame, strip;
    if (!frame_item_magic(b, blockIdx.x, (unsigned)nstrips, magic, frame, strip)) return;      // (nstrips = rzs_strips(L.h, rows_out) and its magic: host)
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    long long sstride64;
    const uint8_t* src = plain_plane<GATHER>(b, P, level - 1, frame, sstride64);
    const int sstride = (int)sstride64;                          // (a strip fits the LDS budget: host-checked)
    const ResizeX* tx = b.tabx + L.tabx_off;
    const ResizeY* ty = b.taby + L.taby_off;
    const int RPW = rows_out >> 2;                               // consecutive output rows per wave
    const int row0 = strip * rows_out + wave * RPW;
    // the row-table entries of this wave's output rows, one per lane (see k_resize)
    const uint2 ryl = *reinterpret_cast<const uint2*>(ty + min(row0 + min(lane, RPW - 1), L.h - 1));
    const int ngroups = NG ? NG : rzs_groups(L.w);
    const int rem = rzs_rem_cols(L.w);
    const bool rowpar = rem <= RZS_ROWPAR_MAX;
    const int shift = rzs_rowpar_shift(rem);
    auto group_col = [&](int gi) { return gi == ngroups - 1 && rowpar ? 64 * gi + rzs_rowpar_slot(lane, shift) : rzs_loop_col(gi, lane); };
    // the column constants of every group, independent of the staging below: issued first
    RzsCols cols[NG ? NG : 1];
    if (NG) {
#pragma unroll
        for (int gi = 0; gi < NG; gi++) rzs_load_cols(tx, L.w, group_col(gi), cols[gi]);
    }
    // the strip's source rows: fetched behind the table loads above, so that one wait covers them all (not a round trip of its own in front of them)
    __builtin_amdgcn_sched_barrier(0);
    const StripSpan sp = rzs_span(ty, L.h, rows_out, strip, sstride64, rzs_readable(level == 1, sstride64, P.w));
    const int r0 = sp.r0, nchunks = (int)sp.chunks;
    {
        typedef const void __attribute__((address_space(1))) * gptr_t;
        typedef void __attribute__((address_space(3))) * lptr_t;
        const uint8_t* base = src + (long long)r0 * sstride64;
        // dwords behind the last whole chunk (a level-0 pitch that is no multiple of 16): plain loads, in front of the DMA (the compiler
        // orders every LDS write behind outstanding LDS-DMA loads)
        if (tid < sp.tail_dwords)
            *reinterpret_cast<uint32_t*>(s_src + 16 * nchunks + 4 * tid) = *reinterpret_cast<const uint32_t*>(base + 16 * (long long)nchunks + 4 * tid);
        // chunk q of the range -> LDS offset 16 q; a wave instruction moves 64 consecutive chunks (lane i's 16 bytes land at M0 + 16 i)
        for (int q0 = 64 * wave; q0 < nchunks; q0 += 256)
            if (q0 + lane < nchunks) __builtin_amdgcn_global_load_lds((gptr_t)(base + 16 * (q0 + lane)), (lptr_t)(s_src + 16 * q0), 16, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA writes have landed; the barrier below covers the other waves
    }
    __syncthreads();
    uint8_t* dplane = b.pyr + (long long)frame * g.frame_plane_bytes + L.plane_off;      // (wave-uniform; a frame's planes are below 2^31 bytes: 32-bit offsets)
    const unsigned dstride = (unsigned)L.stride;
    const int nrows = min(RPW, L.h - row0);                      // this wave's rows inside the level (<= 0: none)
    auto process = [&](int gi, const RzsCols& c) {
        const int dcol = group_col(gi);
        if (gi == ngroups - 1 && rowpar) {
            // row-parallel remainder: 2^shift column slots x (64 >> shift) rows per pass; a lane's row entry comes from the lane that holds it
            const int slot = rzs_rowpar_slot(lane, shift);
            for (int pass = 0; pass * (64 >> shift) < RPW; pass++) {
                const int j = rzs_rowpar_row(lane, shift, pass);
                const uint32_t ry_rows = (uint32_t)__shfl((int)ryl.x, min(j, RPW - 1)), ry_w = (uint32_t)__shfl((int)ryl.y, min(j, RPW - 1));
                const int dy = row0 + j;
                if (slot < rem && j < RPW && dy < L.h) {
                    const int sy0 = (int16_t)(ry_rows & 0xffffu), sy1 = (int16_t)(ry_rows >> 16);
                    uint32_t da[4], db[4];
                    rzs_hrow(s_src, (sy0 - r0) * sstride + c.wa, c, da);
                    rzs_hrow(s_src, (sy1 - r0) * sstride + c.wa, c, db);
                    // columns past L.w (clamped in rzs_load_cols) land in the row padding: stride is a multiple of 64
                    *reinterpret_cast<uint32_t*>(dplane + ((unsigned)dy * dstride + 4u * (unsigned)dcol)) = rzs_vpack(da, db, ry_w << 16, ry_w & 0xffff0000u);
                }
            }
        } else if (4 * dcol < L.w) {
            // The lower source row's horizontal results stay in `cur` for the next output row; the upper row's share of the vertical pass is
            // taken before `cur` is overwritten, so nothing is copied from row to row.
            int have = -1;
            uint32_t cur[4] = {0, 0, 0, 0};
            for (int j = 0; j < nrows; j++) {
                const int dy = row0 + j;
                const uint32_t ry_rows = (uint32_t)__builtin_amdgcn_readlane((int)ryl.x, j), ry_w = (uint32_t)__builtin_amdgcn_readlane((int)ryl.y, j);
                const int sy0 = (int16_t)(ry_rows & 0xffffu), sy1 = (int16_t)(ry_rows >> 16);
                const uint32_t b0s = ry_w << 16, b1s = ry_w & 0xffff0000u;      // the weights (0 .. 2048) in the high halves
                if (sy0 != have) rzs_hrow(s_src, (sy0 - r0) * sstride + c.wa, c, cur);
                uint32_t t[4];
#pragma unroll
                for (int k = 0; k < 4; k++) t[k] = __umulhi(cur[k], b0s);
                asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));      // (taken HERE: sunk below the second hrow, `cur` has to be copied first)
                if (sy1 != sy0) rzs_hrow(s_src, (sy1 - r0) * sstride + c.wa, c, cur);
                have = sy1;
                uint32_t packed = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) packed |= ((t[k] + __umulhi(cur[k], b1s) + 2u) >> 2) << (8 * k);
                // columns past L.w (clamped in rzs_load_cols) land in the row padding: stride is a multiple of 64
                *reinterpret_cast<uint32_t*>(dplane + ((unsigned)dy * dstride + 4u * (unsigned)dcol)) = packed;
            }
        }
    };
    if constexpr (NG != 0) {
#pragma unroll
        for (int gi = 0; gi < NG; gi++) process(gi, cols[gi]);
    } else {
        for (int gi = 0; gi < ngroups; gi++) {
            rzs_load_cols(tx, L.w, group_col(gi), cols[0]);
            process(gi, cols[0]);
        }
    }
}
// The entry points are overloads of k_resize / k_resize_gather, k_resize<NG>: the benchmark's per-stage counters and the profile tools find the pyramid
// stage by that kernel name, whichever form a level takes.
typedef void (*resize_strip_fn)(Batch, int, int, int, unsigned);
template <int NG>
__global__ __launch_bounds__(256) void k_resize(Batch b, int level, int rows_out, int nstrips, unsigned magic) { k_resize_strip_body<false, NG>(b, level, rows_out, nstrips, magic); }
template <int NG>
__global__ __launch_bounds__(256) void k_resize_gather(Batch b, int level, int rows_out, int nstrips, unsigned magic) { k_resize_strip_body<true, NG>(b, level, rows_out, nstrips, magic); }

// Fused pyramid: one launch produces the levels l0+1 .. l0+depth of a PyrGroup (round 2: 2 launches for 8 levels instead of 7
// dependent ones — on one frame each k_resize launch cost ~9 us of latency, 65 of the ~150 us of a frame's kernel chain).
// A workgroup owns a tile of the deepest level and the cone above it.  The region of the source level it needs is staged in
// LDS; every further level is computed from the LDS copy of the level above (the same fixed-point cv::resize arithmetic and
// tables as k_resize), kept in LDS for the next one and written to HBM where the tile OWNS it (regions of neighbouring tiles
// overlap by the bilinear footprint; ownership — region start to the next tile's region start — partitions each level).
// Threads: 32 dword columns x 8 row phases; a thread keeps its four resize-table entries across its rows.
template <bool ALIGNED, bool GATHER>
__global__ __launch_bounds__(256) void k_pyramid(Batch b, int group) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_lv[];
    const DevGeom& g = b.g;
    const PyrGroup& pg = g.pyr[group];
    const int frame = blockIdx.z, ix = blockIdx.x, iy = blockIdx.y;
    const int tid = threadIdx.x;
    const int l0 = pg.l0, depth = pg.depth;
    if (group == 0 && ix == 0 && iy == 0 && tid == 0) b.status[frame] = ORBX_OK;     // (the selection stage may set an error later)
    const int* xt = b.pyr_tab + pg.xtab;
    const int* yt = b.pyr_tab + pg.ytab;
    auto xr = [&](int k, int i, int e) { return xt[(k * (pg.ntx + 1) + i) * 2 + e]; };
    auto yr = [&](int k, int i, int e) { return yt[(k * (pg.nty + 1) + i) * 2 + e]; };
    // stage the source region (level l0): rows ys..ye, dwords from xs (a multiple of 4)
    {
        const LevelGeom& P = g.lv[l0];
        const int xs = xr(0, ix, 0), xe = xr(0, ix, 1), ys = yr(0, iy, 0), ye = yr(0, iy, 1);
        const int nd = ((xe - xs) >> 2) + 1, nr = ye - ys + 1;
        long long sstride;
        const uint8_t* src = plain_plane<GATHER>(b, P, l0, frame, sstride);
        const uint8_t* base = src + (long long)ys * sstride + xs;
        const int xm = P.w - 1 - xs;
        const int total = nr * nd;
        const float inv_nd = 1.0f / (float)nd;
        const int pitch = pg.pitch[0];
        for (int i0 = 0; i0 < total; i0 += 256 * 8) {
            uint32_t v4[8];
            int off[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int i = i0 + k * 256 + tid;
                v4[k] = 0;
                off[k] = -1;
                if (i < total) {
                    int r, d;
                    split_px(i, nd, inv_nd, r, d);
                    const uint8_t* row = base + (long long)r * sstride;
                    off[k] = r * pitch + 4 * d;
                    if (ALIGNED) v4[k] = *reinterpret_cast<const uint32_t*>(row + 4 * d);
                    else v4[k] = (uint32_t)row[min(4 * d, xm)] | (uint32_t)row[min(4 * d + 1, xm)] << 8 | (uint32_t)row[min(4 * d + 2, xm)] << 16 |
                                 (uint32_t)row[min(4 * d + 3, xm)] << 24;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (off[k] >= 0) *reinterpret_cast<uint32_t*>(s_lv + pg.lds_off[0] + off[k]) = v4[k];
        }
    }
    __syncthreads();
    for (int k = 1; k <= depth; k++) {
        const int level = l0 + k;
        const LevelGeom& L = g.lv[level];
        const ResizeX* tx = b.tabx + L.tabx_off;
        const ResizeY* ty = b.taby + L.taby_off;
        const int xs = xr(k, ix, 0), xe = xr(k, ix, 1), ys = yr(k, iy, 0), ye = yr(k, iy, 1);
        const int own_x1 = xr(k, ix + 1, 0), own_y1 = yr(k, iy + 1, 0);          // owned: [xs, own_x1) x [ys, own_y1)
        const int sxs = xr(k - 1, ix, 0), sys = yr(k - 1, iy, 0);
        const uint8_t* sbuf = s_lv + pg.lds_off[k - 1];
        const int spitch = pg.pitch[k - 1];
        uint8_t* dbuf = k < depth ? s_lv + pg.lds_off[k] : nullptr;
        const int dpitch = k < depth ? pg.pitch[k] : 0;
        uint8_t* dplane = b.pyr + (long long)frame * g.frame_plane_bytes + L.plane_off;
        const int ngroups = ((xe - xs) >> 2) + 1;
        // threads: dword columns x row phases, the split chosen per level (the regions narrow towards the deepest level)
        const int lc = ngroups > 16 ? 5 : ngroups > 8 ? 4 : 3;
        const int gx = tid & ((1 << lc) - 1), gy = tid >> lc, ystep = 256 >> lc;
        for (int G0 = 0; G0 < ngroups; G0 += 1 << lc) {
            const int G = G0 + gx;
            if (G >= ngroups) continue;
            const int X = xs + 4 * G;
            ResizeX rx[4];
#pragma unroll
            for (int j = 0; j < 4; j++) rx[j] = tx[min(X + j, L.w - 1)];
            for (int y = ys + gy; y <= ye; y += ystep) {
                const ResizeY ry = ty[y];
                const uint8_t* q0 = sbuf + (ry.sy0 - sys) * spitch - sxs;
                const uint8_t* q1 = sbuf + (ry.sy1 - sys) * spitch - sxs;
                uint32_t packed = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int px = resize_px(q0[rx[j].sx], q0[rx[j].sx1], q1[rx[j].sx], q1[rx[j].sx1], rx[j].a0, rx[j].a1, ry.b0, ry.b1);
                    packed |= (uint32_t)(px & 255) << (8 * j);
                }
                if (dbuf) *reinterpret_cast<uint32_t*>(dbuf + (y - ys) * dpitch + 4 * G) = packed;
                // columns past L.w (clamped above) land in the row padding: stride is a multiple of 64
                if (X < own_x1 && y < own_y1) *reinterpret_cast<uint32_t*>(dplane + (long long)y * L.stride + X) = packed;
            }
        }
        __syncthreads();
    }
}


// Form of level `level`'s resize in this launch group (orbx_internal.h).  Levels >= 2 read pyramid planes: decided with the geometry.
// Level 1 reads the caller's frames: decided here from their alignment and (largest) pitch, which is the pitch of the LDS tile.
int resize_form(const Batch& b, const HostGeom& hg, int level, StripChoice& sc) {
    const DevGeom& g = hg.g;
    sc = StripChoice{0, 0};
    if (level < 1 || level >= g.nlevels) return RZ_FORM_TILED;
    if (g.npyr_groups > 0 && b.nframes < PYR_FUSED_MAX_FRAMES) return RZ_FORM_FUSED;
    const LevelGeom& L = g.lv[level];
    if (level >= 2 || (level0_max_stride(b) == g.lv[0].w && (level0_bits(b) & 3) == 0)) sc = StripChoice{L.rs_rows, L.rs_lds};
    else sc = resize_strip_choice(hg, level, level0_max_stride(b), level0_bits(b));
    return sc.rows_out ? RZ_FORM_STRIP : RZ_FORM_TILED;
}

template <int NG>
static void launch_resize_strip(const Batch& b, int l, const StripChoice& sc, bool gather, hipStream_t stream) {
    const LevelGeom& L = b.g.lv[l];
    const int nstrips = rzs_strips(L.h, sc.rows_out);
    const unsigned magic = frame_item_magic_of(nstrips);
    dim3 grid(frame_item_blocks(b, nstrips));
    const resize_strip_fn fn = gather ? static_cast<resize_strip_fn>(&k_resize_gather<NG>) : static_cast<resize_strip_fn>(&k_resize<NG>);
    hipLaunchKernelGGL(fn, grid, dim3(256), (size_t)sc.lds_bytes, stream, b, l, sc.rows_out, nstrips, magic);
}

// The launches of the pyramid stage, in order (orbx_launch.h).  Fused cones when the batch is too small to fill the chip (the drop-in call: one
// frame): there the chain of dependent launches is the cost (189 vs 236 us per VGA frame); a full batch prefers the leaner per-level kernels
// (0.72 vs 0.81 ms per 1024 frames: the cones recompute their overlap and synchronise per level).
PyramidPlan plan_pyramid(const Batch& b, const HostGeom& hg) {
    const DevGeom& g = hg.g;
    const bool al0 = (level0_bits(b) & 3) == 0;
    PyramidPlan p;
    StripChoice sc;
    if (g.nlevels > 1 && resize_form(b, hg, 1, sc) == RZ_FORM_FUSED) {
        for (int gi = 0; gi < g.npyr_groups; gi++) {
            const bool first = g.pyr[gi].l0 == 0;       // (gather form: only the cone that starts at level 0 reads the caller's frames)
            p.launch[p.n++] = PyramidLaunch{PV_PYRAMID0 + ((!first || al0) ? 1 : 0) + ((b.img_tab && first) ? 2 : 0), gi, StripChoice{0, 0}};
        }
        return p;
    }
    for (int l = 1; l < g.nlevels; l++) {
        const LevelGeom& L = g.lv[l];
        const bool gather = b.img_tab && l == 1;        // (gather form: level 1 is the one resized from the caller's frames)
        if (resize_form(b, hg, l, sc) == RZ_FORM_STRIP) {
            const int ng = rzs_groups(L.w);             // groups of 64 dword columns: up to four keep their column constants in registers
            p.launch[p.n++] = PyramidLaunch{(gather ? PV_STRIP_GATHER0 : PV_STRIP0) + (ng <= 4 ? ng : 0), l, sc};
        } else
            p.launch[p.n++] = PyramidLaunch{PV_TILED0 + ((l > 1 || al0) ? 1 : 0) + (L.rz_window ? 2 : 0) + (gather ? 4 : 0), l, StripChoice{0, 0}};
    }
    return p;
}
const char* pyramid_variant_name(int id) {
    static const char* const names[PV_COUNT] = {
        "k_pyramid<false, false>", "k_pyramid<true, false>", "k_pyramid<false, true>", "k_pyramid<true, true>",
        "k_resize<false, false>", "k_resize<true, false>", "k_resize<false, true>", "k_resize<true, true>",
        "k_resize_gather<false, false>", "k_resize_gather<true, false>", "k_resize_gather<false, true>", "k_resize_gather<true, true>",
        "k_resize<0>", "k_resize<1>", "k_resize<2>", "k_resize<3>", "k_resize<4>",
        "k_resize_gather<0>", "k_resize_gather<1>", "k_resize_gather<2>", "k_resize_gather<3>", "k_resize_gather<4>"};
    return id >= 0 && id < PV_COUNT ? names[id] : "?";
}

// (launch_extract's pyramid stage; the per-frame status fill that rides on it stays with the caller)
int launch_pyramid(const Batch& b, const PyramidPlan& plan, hipStream_t stream) {
    const DevGeom& g = b.g;
    for (int i = 0; i < plan.n; i++) {
        const PyramidLaunch& pl = plan.launch[i];
        if (pl.variant < PV_TILED0) {
            const PyrGroup& pg = g.pyr[pl.index];
            const dim3 grid(pg.ntx, pg.nty, b.nframes);
            const size_t lds = (size_t)pg.lds_bytes;
            switch (pl.variant - PV_PYRAMID0) {
                case 0: hipLaunchKernelGGL((k_pyramid<false, false>), grid, dim3(256), lds, stream, b, pl.index); break;
                case 1: hipLaunchKernelGGL((k_pyramid<true, false>), grid, dim3(256), lds, stream, b, pl.index); break;
                case 2: hipLaunchKernelGGL((k_pyramid<false, true>), grid, dim3(256), lds, stream, b, pl.index); break;
                default: hipLaunchKernelGGL((k_pyramid<true, true>), grid, dim3(256), lds, stream, b, pl.index); break;
            }
        } else if (pl.variant < PV_STRIP0) {
            const int l = pl.index;
            const LevelGeom& L = g.lv[l];
            const dim3 grid(frame_item_blocks(b, ((L.w + 255) / 256) * ((L.h + RZ_ROWS - 1) / RZ_ROWS)));
            const size_t lds = (size_t)L.rz_pitch * L.rz_rows;
            switch (pl.variant - PV_TILED0) {
                case 0: hipLaunchKernelGGL((k_resize<false, false>), grid, dim3(256), lds, stream, b, l); break;
                case 1: hipLaunchKernelGGL((k_resize<true, false>), grid, dim3(256), lds, stream, b, l); break;
                case 2: hipLaunchKernelGGL((k_resize<false, true>), grid, dim3(256), lds, stream, b, l); break;
                case 3: hipLaunchKernelGGL((k_resize<true, true>), grid, dim3(256), lds, stream, b, l); break;
                case 4: hipLaunchKernelGGL((k_resize_gather<false, false>), grid, dim3(256), lds, stream, b, l); break;
                case 5: hipLaunchKernelGGL((k_resize_gather<true, false>), grid, dim3(256), lds, stream, b, l); break;
                case 6: hipLaunchKernelGGL((k_resize_gather<false, true>), grid, dim3(256), lds, stream, b, l); break;
                default: hipLaunchKernelGGL((k_resize_gather<true, true>), grid, dim3(256), lds, stream, b, l); break;
            }
        } else {
            const bool gather = pl.variant >= PV_STRIP_GATHER0;
            switch (pl.variant - (gather ? PV_STRIP_GATHER0 : PV_STRIP0)) {
                case 1: launch_resize_strip<1>(b, pl.index, pl.sc, gather, stream); break;
                case 2: launch_resize_strip<2>(b, pl.index, pl.sc, gather, stream); break;
                case 3: launch_resize_strip<3>(b, pl.index, pl.sc, gather, stream); break;
                case 4: launch_resize_strip<4>(b, pl.index, pl.sc, gather, stream); break;
                default: launch_resize_strip<0>(b, pl.index, pl.sc, gather, stream); break;
            }
        }
        ORBX_LAUNCH_CHECK();
    }
    return ORBX_OK;
}

}  // namespace orbx
