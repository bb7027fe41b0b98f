// Geometry of k_resize_strip (k_pyramid.hip), written once for the host geometry and the kernel so that it can be checked on the CPU
// (tests/_probe/resize_strip_host.cpp), as orb_math.h serves k_fast.hip.
//
// A workgroup produces a STRIP: rows_out consecutive output rows of a level across its whole width.  The source rows it needs,
// r0 = ty[by0].sy0 .. r1 = ty[by1].sy1 of the level below, are ONE byte range of that plane, [r0 * stride, r1 * stride + readable):
// `stride` is the source's row stride (the plane stride for levels >= 2, the caller's pitch for level 1) and `readable` the bytes of a
// row that may be read (the plane stride, or what include/orbx.h promises of a pitched row).  The range is staged in LDS as a flat list
// of 16-byte chunks, chunk q at LDS offset 16 q, so the LDS tile has the source's pitch: source byte (sy, x) lies at (sy - r0) * stride + x.
#pragma once
#include <stdint.h>

#include "orb_math.h"

namespace orbx {

constexpr int RZS_WG_PER_CU = 8;                                // workgroups per CU the LDS budget is sized for (six, five and four were slower: NOTES.md section 27)
constexpr int RZS_LDS_BUDGET = 160 * 1024 / RZS_WG_PER_CU;      // LDS bytes a strip may take (tile + slack)
constexpr int RZS_ROWS_MIN = 12, RZS_ROWS_CAP = 48;             // rows_out: the largest multiple of 4 in [MIN, CAP] whose strips fit the budget.  (MIN: strips of 8 rows stage 11 source
                                                                // rows for 8 and lost to the tiled form on the 1080p levels 2 and 3; 12 rows and more won: profiles/resize_strip_ab.json)
constexpr int RZS_SLACK = 16;                                   // bytes behind the tile: the windowed form reads three aligned dwords from a lane's first tap
constexpr int RZS_ROWPAR_MAX = 32;                              // a remainder group of at most this many dword columns is processed row-parallel

// form of a level's resize (orbx_debug_resize_form)
enum { RZ_FORM_TILED = 0, RZ_FORM_STRIP = 1, RZ_FORM_FUSED = 2 };

// bytes of a source row that may be read: the whole row stride of a pyramid plane; of a caller's frame min(pitch, w rounded up to 16)
ORBX_HD long long rzs_readable(bool src_is_level0, long long stride, int src_w) {
    if (!src_is_level0) return stride;
    const long long w16 = (long long)((src_w + 15) & ~15);
    return stride < w16 ? stride : w16;
}

struct StripSpan {
    int by0, by1;          // output rows of the strip (inclusive)
    int r0, r1;            // source rows it reads (inclusive)
    long long bytes;       // staged range: [r0 * stride, r0 * stride + bytes)
    long long chunks;      // whole 16-byte chunks of it (LDS-DMA)
    int tail_dwords;       // dwords behind the last whole chunk (0 .. 3; plain loads: a chunk is never fetched past the range's end)
    long long lds_bytes;   // tile rounded up to whole chunks + RZS_SLACK
};

// strip `strip` of a level of `h` rows; ty: its row table (sy0 / sy1 of every output row, monotone)
template <class RY>
ORBX_HD StripSpan rzs_span(const RY* ty, int h, int rows_out, int strip, long long stride, long long readable) {
    StripSpan s;
    s.by0 = strip * rows_out;
    s.by1 = imin(s.by0 + rows_out - 1, h - 1);
    s.r0 = ty[s.by0].sy0;
    s.r1 = ty[s.by1].sy1;
    s.bytes = (long long)(s.r1 - s.r0) * stride + readable;
    s.chunks = s.bytes >> 4;
    s.tail_dwords = (int)(s.bytes & 15) >> 2;
    s.lds_bytes = ((s.bytes + 15) & ~15ll) + RZS_SLACK;
    return s;
}

ORBX_HD int rzs_strips(int h, int rows_out) { return (h + rows_out - 1) / rows_out; }

// LDS bytes of a level's largest strip
template <class RY>
inline long long rzs_lds_bytes(const RY* ty, int h, int rows_out, long long stride, long long readable) {
    long long m = 0;
    for (int s = 0; s < rzs_strips(h, rows_out); s++) {
        const long long v = rzs_span(ty, h, rows_out, s, stride, readable).lds_bytes;
        m = v > m ? v : m;
    }
    return m;
}

// rows_out of a level: the largest multiple of 4 up to `cap` whose strips fit `budget`, 0 when not even RZS_ROWS_MIN rows do
template <class RY>
inline int rzs_pick_rows(const RY* ty, int h, long long stride, long long readable, int budget = RZS_LDS_BUDGET, int cap = RZS_ROWS_CAP) {
    for (int r = cap & ~3; r >= RZS_ROWS_MIN; r -= 4)
        if (rzs_lds_bytes(ty, h, r, stride, readable) <= (long long)budget) return r;
    return 0;
}

// ---- lane maps.  A lane produces one dword column (4 output pixels).  The level's dword columns are cut into groups of 64; every wave
// walks all groups for its rows_out / 4 consecutive output rows (row j of wave v: by0 + v * rows_out / 4 + j).  A last group of at most
// RZS_ROWPAR_MAX columns is row-parallel: the wave's lanes hold (column, row) pairs, 2^shift column slots x 64 >> shift rows per pass.
ORBX_HD int rzs_dword_cols(int w) { return (w + 3) >> 2; }
ORBX_HD int rzs_groups(int w) { return (rzs_dword_cols(w) + 63) >> 6; }
ORBX_HD int rzs_rem_cols(int w) { return rzs_dword_cols(w) - 64 * (rzs_groups(w) - 1); }     // columns of the last group (1 .. 64)
ORBX_HD bool rzs_rowpar(int w) { return rzs_rem_cols(w) <= RZS_ROWPAR_MAX; }
ORBX_HD int rzs_rowpar_shift(int rem) {     // log2 of the column slots: the smallest power of two >= rem
    int s = 0;
    while ((1 << s) < rem) s++;
    return s;
}
// looped group g: the lane's dword column (it works when 4 * column < w)
ORBX_HD int rzs_loop_col(int g, int lane) { return 64 * g + lane; }
// row-parallel group g, pass p: the lane's dword column slot and its row j of the wave (it works when slot < rem and j < rows_out / 4)
ORBX_HD int rzs_rowpar_slot(int lane, int shift) { return lane & ((1 << shift) - 1); }
ORBX_HD int rzs_rowpar_row(int lane, int shift, int pass) { return pass * (64 >> shift) + (lane >> shift); }
// LDS byte offset of the first of the three aligned dwords a lane reads of source row sy, its first tap at column sx0
ORBX_HD long long rzs_window_off(int sy, int r0, long long stride, int sx0) { return (long long)(sy - r0) * stride + (sx0 & ~3); }

}  // namespace orbx
