// Host check of k_resize_strip's geometry (orb_slam_amd/csrc/k_resize_strip.h) over random image geometries, without a GPU: the real
// build_geometry / resize_strip_choice (orbx_geometry.hip is host arithmetic only; compiled here against tests/_probe/hip_stub) and, for every
// eligible level and strip, the kernel's lane maps replayed on the CPU.  Stand-alone: may be built with -fsanitize=address,undefined.
//   resize_strip_host [geometries] [seed]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_geometry.hip"

using namespace orbx;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 16);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

static long n_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (n_fail++ < 20) { printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the rule, restated: windowed form, 4-byte aligned source, and the largest multiple of 4 in [12, 48] whose largest strip fits the budget
// (12, not 8: strips of 8 rows measured slower than the tiled form on 1080p levels; NOTES.md section 27, profiles/resize_strip_ab.json)
static int expect_rows(const HostGeom& hg, int l, long long stride, unsigned long long bits, long long& lds_out) {
    const LevelGeom& L = hg.g.lv[l];
    const LevelGeom& P = hg.g.lv[l - 1];
    lds_out = 0;
    if (!L.rz_window) return 0;
    long long readable = P.stride;
    if (l == 1) {
        if ((bits & 3) || (stride & 3) || stride < P.w) return 0;
        readable = std::min<long long>(stride, (P.w + 15) & ~15);
    } else stride = P.stride;
    const ResizeY* ty = hg.taby.data() + L.taby_off;
    for (int R = 48; R >= 12; R -= 4) {
        long long m = 0;
        for (int y0 = 0; y0 < L.h; y0 += R) {
            const int y1 = std::min(y0 + R - 1, L.h - 1);
            const long long bytes = (long long)(ty[y1].sy1 - ty[y0].sy0) * stride + readable;
            m = std::max(m, (bytes + 15) / 16 * 16 + 16);
        }
        if (m <= 160 * 1024 / 8) { lds_out = m; return R; }
    }
    return 0;
}

static long n_levels = 0, n_strip_levels = 0, n_strips = 0, n_rowpar = 0, n_tail = 0;

static void check_level(const HostGeom& hg, int l, long long stride_in, unsigned long long bits) {
    const LevelGeom& L = hg.g.lv[l];
    const LevelGeom& P = hg.g.lv[l - 1];
    const StripChoice sc = resize_strip_choice(hg, l, stride_in, bits);
    long long want_lds;
    const int want = expect_rows(hg, l, stride_in, bits, want_lds);
    n_levels++;
    CHECK(sc.rows_out == want && sc.lds_bytes == want_lds, "level %d w %d h %d stride %lld bits %llu: rows %d (want %d) lds %d (want %lld)", l, L.w, L.h, stride_in, bits, sc.rows_out, want, sc.lds_bytes, want_lds);
    if (!sc.rows_out) return;
    n_strip_levels++;
    const long long stride = l == 1 ? stride_in : P.stride;
    const long long readable = rzs_readable(l == 1, stride, P.w);
    CHECK(sc.lds_bytes <= RZS_LDS_BUDGET && sc.rows_out >= 12 && sc.rows_out <= 48 && sc.rows_out % 4 == 0, "budget: rows %d lds %d", sc.rows_out, sc.lds_bytes);
    CHECK(readable >= P.w && readable <= stride && readable % 4 == 0, "readable %lld of w %d stride %lld", readable, P.w, stride);
    const ResizeX* tx = hg.tabx.data() + L.tabx_off;
    const ResizeY* ty = hg.taby.data() + L.taby_off;
    const int R = sc.rows_out, RPW = R / 4, ndw = rzs_dword_cols(L.w), ngroups = rzs_groups(L.w), rem = rzs_rem_cols(L.w);
    const bool rowpar = rzs_rowpar(L.w);
    const int shift = rzs_rowpar_shift(rem);
    CHECK(rem >= 1 && rem <= 64 && 64 * (ngroups - 1) + rem == ndw && (!rowpar || ((1 << shift) >= rem && (1 << shift) <= 32)), "groups: ndw %d ngroups %d rem %d shift %d", ndw, ngroups, rem, shift);
    if (rowpar) n_rowpar++;
    // column side (the same for every strip): every dword column is some lane's, once; its window and its selected bytes
    std::vector<int> col_seen(ndw, 0), col_wa(ndw, 0);
    int wa_max = 0, sel_max = 0;        // furthest window start / furthest selected byte column
    auto lane_col = [&](int dcol) {
        ResizeX rx[4];
        for (int k = 0; k < 4; k++) rx[k] = tx[std::min(4 * dcol + k, L.w - 1)];
        const int w0 = rx[0].sx;
        for (int k = 0; k < 4; k++) {
            CHECK(rx[k].sx >= w0 && rx[k].sx1 >= rx[k].sx && rx[k].sx1 - w0 <= 7, "window: level %d dcol %d tap %d sx %d sx1 %d w0 %d", l, dcol, k, rx[k].sx, rx[k].sx1, w0);
            CHECK(rx[k].sx1 <= P.w - 1, "tap beyond the source row");
            sel_max = std::max(sel_max, (int)rx[k].sx1);
        }
        wa_max = std::max(wa_max, w0 & ~3);
        col_seen[dcol]++;
    };
    for (int gi = 0; gi < ngroups; gi++) {
        if (gi == ngroups - 1 && rowpar) {
            // every (slot, row) pair of a wave is held by exactly one (lane, pass)
            std::vector<int> pair_seen((size_t)rem * RPW, 0);
            for (int pass = 0; pass * (64 >> shift) < RPW; pass++)
                for (int lane = 0; lane < 64; lane++) {
                    const int slot = rzs_rowpar_slot(lane, shift), j = rzs_rowpar_row(lane, shift, pass);
                    if (slot < rem && j < RPW) pair_seen[(size_t)j * rem + slot]++;
                }
            for (int v : pair_seen) CHECK(v == 1, "row-parallel pair held %d times (rem %d RPW %d)", v, rem, RPW);
            for (int slot = 0; slot < rem; slot++) lane_col(64 * gi + slot);
        } else
            for (int lane = 0; lane < 64; lane++) {
                const int dcol = rzs_loop_col(gi, lane);
                if (4 * dcol < L.w) lane_col(dcol);
            }
    }
    for (int d = 0; d < ndw; d++) CHECK(col_seen[d] == 1, "dword column %d of %d produced %d times", d, ndw, col_seen[d]);
    // row side, strip by strip
    const int nstrips = rzs_strips(L.h, R);
    int next_row = 0;
    for (int s = 0; s < nstrips; s++) {
        const StripSpan sp = rzs_span(ty, L.h, R, s, stride, readable);
        n_strips++;
        CHECK(sp.by0 == next_row && sp.by1 >= sp.by0 && sp.by1 < L.h, "strips partition the rows: strip %d rows %d..%d, expected start %d", s, sp.by0, sp.by1, next_row);
        next_row = sp.by1 + 1;
        // the staged range [r0 * stride, r0 * stride + bytes) inside [r0 * stride, r1 * stride + readable), itself inside the frame's promised bytes
        CHECK(sp.r0 >= 0 && sp.r1 >= sp.r0 && sp.r1 <= P.h - 1, "source rows %d..%d of %d", sp.r0, sp.r1, P.h);
        CHECK(sp.bytes == (long long)(sp.r1 - sp.r0) * stride + readable, "range bytes");
        CHECK(16 * sp.chunks + 4 * sp.tail_dwords == sp.bytes && sp.tail_dwords >= 0 && sp.tail_dwords <= 3, "chunks %lld tail %d bytes %lld", sp.chunks, sp.tail_dwords, sp.bytes);
        CHECK((long long)sp.r0 * stride + sp.bytes <= (long long)(P.h - 1) * stride + readable, "range leaves the frame");
        CHECK(sp.lds_bytes <= sc.lds_bytes && sp.lds_bytes >= 16 * sp.chunks + 4 * sp.tail_dwords + RZS_SLACK, "lds %lld of %d", sp.lds_bytes, sc.lds_bytes);
        if (sp.tail_dwords) n_tail++;
        // every output row of the strip is some wave's row j, once; its two source rows lie inside the staged rows
        int rows_seen = 0;
        for (int v = 0; v < 4; v++)
            for (int j = 0; j < RPW; j++) {
                const int dy = sp.by0 + v * RPW + j;
                if (dy >= L.h) continue;
                CHECK(dy <= sp.by1, "row %d beyond the strip %d..%d", dy, sp.by0, sp.by1);
                rows_seen++;
                for (int sy : {(int)ty[dy].sy0, (int)ty[dy].sy1}) {
                    CHECK(sy >= sp.r0 && sy <= sp.r1, "source row %d outside %d..%d", sy, sp.r0, sp.r1);
                    // the three-dword window of the furthest lane stays inside the allocation; the furthest selected byte inside the staged bytes
                    CHECK(rzs_window_off(sy, sp.r0, stride, wa_max) + 12 <= sp.lds_bytes, "window read leaves the LDS tile: row %d wa %d lds %lld", sy, wa_max, sp.lds_bytes);
                    CHECK((long long)(sy - sp.r0) * stride + sel_max < sp.bytes, "selected byte not staged");
                }
            }
        CHECK(rows_seen == sp.by1 - sp.by0 + 1, "strip %d: %d rows produced of %d", s, rows_seen, sp.by1 - sp.by0 + 1);
    }
    CHECK(next_row == L.h, "strips end at row %d of %d", next_row, L.h);
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 3000;
    if (argc > 2) rng_state ^= (unsigned long long)atoll(argv[2]) * 0x9E3779B97F4A7C15ull;
    int built = 0;
    for (int it = 0; it < n; it++) {
        orbx_params p;
        memset(&p, 0, sizeof(p));
        p.score_type = ORBX_FAST_SCORE;
        p.fast_th = 20;
        p.max_batch = 1;
        p.blur_rounding = ORBX_BLUR_X86_SSE2;
        // sizes: uniform, with every fourth geometry small (narrow levels: one group, tiny remainders)
        const bool small = it % 4 == 3;
        const int w = small ? rnd_in(64, 400) : rnd_in(64, 2000), h = small ? rnd_in(44, 300) : rnd_in(44, 1200);
        p.scale_factor = 1.05f + (float)(rnd() % 6501) * 1e-4f;
        p.nlevels = rnd_in(2, 8);
        p.nfeatures = rnd_in(100, 2000);
        HostGeom hg;
        std::string err;
        if (build_geometry(p, w, h, hg, err) != ORBX_OK) continue;      // (levels too small for the border, degenerate grids: no geometry at all)
        built++;
        for (int l = 1; l < hg.g.nlevels; l++) {
            if (l >= 2) { check_level(hg, l, 0, 0); continue; }
            // level 1: the caller's pitch and alignment
            const long long pitches[] = {w, w + 4, w + 60, (w + 15) & ~15, (w + 63) & ~63, w + 1, w + 2, w + 4 * rnd_in(0, 64), (long long)w + rnd_in(0, 4000), w - 4};
            for (long long pitch : pitches) {
                check_level(hg, l, pitch, 0);
                check_level(hg, l, pitch, 1 + rnd() % 3);      // a byte-offset base
            }
            // what the geometry stores for level 1 is the packed-pitch choice
            const StripChoice sc = resize_strip_choice(hg, 1, w, 0);
            CHECK(hg.g.lv[1].rs_rows == sc.rows_out && hg.g.lv[1].rs_lds == sc.lds_bytes, "stored level-1 choice");
        }
        for (int l = 2; l < hg.g.nlevels; l++) {
            const StripChoice sc = resize_strip_choice(hg, l, 12345, 7);   // (ignored for levels >= 2)
            CHECK(hg.g.lv[l].rs_rows == sc.rows_out && hg.g.lv[l].rs_lds == sc.lds_bytes, "stored choice of level %d", l);
        }
    }
    printf("geometries %d built %d levels %ld strip_levels %ld strips %ld rowpar_levels %ld tail_strips %ld failures %ld\n", n, built, n_levels, n_strip_levels, n_strips, n_rowpar, n_tail, n_fail);
    if (n_fail == 0 && built > n / 2 && n_strip_levels > 0 && n_rowpar > 0 && n_tail > 0) { printf("resize strip host ok\n"); return 0; }
    return 1;
}
