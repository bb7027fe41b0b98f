// Colour -> gray conversion in front of the extractor (include/orbx.h: orbx_to_gray_device and the *_color forms): what
// Tracking::GrabImage does with cvtColor(..., CV_RGB2GRAY / CV_BGR2GRAY) before it builds the Frame (reference src/Tracking.cc:185-195).
//
// The arithmetic is OpenCV 2.4's RGB2Gray<uchar> table path (imgproc/src/color.cpp): gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14 in
// integers (its three 256-entry tables hold exactly these products, the rounding constant folded into the blue one).  A 4-channel
// pixel's fourth byte is ignored, as in CV_RGBA2GRAY / CV_BGRA2GRAY.
//
// The kernel is a byte stream: one lane owns 16 consecutive pixels of one row.  In the aligned form (every base and stride a multiple
// of 16) it reads them with CH 16-byte loads (48 bytes of RGB, 64 of RGBA) and writes one 16-byte gray vector; otherwise, and for the
// last partial chunk of a row, it reads and writes byte by byte.  Exactly w * CH bytes of each source row are read and exactly w bytes
// of each gray row are written.
#include <algorithm>

#include "orbx_launch.h"

namespace orbx {

__device__ __forceinline__ uint32_t gray_of(uint32_t r, uint32_t g, uint32_t b) { return (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14; }

// byte k (a compile-time constant after unrolling) of a run of dwords
template <int N>
__device__ __forceinline__ uint32_t byte_at(const uint32_t (&d)[N], int k) { return (d[k >> 2] >> (8 * (k & 3))) & 255u; }

template <int CH, bool BGR>
__device__ __forceinline__ uint32_t pixel_gray(uint32_t c0, uint32_t c1, uint32_t c2) {
    if constexpr (CH == 1) return c0;
    else if constexpr (BGR) return gray_of(c2, c1, c0);
    else return gray_of(c0, c1, c2);
}

// GATHER: frame f's source is a.tab[f] (base and row stride; a DEVICE table read through the constant address space, so the entry
// arrives with one scalar load per wave, as level0_src does).  blockIdx.y = frame - a.f0.
template <int CH, bool BGR, bool ALIGNED, bool GATHER>
__global__ __launch_bounds__(256) void k_to_gray(ColorArgs a) {
    const unsigned item = blockIdx.x * 256u + threadIdx.x;
    if (item >= (unsigned)a.items) return;
    const int frame = a.f0 + (int)blockIdx.y;
    const unsigned row = item / (unsigned)a.cpr;
    const int x0 = (int)(item - row * (unsigned)a.cpr) * 16;
    const uint8_t* src;
    long long srs;
    if constexpr (GATHER) {
        typedef const ImgSrc __attribute__((address_space(4)))* ctab_t;
        const ctab_t e = (ctab_t)(uintptr_t)a.tab + frame;
        src = e->data;
        srs = e->row_stride;
    } else {
        src = a.src + (long long)frame * a.src_frame_stride;
        srs = a.src_row_stride;
    }
    src += (long long)row * srs + (long long)x0 * CH;
    const long long doff = (long long)frame * a.dst_frame_stride + (long long)row * a.dst_row_stride + x0;
    uint8_t* dst = a.dst + doff;
    uint8_t* dst2 = a.dst2 ? a.dst2 + doff : nullptr;
    const int n = min(16, a.w - x0);
    if (ALIGNED && n == 16) {
        uint32_t d[4 * CH];
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const uint4 v = reinterpret_cast<const uint4*>(src)[k];
            d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
        }
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t c0 = byte_at(d, CH * i);
            uint32_t c1 = 0, c2 = 0;
            if constexpr (CH > 1) { c1 = byte_at(d, CH * i + 1); c2 = byte_at(d, CH * i + 2); }
            o[i >> 2] |= pixel_gray<CH, BGR>(c0, c1, c2) << (8 * (i & 3));
        }
        const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<uint4*>(dst) = v;
        if (dst2) *reinterpret_cast<uint4*>(dst2) = v;
    } else {
        for (int i = 0; i < n; i++) {
            const uint8_t* p = src + i * CH;
            uint32_t c1 = 0, c2 = 0;
            if constexpr (CH > 1) { c1 = p[1]; c2 = p[2]; }
            const uint32_t gv = pixel_gray<CH, BGR>(p[0], c1, c2);
            dst[i] = (uint8_t)gv;
            if (dst2) dst2[i] = (uint8_t)gv;
        }
    }
}

// The variant of (format, alignment, source form): orbx_launch.h's ColorVariant numbering, which counts on the formats being 0 .. 4 in
// the order gray, RGB, BGR, RGBA, BGRA.  Also the case labels of launch_to_gray's switch.
static_assert(ORBX_PIX_GRAY8 == 0 && ORBX_PIX_RGB8 == 1 && ORBX_PIX_BGR8 == 2 && ORBX_PIX_RGBA8 == 3 && ORBX_PIX_BGRA8 == 4, "ColorVariant numbering");
constexpr int color_variant(int fmt, bool aligned, bool gather) {
    return (gather ? CV_GATHER0 + 2 * (fmt - ORBX_PIX_RGB8) : 2 * fmt) + (aligned ? 1 : 0);
}
static_assert(color_variant(ORBX_PIX_BGRA8, true, false) + 1 == CV_GATHER0 && color_variant(ORBX_PIX_BGRA8, true, true) + 1 == CV_COUNT, "ColorVariant numbering");
// fmt: ORBX_PIX_*; a table of gray frames has no conversion (the pipeline reads it itself): id -1
StagePlan plan_to_gray(const ColorArgs& a, int fmt) {
    if (pix_channels(fmt) == 0 || (a.tab && fmt == ORBX_PIX_GRAY8)) return StagePlan();
    const unsigned long long bits = (a.tab ? a.tab_bits : ((uintptr_t)a.src | (unsigned long long)a.src_row_stride | (unsigned long long)a.src_frame_stride)) |
                                    (uintptr_t)a.dst | (uintptr_t)a.dst2 | (unsigned long long)a.dst_row_stride | (unsigned long long)a.dst_frame_stride;
    return stage_plan(color_variant(fmt, (bits & 15) == 0, a.tab != nullptr));
}
const char* color_variant_name(int id) {
    static const char* const names[CV_COUNT] = {
        "k_to_gray<1, false, false, false>", "k_to_gray<1, false, true, false>", "k_to_gray<3, false, false, false>", "k_to_gray<3, false, true, false>",
        "k_to_gray<3, true, false, false>", "k_to_gray<3, true, true, false>", "k_to_gray<4, false, false, false>", "k_to_gray<4, false, true, false>",
        "k_to_gray<4, true, false, false>", "k_to_gray<4, true, true, false>",
        "k_to_gray<3, false, false, true>", "k_to_gray<3, false, true, true>", "k_to_gray<3, true, false, true>", "k_to_gray<3, true, true, true>",
        "k_to_gray<4, false, false, true>", "k_to_gray<4, false, true, true>", "k_to_gray<4, true, false, true>", "k_to_gray<4, true, true, true>"};
    return id >= 0 && id < CV_COUNT ? names[id] : "?";
}

int launch_to_gray(const ColorArgs& args, int nframes, int fmt, hipStream_t stream, StagePlan* report) {
    if (report) *report = StagePlan();
    if (nframes <= 0 || args.w <= 0 || args.h <= 0) return ORBX_OK;
    ColorArgs a = args;
    a.cpr = (a.w + 15) / 16;
    const long long items = (long long)a.cpr * a.h;
    if (items >= (1ll << 31) - 256) return ORBX_ERR_ARG;
    a.items = (int)items;
    const StagePlan plan = plan_to_gray(a, fmt);
    if (plan.id < 0) return ORBX_ERR_ARG;
    constexpr int MAX_Y = 32768;                         // frames per launch (grid.y)
    for (int f0 = 0; f0 < nframes; f0 += MAX_Y) {
        a.f0 = args.f0 + f0;
        const dim3 grid((unsigned)((items + 255) / 256), (unsigned)std::min(MAX_Y, nframes - f0));
#define ORBX_TO_GRAY_CASES(FMT, CH, BGR, GA)                                                                                                            \
    case color_variant(FMT, false, GA): hipLaunchKernelGGL((k_to_gray<CH, BGR, false, GA>), grid, dim3(256), 0, stream, a); break;                \
    case color_variant(FMT, true, GA): hipLaunchKernelGGL((k_to_gray<CH, BGR, true, GA>), grid, dim3(256), 0, stream, a); break;
        switch (plan.id) {
            ORBX_TO_GRAY_CASES(ORBX_PIX_GRAY8, 1, false, false)
            ORBX_TO_GRAY_CASES(ORBX_PIX_RGB8, 3, false, false) ORBX_TO_GRAY_CASES(ORBX_PIX_BGR8, 3, true, false)
            ORBX_TO_GRAY_CASES(ORBX_PIX_RGBA8, 4, false, false) ORBX_TO_GRAY_CASES(ORBX_PIX_BGRA8, 4, true, false)
            ORBX_TO_GRAY_CASES(ORBX_PIX_RGB8, 3, false, true) ORBX_TO_GRAY_CASES(ORBX_PIX_BGR8, 3, true, true)
            ORBX_TO_GRAY_CASES(ORBX_PIX_RGBA8, 4, false, true) ORBX_TO_GRAY_CASES(ORBX_PIX_BGRA8, 4, true, true)
            default: return ORBX_ERR_ARG;
        }
#undef ORBX_TO_GRAY_CASES
        ORBX_LAUNCH_CHECK();
    }
    if (report) *report = plan;
    return ORBX_OK;
}

}  // namespace orbx
