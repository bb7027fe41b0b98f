// Host-side pieces the kernel translation units share: the launch check, the per-stage timers' scope, and the per-stage launchers that
// launch_extract (orbx_launch.hip) strings together.  One translation unit per stage since round 6 (k_pyramid.hip, k_fast.hip, k_select.hip,
// k_blur.hip, k_describe.hip, k_describe_od.hip); orbx_build_id() hashes all of them.
#pragma once
#include <hip/hip_runtime.h>

#include "orbx_internal.h"

namespace orbx {

#define ORBX_LAUNCH_CHECK()                                   \
    do {                                                      \
        hipError_t e_ = hipGetLastError();                    \
        if (e_ != hipSuccess) return ORBX_ERR_DEVICE;         \
    } while (0)

constexpr size_t INGEST_MAX_BYTES = (size_t)512 << 10;   // the one-frame call: staged frames up to this size are fetched by k_ingest
constexpr int PYR_FUSED_MAX_FRAMES = 32;      // launch groups below this take the latency-oriented sequence: fused pyramid cones, FAST + blur in one launch, one selection class

struct StageScope {   // records (start, stop) events around one stage when timing is on
    StageTimer* t; hipStream_t s; int stage;
    StageScope(StageTimer* t_, hipStream_t s_, int stage_) : t(t_ && t_->enabled ? t_ : nullptr), s(s_), stage(stage_) {
        if (t) { hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, s); t->pool.push_back(e); } else t = nullptr; }
    }
    ~StageScope() {
        if (t) { hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, s); t->pool.push_back(e); t->pool_stage.push_back(stage); } else { (void)hipEventDestroy(t->pool.back()); t->pool.pop_back(); } }
    }
};

// ------------------------------------------------------------------------------------ launch variants
// Every launch site picks one template instantiation per launch from the call form and the geometry.  The choice is a pure host function
// (plan_*), the launch switches on its result, and the same result is what the diagnostics report (orbx_debug_launch_variant) and what the
// device-free planning call predicts (orbx_debug_plan): the conditions stand once per stage.  An enum value per instantiation a launch site
// can reach, named by the kernel and its template arguments; *_COUNT is what orbx_debug_variant_count returns.
enum VStage { VS_COLOR = ORBX_VS_COLOR, VS_INGEST, VS_PYRAMID, VS_FAST, VS_QUOTA, VS_CELL_SELECT, VS_LEVEL_SELECT, VS_BLUR, VS_DESCRIBE, VS_COUNT };
static_assert(VS_COUNT == ORBX_VS_COUNT, "include/orbx.h names the stages");

// k_to_gray<CH, BGR, ALIGNED, GATHER>: contiguous source 2 * format + aligned (ORBX_PIX_GRAY8 .. BGRA8), then the table forms of the four
// colour formats (a gray table is read by the pipeline itself: no entry point converts one)
enum ColorVariant { CV_GATHER0 = 10, CV_COUNT = 18 };
// k_pyramid<ALIGNED, GATHER> (bit 0 aligned, bit 1 gather), the tiled k_resize / k_resize_gather <ALIGNED, WINDOW> (bit 0 aligned, bit 1 window,
// bit 2 gather), the strips k_resize<NG> / k_resize_gather<NG> (NG 0 .. 4)
enum PyramidVariant { PV_PYRAMID0 = 0, PV_TILED0 = 4, PV_STRIP0 = 12, PV_STRIP_GATHER0 = 17, PV_COUNT = 22 };
// k_fast_cells / k_fast_cells_gather / k_fast_blur / k_fast_blur_gather: bit 0 aligned, bit 1 small shape, bit 2 gather, bit 3 blur in the launch
enum FastVariant { FV_ALIGNED = 1, FV_SMALL = 2, FV_GATHER = 4, FV_BLUR = 8, FV_COUNT = 16 };
enum QuotaVariant { QV_QUOTA = 0, QV_COUNT };
enum CellSelectVariant { CS_SELECT = 0, CS_SELECT_GATHER, CS_LONG, CS_LONG_GATHER, CS_COUNT };     // (the long kernels follow the short ones: mask only)
enum LevelSelectVariant { LS_ONE = 0, LS_CHUNKED, LS_COUNT };
// k_blur / k_blur_gather <ALIGNED, BLUR_ROWS> (bit 0 aligned, bit 1 gather), k_blur_mfma.  (Launch groups below PYR_FUSED_MAX_FRAMES blur inside
// k_fast_blur or per keypoint window: no stand-alone launch with BLUR_ROWS_SMALL exists.)
enum BlurVariant { BV_ALIGNED = 1, BV_GATHER = 2, BV_MFMA = 4, BV_COUNT };
// k_describe / k_describe_gather / k_describe_od / k_describe_od_gather <FMA>: bit 0 FMA, bit 1 gather, bit 2 blur on demand
enum DescribeVariant { DV_FMA = 1, DV_GATHER = 2, DV_OD = 4, DV_COUNT = 8 };

// What one stage of a launch group launches: the variant of its first launch (-1: the stage launches nothing), every variant it launches as a
// bit mask, and ORBX_VF_* flags.
struct StagePlan { int id = -1; unsigned flags = 0; unsigned long long mask = 0; };
inline StagePlan stage_plan(int id, unsigned flags = 0) { StagePlan s; s.id = id; s.flags = flags; s.mask = 1ull << id; return s; }
// One launch of the pyramid stage: a cone of k_pyramid (index: the PyrGroup) or one level of k_resize (index: the level; sc: its strip form)
struct PyramidLaunch { int variant, index; StripChoice sc; };
struct PyramidPlan { int n = 0; PyramidLaunch launch[MAX_LEVELS]; };
struct LaunchPlan {
    StagePlan st[VS_COUNT];
    PyramidPlan pyr;
    bool on_demand = false, overlap = false, fuse_blur = false;
};

int variant_count(int stage);                       // orbx_launch.hip
const char* variant_name(int stage, int id);        // ... "?" for an id outside the stage's enum
// The decisions of one launch group (orbx_launch.hip); have_side: a side stream exists for the blur.  Stages a call does not reach (early stop,
// phases) stay at id -1, as do VS_COLOR / VS_INGEST, which belong to the entry points (plan_to_gray, plan_ingest).
LaunchPlan plan_extract(const Batch& b, const HostGeom& hg, int stop_after, bool have_side, int phases);
PyramidPlan plan_pyramid(const Batch& b, const HostGeom& hg);                                  // k_pyramid.hip
StagePlan plan_fast(const Batch& b, const HostGeom& hg, bool fuse_blur);                       // k_fast.hip
StagePlan plan_quota(const HostGeom& hg);                                                      // k_select.hip
StagePlan plan_cell_select(const Batch& b, const HostGeom& hg);
StagePlan plan_level_select(const Batch& b, const HostGeom& hg);
StagePlan plan_blur(const Batch& b, const HostGeom& hg);                                       // k_blur.hip
StagePlan plan_describe(const Batch& b, const HostGeom& hg, bool on_demand);                   // k_describe.hip
StagePlan plan_to_gray(const ColorArgs& a, int fmt);                                           // k_color.hip (id -1: no such launch)
StagePlan plan_ingest(size_t frame_bytes, bool zero_copy);                                     // orbx_launch.hip
const char* pyramid_variant_name(int id);
const char* fast_variant_name(int id);
const char* cell_select_variant_name(int id);
const char* level_select_variant_name(int id);
const char* blur_variant_name(int id);
const char* describe_variant_name(int id);
const char* color_variant_name(int id);

int launch_pyramid(const Batch& b, const PyramidPlan& plan, hipStream_t stream);                                // k_pyramid.hip
int launch_fast(const Batch& b, const HostGeom& hg, hipStream_t stream, const StagePlan& plan);               // k_fast.hip
int launch_quota(const Batch& b, const HostGeom& hg, hipStream_t stream, const StagePlan& plan);              // k_select.hip
int launch_cell_select(const Batch& b, const HostGeom& hg, hipStream_t stream, const StagePlan& plan);
int launch_level_select(const Batch& b, const HostGeom& hg, hipStream_t stream, const StagePlan& plan);
int launch_blur(const Batch& b, const HostGeom& hg, hipStream_t stream, const StagePlan& plan);               // k_blur.hip
int launch_describe(const Batch& b, const HostGeom& hg, hipStream_t stream, const StagePlan& plan);           // k_describe.hip, k_describe_od.hip
int launch_describe_od(const Batch& b, const HostGeom& hg, hipStream_t stream, int variant);
// (k_describe_od.hip: describe_od_supported — orbx_internal.h)

}  // namespace orbx
