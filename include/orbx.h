/* orbx.h — C ABI of the MI355X-native ORB front-end (liborbx.so).
 *
 * Drop-in boundary for ORB_SLAM's per-frame hot path.  Every entry point uses plain pointers and
 * sizes only (no C++/torch types) so the reference's C++ classes — or any FFI — can bind it.
 * The reference-side shim that keeps `ORB_SLAM::ORBextractor` / `ORB_SLAM::ORBmatcher` source
 * compatible lives in orb_slam_amd/cpp/ (see INTEGRATION.md).
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   orbx_create / orbx_destroy      <- ORBextractor::ORBextractor(int,float,int,int,int)   include/ORBextractor.h:38, src/ORBextractor.cc:457-511
 *   orbx_extract                    <- ORBextractor::operator()(InputArray,InputArray,vector<KeyPoint>&,OutputArray)
 *                                                                                           include/ORBextractor.h:43-45, src/ORBextractor.cc:718-779
 *   orbx_get_levels                 <- ORBextractor::GetLevels()                           include/ORBextractor.h:47-48
 *   orbx_get_scale_factor           <- ORBextractor::GetScaleFactor()                      include/ORBextractor.h:50-51
 *   orbx_extract_batch_device       <- the same operator(), throughput form (device-resident frames, many per call)
 *   orbx_to_gray_device, orbx_extract_color, orbx_extract_batch_device_color, orbx_extract_batch_color
 *                                   <- Tracking::GrabImage's cvtColor(CV_RGB2GRAY / CV_BGR2GRAY) in front of Frame::Frame   src/Tracking.cc:185-195
 *   orbm_hamming256                 <- ORBmatcher::DescriptorDistance(const Mat&,const Mat&) include/ORBmatcher.h:44, src/ORBmatcher.cc:1794-1810
 *   orbm_match_top2[_masked][_device|_batch_device]
 *                                   <- the best / second-best scan shared by every ORBmatcher search
 *                                      (src/ORBmatcher.cc:87-111, :201-222, :454-474, :629-650, ...)
 *   orbm_match_top2_segments[_device]
 *                                   <- the same scan over a per-query candidate list (window / vocabulary node): "next" row N2
 *   orbm_distinctive[_device]       <- MapPoint::ComputeDistinctiveDescriptors(): N x N Hamming distances of a map point's observed
 *                                      descriptors, the one with the least median distance to the rest   src/MapPoint.cc:185-250 ("next" row N4)
 *   orbm_count_accepted             <- accept rule `best<=TH && (float)best < mfNNratio*(float)second` (src/ORBmatcher.cc:224-226)
 *
 * All compute runs in hand-written HIP kernels for gfx950.  There is NO CPU fallback: every
 * compute entry point returns ORBX_ERR_DEVICE when no usable GPU / kernel image is present.
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define ORBX_OK             0
#define ORBX_EMPTY          1   /* empty image: nothing done, outputs untouched (reference src/ORBextractor.cc:721-722) */
#define ORBX_ERR_ARG       -1
#define ORBX_ERR_DEVICE    -2   /* no GPU, HIP error, or kernel image missing */
#define ORBX_ERR_CAPACITY  -3   /* caller buffer or internal list too small; or an implementation limit the reference does not have
                                 * (a grid cell wider than 6500 px, > 16384 cells on a level — far outside ORB_SLAM's settings) */
#define ORBX_ERR_GEOMETRY  -4   /* image/grid geometry the reference itself cannot process (cv::Exception / div-by-zero there) */

/* ORBextractor::{HARRIS_SCORE, FAST_SCORE} (include/ORBextractor.h:36) */
#define ORBX_HARRIS_SCORE 0
#define ORBX_FAST_SCORE   1

/* GaussianBlur column rounding: what an x86-64 OpenCV 2.4 does (SSE2 column filter:
 * ties-to-even for x < (w & ~3), half-up for the scalar tail) or half-up everywhere (non-SIMD build) */
#define ORBX_BLUR_X86_SSE2 0
#define ORBX_BLUR_HALF_UP  1

/* How the two float expressions of src/ORBextractor.cc that a compiler may contract are evaluated:
 * `x*b + y*a`, `x*a - y*b` in computeOrbDescriptor (:165-166) and the Harris response (:118-119).
 *   ORBX_FP_ISO           unfused, one rounding per operation: the source text under ISO C++ rules = the reference built with
 *                         -ffp-contract=off, or for a CPU without FMA instructions (default; oracle/_ref, the golden fixtures)
 *   ORBX_FP_GCC_CONTRACT  fused where GCC fuses them under the reference's own flags (CMakeLists.txt:12-13: -O3 -march=native with
 *                         GCC's default -ffp-contract=fast, any x86 since 2013): fma(x,b,y*a), fma(x,a,-(y*b)),
 *                         fma(-(a+b), k*(a+b), fma(a,b,-(c*c))) — read off that build's object code (oracle/_ref_native).
 * The two differ in ~1 descriptor bit per 10^5 key points and in the last bits of ~30 % of the Harris responses
 * (tests/test_ref_pin_native.py).  orbx_default_params takes ORBX_FP_CONTRACT=1 from the environment. */
#define ORBX_FP_ISO          0
#define ORBX_FP_GCC_CONTRACT 1

/* identical to OpenCV 2.4's cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id */
typedef struct orbx_keypoint {
    float x, y;
    float size;
    float angle;
    float response;
    int32_t octave;
    int32_t class_id;
} orbx_keypoint;

typedef struct orbx_params {
    /* the five reference constructor arguments, same meaning and defaults (1000, 1.2f, 8, FAST_SCORE, 20) */
    int32_t nfeatures;
    float   scale_factor;
    int32_t nlevels;
    int32_t score_type;
    int32_t fast_th;
    /* device-side additions */
    int32_t device;         /* HIP device ordinal */
    int32_t max_batch;      /* frames processed per launch group by orbx_extract_batch_device (>=1) */
    int32_t blur_rounding;  /* ORBX_BLUR_* */
    int32_t fp_contract;    /* ORBX_FP_* (took the first reserved slot: a zeroed struct of an older caller means ORBX_FP_ISO) */
    int32_t reserved[7];    /* must be zero */
} orbx_params;

typedef struct orbx_extractor orbx_extractor;   /* opaque; not thread-safe (same as the reference instance) */

void  orbx_default_params(orbx_params* p);
int   orbx_create(const orbx_params* p, orbx_extractor** out);
void  orbx_destroy(orbx_extractor* h);
int   orbx_get_levels(const orbx_extractor* h);
float orbx_get_scale_factor(const orbx_extractor* h);
/* upper bound on keypoints per frame (= sum of the per-level quotas; == nfeatures for sane parameters) */
int   orbx_max_keypoints(const orbx_extractor* h);
const char* orbx_last_error(const orbx_extractor* h);
/* 16 hex digits: hash of the kernel sources this library was built from (the Makefile passes it in).  bench.py compares it with
 * the hash recorded in profiles/traffic.json / valu_mix.json and refuses to replay counters measured on other kernels. */
const char* orbx_build_id(void);

/* One frame, host buffers (the operator() drop-in).  img: 8-bit single channel, `stride` bytes per row.
 * kps[cap], desc[cap*32] are caller buffers, cap >= orbx_max_keypoints().  *n_out = number of features.
 * Keypoint order, coordinates, angle, response, octave and descriptors are bit-identical to the
 * reference algorithm (see DESIGN.md "Parity").  Synchronous. */
int orbx_extract(orbx_extractor* h, const uint8_t* img, int w, int hgt, ptrdiff_t stride,
                 orbx_keypoint* kps, uint8_t* desc, int cap, int* n_out);

/* Throughput form.  d_imgs: DEVICE pointer to nframes frames, frame f at d_imgs + f*frame_stride,
 * rows `row_stride` bytes apart.  d_kps[nframes*cap], d_desc[nframes*cap*32], d_n[nframes]: DEVICE
 * buffers.  Work is enqueued on `stream` (a hipStream_t, may be NULL) and NOT synchronised.
 * d_status[nframes] (optional DEVICE int32 buffer) receives ORBX_OK / ORBX_ERR_CAPACITY per frame.
 * Pitched frames (row_stride > w): every row, the last row of the last frame included, must be readable up to
 * min(row_stride, w rounded up to 16) bytes — the kernels stage rows in whole 16-byte chunks (as a hipMallocPitch-style
 * buffer of row_stride x hgt bytes per frame guarantees).  Fastest when d_imgs, row_stride and frame_stride are multiples of
 * 16 (any alignment is accepted: bytes are then assembled on the fly). */
/* Temporal coherence is used for SPEED only, per frame slot: slot f of a launch group (frame f0 + f of a call, f < max_batch) remembers which
 * of its grid-cell bands took the reference's threshold-7 fallback (src/ORBextractor.cc:609-614) in the last launch groups and starts those at 7
 * right away.  Outputs never depend on it; a caller that keeps each camera / sequence in the same slots of consecutive calls gets the fast pass,
 * a slot whose content changes class pays one slower pass per band for a few calls.  ORBX_FALLBACK_HINT=0 at orbx_create switches it off. */
int orbx_extract_batch_device(orbx_extractor* h, const uint8_t* d_imgs, int nframes, int w, int hgt,
                              ptrdiff_t row_stride, ptrdiff_t frame_stride,
                              orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap,
                              int32_t* d_status, void* stream);

/* The same call cut into the three parts a host can interleave with other work on other streams (tools/corun_probe.py times
 * them alone and in pairs; the bench's lanes queue whole calls — NOTES.md 8.1):
 *   ORBX_PHASE_PYRAMID   ComputePyramid                                              (src/ORBextractor.cc:781-822)
 *   ORBX_PHASE_DETECT    FAST + NMS per cell, quotas, retainBest, GaussianBlur       (:527-707, :760)
 *   ORBX_PHASE_DESCRIBE  IC_Angle, rBRIEF, scaling, outputs                          (:124-194, :709-779)
 * `phases` is a bit mask of CONSECUTIVE parts; the parts of one batch must be queued in this order on ONE stream with identical
 * arguments, and nframes <= max_batch (the handle's scratch holds one launch group).  A call whose parts are not consecutive
 * (PYRAMID | DESCRIBE) or that queues a part before the parts in front of it were queued for the same batch returns
 * ORBX_ERR_ARG; repeating a part is allowed.  ORBX_PHASE_ALL == orbx_extract_batch_device. */
#define ORBX_PHASE_PYRAMID  1
#define ORBX_PHASE_DETECT   2
#define ORBX_PHASE_DESCRIBE 4
#define ORBX_PHASE_ALL      7
int orbx_extract_batch_device_phases(orbx_extractor* h, const uint8_t* d_imgs, int nframes, int w, int hgt,
                                     ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                     orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap,
                                     int32_t* d_status, void* stream, int phases);

/* Gather form of orbx_extract_batch_device: frames from a pointer array, in device or in host memory (a multi-camera rig with one
 * buffer per camera, frames handed over by a decoder, ROIs / views of larger images, host frames as Frame.cc has them).
 * imgs: HOST array of nframes pointers; frame f is w x hgt bytes, rows row_strides[f] bytes apart (row_strides == NULL: every row
 * stride is w).  All frames share one geometry (w, hgt).  Outputs, stream and d_status are as in orbx_extract_batch_device: frame f's
 * results are at d_kps + f*cap, d_desc + f*cap*32, d_n + f, and are bit-identical to what orbx_extract_batch_device gives for the same
 * pixels.  Frames may repeat, overlap or come in any order.  Frame f0 + f of a launch group uses fallback-hint slot f, as there.
 *   ORBX_FRAMES_ON_DEVICE  imgs[f] are DEVICE pointers, read in place by the kernels (the level-0 readers take base and row stride per
 *                          frame from a table the library uploads per launch group).  Asynchronous on `stream`; the pointer array may be
 *                          reused as soon as the call returns.  (The per-group tables rotate through four slots: with more than four
 *                          launch groups queued and not yet run — in one call or over consecutive calls — the calling thread waits for
 *                          the kernels of the group four back before it queues the next.)  Each row must be readable up to min(row_strides[f], w rounded up to 16)
 *                          bytes (the pitched-row rule of orbx_extract_batch_device, per frame).  Fastest when every pointer and row
 *                          stride is a multiple of 16.
 *   ORBX_FRAMES_ON_HOST    imgs[f] are HOST pointers, pageable or pinned.  Each launch group is uploaded into a device buffer of the
 *                          handle on an internal copy stream (pinned frames straight from the caller's memory, pageable ones through a
 *                          pinned staging buffer filled by the calling thread) while the previous group computes.  The call returns once
 *                          every frame has been read, so the caller may overwrite its buffers at once; outputs are ready when `stream`
 *                          reaches them.  Exactly w bytes of each row are read.
 * Host-checkable arguments only: a NULL array or entry, row_strides[f] < w or >= 2^24, or a bad `where` give ORBX_ERR_ARG (as does a
 * device pointer in the host form); nframes <= 0, w <= 0 or hgt <= 0 give ORBX_EMPTY; cap < orbx_max_keypoints() ORBX_ERR_CAPACITY.
 * There is no phased variant of this call. */
#define ORBX_FRAMES_ON_DEVICE 0
#define ORBX_FRAMES_ON_HOST   1
int orbx_extract_batch(orbx_extractor* h, const uint8_t* const* imgs, const ptrdiff_t* row_strides, int nframes, int w, int hgt,
                       int where, orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap,
                       int32_t* d_status, void* stream);

/* ---- colour frames (src/Tracking.cc:185-195) ---------------------------------------------------
 * Tracking::GrabImage converts every 3-channel camera frame with cvtColor(CV_RGB2GRAY) or cvtColor(CV_BGR2GRAY), picked by Camera.RGB
 * (Data/Settings.yaml: 1 = RGB, 0 = BGR), and builds the Frame on that gray image (Frame::im).  These calls do the conversion on the GPU.
 * The gray level is OpenCV 2.4's RGB2Gray<uchar> (imgproc/src/color.cpp), in integers:
 *     gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14
 * (pure red 76, green 150, blue 29, white 255).  For 4-channel pixels (CV_RGBA2GRAY / CV_BGRA2GRAY) the fourth byte is ignored.  OpenCV
 * builds that route cvtColor through IPP are not covered.  Every key point, descriptor and status of a colour call
 * equals that of the matching gray call on the converted frame; fmt == ORBX_PIX_GRAY8 gives exactly the gray call's outputs.
 * Pixel rows are read exactly: w * channels bytes of each colour row, nothing past them.
 * Host-checkable arguments: an unknown fmt, a row stride < w * channels, a gray row stride < w give ORBX_ERR_ARG; an empty geometry
 * gives ORBX_EMPTY; no usable GPU gives ORBX_ERR_DEVICE (there is no CPU fallback). */
#define ORBX_PIX_GRAY8  0   /* 1 byte per pixel */
#define ORBX_PIX_RGB8   1   /* bytes R, G, B   (Camera.RGB: 1) */
#define ORBX_PIX_BGR8   2   /* bytes B, G, R   (Camera.RGB: 0; OpenCV's own order) */
#define ORBX_PIX_RGBA8  3   /* bytes R, G, B, A (A ignored) */
#define ORBX_PIX_BGRA8  4   /* bytes B, G, R, A (A ignored) */

/* The conversion alone: nframes DEVICE frames, frame f at d_src + f*src_frame_stride, rows src_row_stride bytes apart, into the DEVICE gray
 * planes d_gray + f*gray_frame_stride, rows gray_row_stride bytes apart (exactly w bytes of each gray row are written).  Asynchronous on
 * `stream`.  Frame strides must be >= 0, and the gray frames of one call must not overlap (ORBX_ERR_ARG).  Fastest when every base and
 * stride is a multiple of 16. */
int orbx_to_gray_device(const uint8_t* d_src, int nframes, int w, int hgt, ptrdiff_t src_row_stride, ptrdiff_t src_frame_stride, int fmt,
                        uint8_t* d_gray, ptrdiff_t gray_row_stride, ptrdiff_t gray_frame_stride, void* stream);

/* orbx_extract on a colour host frame: GrabImage + Frame::Frame as one call.  The frame is staged in pinned, device-mapped memory and
 * converted by the kernel that fetches it; gray_out (optional host buffer of w*hgt bytes, NULL = not wanted) receives the gray image
 * (Frame::im).  Synchronous. */
int orbx_extract_color(orbx_extractor* h, const uint8_t* img, int w, int hgt, ptrdiff_t stride, int fmt,
                       orbx_keypoint* kps, uint8_t* desc, int cap, int* n_out, uint8_t* gray_out);

/* orbx_extract_batch_device on colour frames.  d_gray == NULL: each launch group is converted into a gray ring of the handle (one launch
 * group, 16-byte aligned, pitch w rounded up to 16; allocated on the first such call) and extracted from there.  d_gray != NULL: DEVICE gray
 * planes for all nframes frames (frame f at d_gray + f*gray_frame_stride, rows gray_row_stride bytes apart, not overlapping), written by the
 * conversion and then read by the extraction in place, so they follow the pitched-row rule of orbx_extract_batch_device.  Frame f0 + f of
 * a launch group uses fallback-hint slot f, as there.  There is no phased variant of this call. */
int orbx_extract_batch_device_color(orbx_extractor* h, const uint8_t* d_imgs, int nframes, int w, int hgt,
                                    ptrdiff_t row_stride, ptrdiff_t frame_stride, int fmt,
                                    orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, int32_t* d_status,
                                    uint8_t* d_gray, ptrdiff_t gray_row_stride, ptrdiff_t gray_frame_stride, void* stream);

/* orbx_extract_batch on colour frames: the same pointer array, `where`, outputs and ordering rules (row_strides[f] >= w * channels and
 * < 2^24).  ORBX_FRAMES_ON_DEVICE frames are read in place by the conversion kernel; ORBX_FRAMES_ON_HOST frames (pinned or pageable) are
 * uploaded per launch group into one of two colour buffers of the handle on the internal copy stream (allocated on the first such call)
 * while the previous group computes.  Each launch group is converted into the handle's gray ring and extracted from there.  There is no
 * phased variant of this call. */
int orbx_extract_batch_color(orbx_extractor* h, const uint8_t* const* imgs, const ptrdiff_t* row_strides, int nframes, int w, int hgt,
                             int where, int fmt, orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap,
                             int32_t* d_status, void* stream);

/* ---- matcher ---------------------------------------------------------------------------------- */
/* Hamming distance of two 256-bit descriptors (pure, re-entrant, host). */
int orbm_hamming256(const uint8_t* a, const uint8_t* b);

/* For each of nq query descriptors (32 B each) scan all nt train descriptors:
 *   best[q], second[q] = the two smallest distances WITH multiplicity; best_idx[q] = FIRST index
 *   attaining best (strict '<' update order of the reference loops); nt==0 -> -1, INT_MAX, INT_MAX.
 * Host-pointer form (copies in/out, synchronous) and device-pointer form (async on `stream`: its scratch — the partial
 * results of the train splits — is allocated and freed in stream order from a memory pool the library creates for itself
 * (hipMallocFromPoolAsync; the device's default pool is left as the host set it), so concurrent calls on different streams,
 * also from one host thread, never share a buffer).  nt < 2^22.
 * The kernels compute the distances on the matrix cores, exactly: +-1 encoded bits through CDNA4's block-scaled FP4 MFMA
 * (v_mfma_scale_f32_32x32x64_f8f6f4, f32 accumulate; the process default since round 5) or through the int8 MFMA
 * (ORBX_MATCH_MFMA=8 in the environment); ORBX_MATCH_MFMA=0 selects the xor + popcount kernels instead, ORBX_MATCH_MFMA=4 names
 * the default; orbm_debug_set_match_path() switches at run time (same results; tests/test_gpu_matcher.py runs every case
 * through all three).  The FP4 form keeps train indices in 15 bits per scan: batch calls with cap > 32768 take the int8 form.
 * Alignment: 4 bytes for every descriptor array of every matcher entry point — what the reference's DescriptorDistance needs, which
 * reads a descriptor as 8 x int32 (src/ORBmatcher.cc:1796-1801).  ORBX_ERR_ARG otherwise. */
int orbm_match_top2(const uint8_t* Q, int nq, const uint8_t* T, int nt,
                    int32_t* best_idx, int32_t* best, int32_t* second, int device);
int orbm_match_top2_device(const uint8_t* dQ, int nq, const uint8_t* dT, int nt,
                           int32_t* d_best_idx, int32_t* d_best, int32_t* d_second, void* stream);
/* The same scan over the train descriptors with t_valid[t] != 0 only (one byte per train descriptor; NULL = all): the
 * `if(vpMapPointMatches[realIdxF]) continue;` of the reference's scans (src/ORBmatcher.cc:205-206).  best_idx is an index into the
 * ORIGINAL train array; no valid descriptor -> -1, INT_MAX, INT_MAX.  nq, nt < 2^22. */
int orbm_match_top2_masked(const uint8_t* Q, int nq, const uint8_t* T, int nt, const uint8_t* t_valid,
                           int32_t* best_idx, int32_t* best, int32_t* second, int device);
int orbm_match_top2_masked_device(const uint8_t* dQ, int nq, const uint8_t* dT, int nt, const uint8_t* d_t_valid,
                                  int32_t* d_best_idx, int32_t* d_best, int32_t* d_second, void* stream);
/* nbatch independent problems with per-problem sizes read on the device:
 * problem i: queries dQ + i*cap*32 (d_nq[i] of them), train dT + i*cap*32 (d_nt[i]); outputs at i*cap. */
int orbm_match_top2_batch_device(const uint8_t* dQ, const int32_t* d_nq, const uint8_t* dT, const int32_t* d_nt,
                                 int nbatch, int cap, int32_t* d_best_idx, int32_t* d_best, int32_t* d_second,
                                 void* stream);
/* Candidate-set form — the shape every ORBmatcher search actually scans (GetFeaturesInArea windows,
 * src/Frame.cc:200-265; the features of one vocabulary node, src/ORBmatcher.cc:171-260): query q scans the train
 * descriptors with indices cand[seg_off[q] .. seg_off[q+1]) in LIST order; best_idx = the first listed candidate
 * attaining the best distance (a train index), -1 / INT_MAX / INT_MAX for an empty list.  seg_off has nq+1 entries,
 * non-decreasing, every segment shorter than 2^22 candidates (the key keeps the list position in 22 bits); candidate
 * indices outside [0, nt) are skipped. */
int orbm_match_top2_segments(const uint8_t* Q, int nq, const uint8_t* T, int nt, const int32_t* seg_off, const int32_t* cand,
                             int32_t* best_idx, int32_t* best, int32_t* second, int device);
int orbm_match_top2_segments_device(const uint8_t* dQ, int nq, const uint8_t* dT, int nt, const int32_t* d_seg_off,
                                    const int32_t* d_cand, int32_t* d_best_idx, int32_t* d_best, int32_t* d_second, void* stream);
/* number of queries passing  best <= th && (float)best < ratio*(float)second  (host arrays) */
int orbm_count_accepted(const int32_t* best, const int32_t* second, int nq, int th, float ratio);
/* test hook: which kernels the dense top-2 calls use from now on in this process: -1 = default (environment), 0 = xor + popcount,
 * 1 = int8 MFMA, 2 = FP4 MFMA; orbm_debug_get_match_path() = the path in effect (0 / 1 / 2) */
int orbm_debug_set_match_path(int path);
int orbm_debug_get_match_path(void);

/* Device-memory helpers for hosts that do not want to include the HIP headers (a C or C++ translation unit of ORB_SLAM can
 * keep frames, keypoints, descriptors and the search structures resident on the GPU with these four calls and chain the
 * *_device entry points of orbx.h / orbf.h / orbv.h / orbs.h; see orb_slam_amd/cpp/example_pipeline.cpp).  Synchronous. */
int orbx_device_alloc(int device, size_t bytes, void** d_ptr);       /* zero-initialised */
int orbx_device_free(int device, void* d_ptr);
int orbx_device_upload(int device, void* d_dst, const void* src, size_t bytes);
int orbx_device_download(int device, void* dst, const void* d_src, size_t bytes);      /* waits for all queued work of the device */

/* Stream / event helpers in the same spirit (opaque HIP handles): what a host needs to run several extractor handles
 * concurrently and order them against each other — the lanes of orb_slam_amd/cpp/LanePipeline.h — without HIP headers. */
int orbx_stream_create(int device, void** stream);                  /* a non-blocking stream */
int orbx_stream_create_priority(int device, int priority, void** stream);   /* hipStreamCreateWithPriority(non-blocking, priority) */
int orbx_stream_destroy(int device, void* stream);
int orbx_stream_synchronize(int device, void* stream);              /* stream == NULL: everything queued on the device */
int orbx_event_create(int device, void** event);                    /* ordering only (no timing) */
int orbx_event_destroy(int device, void* event);
int orbx_event_record(void* event, void* stream);
int orbx_stream_wait_event(void* stream, void* event);
int orbx_device_copy_async(void* d_dst, const void* d_src, size_t bytes, void* stream);    /* device to device */
/* Pinned host memory and stream-ordered copies: what a host-side caller with small per-call inputs needs to keep one search at
 * two copies + its launches + ONE synchronisation (orb_slam_amd/cpp/ORBmatcher.cc stages every search through one pinned block).
 * h_src / h_dst should come from orbx_host_alloc (pageable memory works but the copy then blocks the calling thread). */
int orbx_host_alloc(int device, size_t bytes, void** h_ptr);        /* hipHostMalloc */
int orbx_host_free(int device, void* h_ptr);
int orbx_device_upload_async(void* d_dst, const void* h_src, size_t bytes, void* stream);
int orbx_device_download_async(void* h_dst, const void* d_src, size_t bytes, void* stream);

/* MapPoint::ComputeDistinctiveDescriptors for M map points at once (src/MapPoint.cc:216-244): point p owns the descriptors
 * [seg_off[p], seg_off[p+1]) of `desc`; best_idx[p] = the index INSIDE its segment of the descriptor whose sorted row of
 * distances (self included) has the smallest element at position (int)(0.5*(N-1)) — first such row on ties —, best_median[p]
 * that value; -1 / INT_MAX for an empty segment. */
int orbm_distinctive(const uint8_t* desc, const int32_t* seg_off, int npoints, int32_t* best_idx, int32_t* best_median, int device);
int orbm_distinctive_device(const uint8_t* d_desc, const int32_t* d_seg_off, int npoints, int32_t* d_best_idx,
                            int32_t* d_best_median, void* stream);

/* ---- diagnostics (stage dumps for the parity tests; not part of the drop-in surface) ------------ */
#define ORBX_DBG_PLANE      0   /* unblurred level plane, tight w*h bytes */
#define ORBX_DBG_BLUR       1   /* blurred level plane, tight w*h bytes */
#define ORBX_DBG_NMS        2   /* per-pixel FAST score of NMS survivors (0 elsewhere), tight w*h bytes */
#define ORBX_DBG_LEVEL_KPS  3   /* selected keypoints of a level before orientation: int32 triples (x,y,response bits) */
#define ORBX_DBG_BANDS      4   /* the FAST work items (row bands of grid cells) of a level: int32[8] each = x0, x1 (the cell's columns), y0, y1
                                 * (the rows the band owns), survivors listed, of them with score >= fastTh, with score >= 7, and the threshold
                                 * the band's list was made at (fastTh, or 7 for a band that kept <= 3 survivors at fastTh) */
/* run the kernel sequence only up to `stage` (0 pyramid, 1 FAST + NMS + cell lists, 2 quotas, 3 per-cell retainBest,
 * 4 per-level cap, 5 blur, 6 describe); <0 = everything (default) */
int orbx_debug_set_stop_after(orbx_extractor* h, int stage);
/* 1: full launch groups compute the GaussianBlur per keypoint window inside the description kernel (k_describe_od: no blurred plane, no blur
 * kernel); 0: the blur kernels + k_describe.  Same outputs.  Default: ORBX_BLUR_ON_DEMAND in the environment at orbx_create, else the build's
 * choice.  ORBX_DBG_BLUR planes exist only in mode 0. */
int orbx_debug_set_blur_on_demand(orbx_extractor* h, int mode);
/* per-stage GPU time from HIP events recorded on the launch stream: enable = 0 off, 1 on, 2 on + reset totals.
 * orbx_debug_stage_time synchronises the device and returns the accumulated ms / launch-group count of a stage. */
int orbx_debug_stage_timing(orbx_extractor* h, int enable);
int orbx_debug_stage_time(orbx_extractor* h, int stage, double* total_ms, long* launches);
int orbx_debug_level_size(const orbx_extractor* h, int level, int* w, int* hgt);
/* how the last launch group built pyramid level `level` (>= 1): form 0 = k_resize (256-px tile columns), 1 = k_resize_strip (full-width row
 * strips of rows_out output rows), 2 = the fused k_pyramid cones of a small launch group; rows_out is 0 unless form is 1 */
int orbx_debug_resize_form(const orbx_extractor* h, int level, int* form, int* rows_out);
/* Which kernel variant (template instantiation) each stage of the extractor launched.  Stages: */
#define ORBX_VS_COLOR        0   /* colour -> gray conversion in front of the pipeline (k_to_gray) */
#define ORBX_VS_INGEST       1   /* the one-frame call's fetch of the staged frame (k_ingest) */
#define ORBX_VS_PYRAMID      2   /* k_pyramid cones | k_resize per level (tiled or strip) */
#define ORBX_VS_FAST         3   /* k_fast_cells | k_fast_blur */
#define ORBX_VS_QUOTA        4
#define ORBX_VS_CELL_SELECT  5   /* k_cell_select, then k_cell_select_long in full launch groups with long lists */
#define ORBX_VS_LEVEL_SELECT 6
#define ORBX_VS_BLUR         7   /* the stand-alone blur launch (none when the blur rides in k_fast_blur or runs per keypoint window) */
#define ORBX_VS_DESCRIBE     8   /* k_describe | k_describe_od */
#define ORBX_VS_COUNT        9
/* flags of a stage's launch */
#define ORBX_VF_LDS_OVER_64K  1u  /* the launch asks for more than 64 KiB of dynamic LDS (hipFuncSetAttribute first) */
#define ORBX_VF_FUSE_BLUR     2u  /* FAST: the blur's short strips ride in the same launch */
#define ORBX_VF_OVERLAP       4u  /* blur: forked onto the side stream next to the selection kernels */
#define ORBX_VF_ON_DEMAND     8u  /* describe: the blur per keypoint window inside the kernel */
#define ORBX_VF_XCD_AFFINITY 16u  /* the launch renumbers its blocks so that a frame's work items share one XCD */
/* id: the variant of the stage's first launch, in [0, orbx_debug_variant_count(stage)), or -1 when the stage launched nothing; mask: bit v set
 * for every variant v the stage launched (the pyramid launches one kernel per cone or level, the cell selection up to two) */
typedef struct orbx_stage_variant {
    int32_t id;
    uint32_t flags;
    uint64_t mask;
} orbx_stage_variant;
/* the variant `stage` of the LAST launch group took, and its name (the kernel with its template arguments, for messages; name may be NULL).
 * A host-side record made when the group was queued: no launch, no synchronisation, no device read.  The parts of a phased call
 * (orbx_extract_batch_device_phases) add to one record: after the last part it holds every stage of the batch. */
int orbx_debug_launch_variant(const orbx_extractor* h, int stage, orbx_stage_variant* out, char* name, int name_cap);
/* host-only: the number of variants of a stage (-1 for an unknown stage), and the name of one ("?" outside the range) */
int orbx_debug_variant_count(int stage);
const char* orbx_debug_variant_name(int stage, int id);
/* host-only (needs no GPU): the variants a launch group of `nframes` w x h frames would take, out[ORBX_VS_COUNT], decided by the same
 * functions the launches switch on.  The group is described the way the pipeline sees it: its level-0 rows row_stride bytes apart, frames
 * frame_stride bytes apart (contiguous form) or named by a table (gather != 0; frame_stride ignored), base_bits = the low bits of the OR of
 * every frame's base address.  color_fmt >= 0 (ORBX_PIX_*): a conversion launch stands in front (color_gather: from a table; color_bits:
 * the low bits of the OR of its source and destination bases and strides).  one_frame: the orbx_extract form, whose staged frame of
 * one_frame_bytes bytes k_ingest fetches.  side_stream: the handle has its side stream (default; ORBX_OVERLAP=0 has none). */
typedef struct orbx_plan_args {
    int32_t w, h, nframes;
    int32_t gather, xcd_affinity, on_demand, od_min_frames, stop_after;
    int64_t row_stride, frame_stride;
    uint32_t base_bits;
    int32_t color_fmt, color_gather;
    uint32_t color_bits;
    int32_t one_frame, side_stream;
    int64_t one_frame_bytes;
} orbx_plan_args;
int orbx_debug_plan(const orbx_params* p, const orbx_plan_args* a, orbx_stage_variant* out);
/* copies stage data of `frame` (index inside the last batch) / `level` into host memory; returns bytes or <0 */
long orbx_debug_fetch(orbx_extractor* h, int what, int frame, int level, void* host_out, long cap_bytes);
/* evaluate the device arithmetic on arrays (kind 0: fast_atan2(in0,in1)->out0; kind 1: sincos(in0)->out0,out1) */
/* host-only (needs no GPU): the geometry the library derives for a w x h image — per level 8 ints
 * {w, h, quota, grid_cols, grid_rows, cell_w, cell_h, n_bands}; returns the number of levels or an ORBX_ERR_* code */
int orbx_debug_geometry(const orbx_params* p, int w, int hgt, int32_t* out, int cap_levels);
/* the wave-parallel std::nth_element (greater-by-response) used by the retainBest kernels, on one list:
 * out_perm[i] = original index of the element that ends up at position i (n <= 13000) */
int orbx_debug_nth_element(const float* resp, int n, int nth, int32_t* out_perm, int device);
int orbx_debug_eval_math(int kind, const float* in0, const float* in1, float* out0, float* out1, int n, int device);
/* evaluate the device's FAST compass pre-test (k_fast_cells phase A1) on n dword quintuples at threshold t: c = four centre pixels,
 * e / w = the pixels 3 to their right / left, nn / ss = 3 rows above / below; out: the flag of pixel j in bit 8 j + 7 */
int orbx_debug_eval_compass(const uint32_t* c, const uint32_t* e, const uint32_t* w, const uint32_t* nn, const uint32_t* ss, uint32_t* out, int n, int t, int device);
/* evaluate the FAST kernels' exact score (phase B, packed halves) and opposite-pair pre-test (phase A2) on n caller-supplied rings at threshold
 * tmin: centre[i] the pixel, ring16[16 i + k] ring pixel k (k = 0 at (0, +3), then through (+3, 0), (0, -3), (-3, 0)).  score[i] = the
 * cv::FAST corner score, or 0 where it is below tmin; pair[i] = 1 where the pair test passes the pixel on */
int orbx_debug_eval_score(const uint8_t* centre, const uint8_t* ring16, uint8_t* score, uint8_t* pair, int n, int tmin, int device);
/* run k_describe_od's per-key-point blur (its row pass, float column pass and rounding epilogue, four windows per wave as in the kernel) on n
 * caller-supplied windows of 43 rows x 48 bytes: out = the n blurred regions of 37 rows x 40 bytes the descriptor taps read (window rows 3 .. 39,
 * columns 4 .. 43).  rounding: ORBX_BLUR_* for every column; general != 0: through the per-lane epilogue of edge windows instead of the fast one */
int orbx_debug_eval_blur_window(const uint8_t* windows, uint8_t* out, int n, int rounding, int general, int device);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
