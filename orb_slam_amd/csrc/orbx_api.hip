// C ABI of the extractor (include/orbx.h): handle, device memory, launch orchestration.
// All pixel work happens in the k_*.hip kernels (strung together by orbx_launch.hip); there is no host fallback.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "orbx_internal.h"
#include "orbx_launch.h"

namespace orbx {
int launch_eval_math(int kind, const float* in0, const float* in1, float* out0, float* out1, int n);
int launch_eval_compass(const uint32_t* c, const uint32_t* e, const uint32_t* w, const uint32_t* nn, const uint32_t* ss, uint32_t* out, int n, int t);
int launch_eval_score(const uint8_t* centre, const uint8_t* ring16, uint8_t* score, uint8_t* pair, int n, int tmin);
int launch_eval_blur_window(const uint8_t* win, uint8_t* out, int n, int ties_even, int general);
void stage_timer_collect(StageTimer& t);
int launch_debug_nth(const float* d_resp, int n, int nth, int* d_out);
int launch_ingest(uint8_t* d_dst, const uint8_t* mapped_src, size_t bytes, hipStream_t stream);
}
using namespace orbx;

struct orbx_extractor {
    orbx_params p;
    std::string err;
    // geometry for the current image size, and the per-batch working set (max_batch frames): replaced together by ensure_geometry
    // (hidden: the library exports the C ABI, not its internals)
    int gw = 0, gh = 0;
    HostGeom hg;
    struct __attribute__((visibility("hidden"))) Geom {
        DevBuf cells, cellrecs, bands, tabx, taby, pyr_tab;
        DevBuf pyr, blur, cand, sel, cstate, csel, cbands, level_total, level_count, status, long_cells;
    } geo;
    bool fallback_hint = true;        // ORBX_FALLBACK_HINT=0 at orbx_create
    // single-frame staging for orbx_extract
    DevBuf d_img1;
    PinnedBuf h_img1;            // pinned staging of the input frame, mapped into the device: fetched by k_ingest
    DevBuf d_out1;               // one block: [n, status, pad to 64 B][kps: cap x 28 B, padded to 64][desc: cap x 32 B]
    PinnedBuf h_out1;            // the same block in pinned host memory, mapped into the device: k_describe writes the results there
                                 //   (its device address); d_out1 + one D2H copy only with ORBX_ZERO_COPY=0
    bool zero_copy = true;       // ORBX_ZERO_COPY=0 at orbx_create: DMA copies both ways instead (A/B measurements)
    Stream s1;                   // stream of the single-frame path
    // diagnostics
    int stop_after = -1;
    bool no_xcd_affinity = false;     // ORBX_XCD_AFFINITY=0 at orbx_create (A/B measurements)
    int od_min_frames = ORBX_OD_MIN_FRAMES_DEFAULT;    // ORBX_OD_MIN_FRAMES at orbx_create (A/B measurements)
    int blur_on_demand = ORBX_BLUR_ON_DEMAND_DEFAULT;   // ORBX_BLUR_ON_DEMAND=0/1 at orbx_create, orbx_debug_set_blur_on_demand
    StageTimer timer;
    SideStream side;
    Batch last;
    bool have_last = false;
    LaunchPlan last_plan;             // what the last launch group launched (orbx_debug_launch_variant) ...
    StagePlan pend_color, pend_ingest;   // ... and what its entry point queued in front of it; cleared when the group takes them over
    // phased calls (orbx_extract_batch_device_phases): the parts already queued for the batch described by ph_key
    int ph_done = 0;
    struct PhaseKey {
        const void *img, *kps, *desc, *n, *stream;
        int nframes, w, hgt, cap;
        ptrdiff_t row_stride, frame_stride;
        bool operator==(const PhaseKey& o) const {
            return img == o.img && kps == o.kps && desc == o.desc && n == o.n && stream == o.stream && nframes == o.nframes && w == o.w && hgt == o.hgt &&
                   cap == o.cap && row_stride == o.row_stride && frame_stride == o.frame_stride;
        }
    } ph_key = {};
    // gather form (orbx_extract_batch): the per-frame level-0 table of each launch group, staged in a pinned ring and copied in stream
    // order into the matching device slot; tab_ev[i] is recorded after the kernels of the group that used slot i, so a slot is rewritten
    // only once both its copy and the kernels reading the device copy are done
    static constexpr int TAB_RING = 4;
    DevBuf d_tab;
    PinnedBuf h_tab;
    Event tab_ev[TAB_RING];
    int tab_next = 0;
    std::vector<ImgSrc> last_tab;     // the last gather group's table (orbx_debug_fetch of level 0)
    // host form: two device frame buffers of one launch group each (pitch: the row's bytes rounded up to 16), two pinned staging buffers
    // for pageable frames, and the copy stream.  up_ev[i]: the upload into buffer i is done; kern_ev[i]: the kernels that read buffer i are done.
    Stream up;
    struct __attribute__((visibility("hidden"))) HostUpload {
        DevBuf d[2];
        PinnedBuf stage[2];
        Event up_ev[2], kern_ev[2];
        int next = 0;
    };
    HostUpload hup;              // gray frames (orbx_extract_batch)
    HostUpload cup;              // colour frames (orbx_extract_batch_color): allocated on the first colour host call
    // colour forms: the gray level 0 of one launch group (pitch w rounded up to 16), converted from the caller's colour frames and read by
    // the contiguous pipeline; the one-frame call's pinned, device-mapped colour staging and gray copy (d_cimg1: ORBX_ZERO_COPY=0 only).
    // All allocated on the first colour call that needs them: gray-only callers pay for none.
    DevBuf d_cring;
    PinnedBuf h_cimg1, h_gray1;
    DevBuf d_cimg1;
};

template <typename T>
static int upload(orbx_extractor* h, DevBuf& d, const std::vector<T>& v) {
    HIPCHK(h, d.ensure(std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!v.empty()) HIPCHK(h, hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return ORBX_OK;
}

static int ensure_geometry(orbx_extractor* h, int w, int hgt) {
    if (h->gw == w && h->gh == hgt) return ORBX_OK;
    HIPCHK(h, hipDeviceSynchronize());
    h->geo = {};
    h->gw = h->gh = 0;
    h->have_last = false;
    HostGeom hg;
    int rc = build_geometry(h->p, w, hgt, hg, h->err);
    if (rc != ORBX_OK) return rc;
    h->hg = hg;
    const DevGeom& g = h->hg.g;
    const size_t B = (size_t)h->p.max_batch;
    orbx_extractor::Geom& d = h->geo;
    if ((rc = upload(h, d.cells, h->hg.cells)) != ORBX_OK) return rc;
    if ((rc = upload(h, d.cellrecs, h->hg.cellrecs)) != ORBX_OK) return rc;
    if ((rc = upload(h, d.bands, h->hg.bands)) != ORBX_OK) return rc;
    if ((rc = upload(h, d.tabx, h->hg.tabx)) != ORBX_OK) return rc;
    if ((rc = upload(h, d.taby, h->hg.taby)) != ORBX_OK) return rc;
    if ((rc = upload(h, d.pyr_tab, h->hg.pyr_tab)) != ORBX_OK) return rc;
    HIPCHK(h, d.pyr.ensure(B * g.frame_plane_bytes));
    HIPCHK(h, d.blur.ensure(B * g.frame_plane_bytes));
    HIPCHK(h, d.cand.ensure(B * std::max(g.frame_cands, 1) * sizeof(Cand)));
    HIPCHK(h, d.sel.ensure((B * std::max(g.frame_sel, 1) + 4) * sizeof(Cand)));      // (+ 4: k_describe reads a wave's four keypoints as one 32-byte scalar load)
    HIPCHK(h, d.cstate.ensure(B * g.nbands_total * sizeof(CellState)));
    HIPCHK(h, hipMemset(d.cstate, 0, B * g.nbands_total * sizeof(CellState)));      // (the fallback runs start at 0: k_fast_cells reads its slot's state before it writes it)
    HIPCHK(h, d.csel.ensure(B * g.ncells_total * sizeof(CellSel)));
    HIPCHK(h, d.cbands.ensure(B * g.ncells_total * sizeof(CellBands)));
    HIPCHK(h, hipMemset(d.cbands, 0, B * g.ncells_total * sizeof(CellBands)));
    HIPCHK(h, d.level_total.ensure(B * MAX_LEVELS * sizeof(int32_t)));
    HIPCHK(h, d.level_count.ensure(B * MAX_LEVELS * sizeof(int32_t)));
    HIPCHK(h, hipMemset(d.level_total, 0, B * MAX_LEVELS * sizeof(int32_t)));
    HIPCHK(h, hipMemset(d.level_count, 0, B * MAX_LEVELS * sizeof(int32_t)));
    HIPCHK(h, d.status.ensure(B * sizeof(int32_t)));
    HIPCHK(h, d.long_cells.ensure((B * g.ncells_total + 64) * sizeof(int32_t)));
    HIPCHK(h, hipDeviceSynchronize());
    h->gw = w;
    h->gh = hgt;
    return ORBX_OK;
}

static void fill_batch(orbx_extractor* h, Batch& b) {
    const orbx_extractor::Geom& d = h->geo;
    b.g = h->hg.g; b.cells = d.cells.as<CellGeom>(); b.cellrec = d.cellrecs.as<CellRec>(); b.bands = d.bands.as<BandGeom>(); b.tabx = d.tabx.as<ResizeX>(); b.taby = d.taby.as<ResizeY>();
    b.pyr_tab = d.pyr_tab.as<int>(); b.pyr = d.pyr.as(); b.blur = d.blur.as();
    b.cand = d.cand.as<Cand>(); b.sel = d.sel.as<Cand>(); b.cstate = d.cstate.as<CellState>(); b.csel = d.csel.as<CellSel>(); b.cbands = d.cbands.as<CellBands>();
    b.level_total = d.level_total.as<int32_t>(); b.level_count = d.level_count.as<int32_t>(); b.status = d.status.as<int32_t>();
    b.long_cells = d.long_cells.as<int32_t>();
}

// the parts of a launch group's Batch that do not depend on where its frames are
static void group_batch(orbx_extractor* h, Batch& b, int f0, int n, orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, int32_t* d_status) {
    memset(&b, 0, sizeof(b));
    fill_batch(h, b);
    b.fallback_hint = h->fallback_hint ? 1 : 0;
    b.nframes = n;
    b.xcd_affinity = (b.nframes >= XCD_AFFINITY_MIN_FRAMES && !h->no_xcd_affinity) ? 1 : 0;
    b.blur_on_demand = h->blur_on_demand;
    b.od_min_frames = h->od_min_frames;
    b.out_kps = d_kps + (size_t)f0 * cap;
    b.out_desc = d_desc + (size_t)f0 * cap * 32;
    b.out_n = d_n + f0;
    b.out_status = d_status ? d_status + f0 : nullptr;
    b.cap = cap;
}

// pinned (page-locked, registered) host memory: the copy engine reads it in place.  Pageable memory makes hipPointerGetAttributes fail
// or report hipMemoryTypeUnregistered.
static hipMemoryType host_memory_type(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return hipMemoryTypeUnregistered;
    }
    return a.type;
}

// queues one launch group; it becomes the group the diagnostics read
static int launch_group(orbx_extractor* h, const Batch& b, hipStream_t stream, int phases = ORBX_PHASE_ALL) {
    LaunchPlan plan;
    const int rc = launch_extract(b, h->hg, stream, h->stop_after, &h->timer, &h->side, phases, &plan);
    plan.st[VS_COLOR] = h->pend_color;
    plan.st[VS_INGEST] = h->pend_ingest;
    h->pend_color = h->pend_ingest = StagePlan();
    // a later part of a phased call (one launch group, the same batch: checked by the caller): the parts queued before keep their record
    if (!(phases & ORBX_PHASE_PYRAMID) && h->have_last)
        for (int s = 0; s < VS_COUNT; s++)
            if (plan.st[s].id < 0) plan.st[s] = h->last_plan.st[s];
    if (rc != ORBX_OK) { h->err = "kernel launch failed (no gfx950 code object for this device?)"; return rc; }
    h->last = b;
    h->last_plan = plan;
    h->have_last = true;
    return ORBX_OK;
}

static int ensure_cring(orbx_extractor* h, int w, int hgt, size_t& pitch);
static int convert(orbx_extractor* h, const uint8_t* src, ptrdiff_t srs, ptrdiff_t sfs, const ImgSrc* tab, unsigned long long tab_bits, int n, int w,
                   int hgt, int fmt, uint8_t* dst, ptrdiff_t drs, ptrdiff_t dfs, uint8_t* dst2, hipStream_t stream);

// device form of orbx_extract_batch[_color]: one table per launch group; the kernels read the caller's frames through it (gray), or the
// conversion kernel does and writes the handle's gray ring, which the contiguous path then reads (colour)
static int extract_gather(orbx_extractor* h, int fmt, const uint8_t* const* imgs, const ptrdiff_t* row_strides, int nframes, int w, int hgt,
                          orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, int32_t* d_status, hipStream_t stream) {
    const int mb = h->p.max_batch;
    size_t gp = 0;
    if (fmt != ORBX_PIX_GRAY8) {
        const int rc = ensure_cring(h, w, hgt, gp);
        if (rc != ORBX_OK) return rc;
    }
    const size_t tab_bytes = (size_t)orbx_extractor::TAB_RING * mb * sizeof(ImgSrc);
    HIPCHK(h, h->d_tab.ensure(tab_bytes));
    HIPCHK(h, h->h_tab.ensure(tab_bytes, hipHostMallocDefault));
    for (Event& e : h->tab_ev) HIPCHK(h, e.ensure());
    for (int f0 = 0; f0 < nframes; f0 += mb) {
        const int n = std::min(mb, nframes - f0);
        const int slot = h->tab_next;
        h->tab_next = (slot + 1) % orbx_extractor::TAB_RING;
        HIPCHK(h, hipEventSynchronize(h->tab_ev[slot]));      // the slot's last copy and the kernels that read its device copy are done
        ImgSrc* ht = h->h_tab.as<ImgSrc>() + (size_t)slot * mb;
        ImgSrc* dt = h->d_tab.as<ImgSrc>() + (size_t)slot * mb;
        unsigned long long bits = 0;
        long long min_stride = LLONG_MAX, max_stride = 0;
        for (int i = 0; i < n; i++) {
            const long long s = row_strides ? (long long)row_strides[f0 + i] : (long long)w * pix_channels(fmt);
            ht[i].data = imgs[f0 + i];
            ht[i].row_stride = s;
            bits |= (uintptr_t)imgs[f0 + i] | (unsigned long long)s;
            min_stride = std::min(min_stride, s);
            max_stride = std::max(max_stride, s);
        }
        HIPCHK(h, hipMemcpyAsync(dt, ht, (size_t)n * sizeof(ImgSrc), hipMemcpyHostToDevice, stream));
        Batch b;
        group_batch(h, b, f0, n, d_kps, d_desc, d_n, cap, d_status);
        if (fmt == ORBX_PIX_GRAY8) {
            b.img_row_stride = min_stride;
            b.img_tab = dt;
            b.img_tab_bits = bits;
            b.img_tab_min_stride = min_stride;
            b.img_tab_max_stride = max_stride;
        } else {
            const int rc = convert(h, nullptr, 0, 0, dt, bits, n, w, hgt, fmt, h->d_cring.as(), (ptrdiff_t)gp, (ptrdiff_t)(gp * hgt), nullptr, stream);
            if (rc != ORBX_OK) return rc;
            b.img = h->d_cring.as();
            b.img_row_stride = (long long)gp;
            b.img_frame_stride = (long long)(gp * hgt);
        }
        const int rc = launch_group(h, b, stream);
        if (rc != ORBX_OK) return rc;
        HIPCHK(h, hipEventRecord(h->tab_ev[slot], stream));
        if (fmt == ORBX_PIX_GRAY8) h->last_tab.assign(ht, ht + n);
    }
    return ORBX_OK;
}

// the handle's gray ring for the colour forms: one launch group of w x hgt planes, pitch w rounded up to 16 (grown with the geometry:
// nothing queued may still use the old ring)
static int ensure_cring(orbx_extractor* h, int w, int hgt, size_t& pitch) {
    pitch = ((size_t)w + 15) & ~(size_t)15;
    const size_t bytes = pitch * hgt * h->p.max_batch;
    if (h->d_cring.size() < bytes) {
        HIPCHK(h, hipDeviceSynchronize());
        HIPCHK(h, h->d_cring.ensure(bytes));
    }
    return ORBX_OK;
}

// queues the conversion of n contiguous frames into gray planes
static int convert(orbx_extractor* h, const uint8_t* src, ptrdiff_t srs, ptrdiff_t sfs, const ImgSrc* tab, unsigned long long tab_bits, int n, int w,
                   int hgt, int fmt, uint8_t* dst, ptrdiff_t drs, ptrdiff_t dfs, uint8_t* dst2, hipStream_t stream) {
    ColorArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src; a.src_row_stride = srs; a.src_frame_stride = sfs; a.tab = tab; a.tab_bits = tab_bits;
    a.dst = dst; a.dst2 = dst2; a.dst_row_stride = drs; a.dst_frame_stride = dfs; a.w = w; a.h = hgt;
    const int rc = launch_to_gray(a, n, fmt, stream, &h->pend_color);
    if (rc != ORBX_OK) h->err = rc == ORBX_ERR_ARG ? "frame too large for the conversion kernel" : "kernel launch failed (no gfx950 code object for this device?)";
    return rc;
}

// host form of orbx_extract_batch[_color]: each launch group is uploaded into one of two device buffers of U on the copy stream (pinned frames
// straight from the caller's memory, pageable ones through a pinned staging buffer filled by this thread) while the previous group computes,
// and then runs the contiguous path on that buffer (gray) or on the gray ring the conversion writes from it (colour)
static int extract_host(orbx_extractor* h, orbx_extractor::HostUpload& U, int fmt, const uint8_t* const* imgs, const ptrdiff_t* row_strides, int nframes,
                        int w, int hgt, orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, int32_t* d_status, hipStream_t stream) {
    const int mb = h->p.max_batch;
    const size_t rowb = (size_t)w * pix_channels(fmt);                 // bytes of a frame row
    const size_t P = (rowb + 15) & ~(size_t)15, fb = P * hgt;
    size_t gp = 0;
    if (fmt != ORBX_PIX_GRAY8) {
        const int rc = ensure_cring(h, w, hgt, gp);
        if (rc != ORBX_OK) return rc;
    }
    HIPCHK(h, h->up.ensure());
    for (int i = 0; i < 2; i++) {
        HIPCHK(h, U.up_ev[i].ensure());
        HIPCHK(h, U.kern_ev[i].ensure());
    }
    std::vector<char> pinned(nframes);
    bool any_pageable = false;
    for (int f = 0; f < nframes; f++) {
        const hipMemoryType t = host_memory_type(imgs[f]);
        if (t == hipMemoryTypeDevice || t == hipMemoryTypeArray) { h->err = "ORBX_FRAMES_ON_HOST with a device pointer"; return ORBX_ERR_ARG; }
        pinned[f] = t == hipMemoryTypeHost;
        any_pageable |= !pinned[f];
    }
    // grown with the geometry (nothing queued may still use the old buffers); the pinned staging buffers only once a pageable frame comes
    const size_t bytes = fb * mb;
    const bool stage = any_pageable || U.stage[0].size() > 0;
    bool grow = false;
    for (int i = 0; i < 2; i++) grow |= U.d[i].size() < bytes || (stage && U.stage[i].size() < bytes);
    if (grow) {
        HIPCHK(h, hipDeviceSynchronize());
        for (int i = 0; i < 2; i++) {
            HIPCHK(h, U.d[i].ensure(bytes));
            if (stage) HIPCHK(h, U.stage[i].ensure(bytes, hipHostMallocDefault));
        }
    }
    for (int f0 = 0; f0 < nframes; f0 += mb) {
        const int n = std::min(mb, nframes - f0);
        const int i = U.next;
        U.next ^= 1;
        uint8_t* dbuf = U.d[i].as();
        uint8_t* stage = U.stage[i].as();
        HIPCHK(h, hipStreamWaitEvent(h->up, U.kern_ev[i], 0));    // the kernels of the group that last read buffer i
        bool stage_free = false;
        for (int j = 0; j < n;) {
            const uint8_t* src = imgs[f0 + j];
            const ptrdiff_t s = row_strides ? row_strides[f0 + j] : (ptrdiff_t)rowb;
            if (pinned[f0 + j]) {
                HIPCHK(h, hipMemcpy2DAsync(dbuf + j * fb, P, src, (size_t)s, rowb, (size_t)hgt, hipMemcpyHostToDevice, h->up));
                j++;
                continue;
            }
            if (!stage_free) {                                    // its last upload (two groups back) has been read out
                HIPCHK(h, hipEventSynchronize(U.up_ev[i]));
                stage_free = true;
            }
            int j1 = j;                                           // a run of pageable frames: one copy
            for (; j1 < n && !pinned[f0 + j1]; j1++) {
                const uint8_t* fs = imgs[f0 + j1];
                const ptrdiff_t fst = row_strides ? row_strides[f0 + j1] : (ptrdiff_t)rowb;
                uint8_t* d = stage + j1 * fb;
                if (fst == (ptrdiff_t)P) memcpy(d, fs, fb - (P - rowb));           // (the last row: its bytes, not P)
                else for (int y = 0; y < hgt; y++) memcpy(d + y * P, fs + (ptrdiff_t)y * fst, rowb);
            }
            HIPCHK(h, hipMemcpyAsync(dbuf + j * fb, stage + j * fb, (size_t)(j1 - j) * fb, hipMemcpyHostToDevice, h->up));
            j = j1;
        }
        HIPCHK(h, hipEventRecord(U.up_ev[i], h->up));
        HIPCHK(h, hipStreamWaitEvent(stream, U.up_ev[i], 0));
        Batch b;
        group_batch(h, b, f0, n, d_kps, d_desc, d_n, cap, d_status);
        if (fmt == ORBX_PIX_GRAY8) {
            b.img = dbuf;
            b.img_row_stride = (long long)P;
            b.img_frame_stride = (long long)fb;
        } else {
            int rc = convert(h, dbuf, (ptrdiff_t)P, (ptrdiff_t)fb, nullptr, 0, n, w, hgt, fmt, h->d_cring.as(), (ptrdiff_t)gp, (ptrdiff_t)(gp * hgt), nullptr, stream);
            if (rc != ORBX_OK) return rc;
            HIPCHK(h, hipEventRecord(U.kern_ev[i], stream));      // buffer i is read out once converted
            b.img = h->d_cring.as();
            b.img_row_stride = (long long)gp;
            b.img_frame_stride = (long long)(gp * hgt);
        }
        const int rc = launch_group(h, b, stream);
        if (rc != ORBX_OK) return rc;
        if (fmt == ORBX_PIX_GRAY8) HIPCHK(h, hipEventRecord(U.kern_ev[i], stream));
    }
    // every caller frame has been read once both uploads are done (pinned frames are DMA'd from the caller's memory)
    for (int i = 0; i < 2; i++) HIPCHK(h, hipEventSynchronize(U.up_ev[i]));
    return ORBX_OK;
}

static int extract_one(orbx_extractor* h, int w, int hgt, int dstride, size_t bytes, orbx_keypoint* kps, uint8_t* desc, int* n_out);

extern "C" {

void orbx_default_params(orbx_params* p) {
    memset(p, 0, sizeof(*p));
    p->nfeatures = 1000;       // include/ORBextractor.h:38 defaults
    p->scale_factor = 1.2f;
    p->nlevels = 8;
    p->score_type = ORBX_FAST_SCORE;
    p->fast_th = 20;
    p->device = 0;
    p->max_batch = 1;
    p->blur_rounding = ORBX_BLUR_X86_SSE2;
    const char* fc = getenv("ORBX_FP_CONTRACT");           // setup time only (never on a launch path)
    p->fp_contract = (fc && fc[0] == '1' && fc[1] == 0) ? ORBX_FP_GCC_CONTRACT : ORBX_FP_ISO;
}

int orbx_create(const orbx_params* p, orbx_extractor** out) {
    if (!p || !out) return ORBX_ERR_ARG;
    *out = nullptr;
    if (p->max_batch < 1 || p->nlevels < 1 || p->nlevels > MAX_LEVELS || p->nfeatures < 1) return ORBX_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || p->device < 0 || p->device >= ndev) return ORBX_ERR_DEVICE;
    if (hipSetDevice(p->device) != hipSuccess) return ORBX_ERR_DEVICE;
    orbx_extractor* h = new orbx_extractor();
    h->p = *p;
    // The blur runs on a side stream next to the latency-bound selection kernels (see launch_extract);
    // ORBX_OVERLAP=0 keeps everything on one stream (cleaner per-kernel timings when profiling).
    { const char* xa = getenv("ORBX_XCD_AFFINITY"); h->no_xcd_affinity = xa && xa[0] == '0'; }
    { const char* fh = getenv("ORBX_FALLBACK_HINT"); h->fallback_hint = !(fh && fh[0] == '0'); }
    { const char* om = getenv("ORBX_OD_MIN_FRAMES"); if (om && atoi(om) >= 1) h->od_min_frames = atoi(om); }
    { const char* od = getenv("ORBX_BLUR_ON_DEMAND"); if (od && (od[0] == '0' || od[0] == '1') && od[1] == 0) h->blur_on_demand = od[0] - '0'; }
    { const char* zc = getenv("ORBX_ZERO_COPY"); h->zero_copy = !(zc && zc[0] == '0'); }
    const char* ovl = getenv("ORBX_OVERLAP");
    if (!(ovl && ovl[0] == '0') && (h->side.aux.ensure() != hipSuccess || h->side.fork.ensure() != hipSuccess || h->side.join.ensure() != hipSuccess)) {
        delete h;
        return ORBX_ERR_DEVICE;
    }
    *out = h;
    return ORBX_OK;
}

void orbx_destroy(orbx_extractor* h) {
    if (!h) return;
    (void)hipSetDevice(h->p.device);
    (void)hipDeviceSynchronize();      // the owners free nothing that queued work still reads
    delete h;
}

int orbx_get_levels(const orbx_extractor* h) { return h ? h->p.nlevels : 0; }
float orbx_get_scale_factor(const orbx_extractor* h) { return h ? (float)(double)h->p.scale_factor : 0.f; }
const char* orbx_last_error(const orbx_extractor* h) { return h ? h->err.c_str() : "null handle"; }
#ifndef ORBX_SRC_HASH
#define ORBX_SRC_HASH "unknown"
#endif
const char* orbx_build_id(void) { return ORBX_SRC_HASH; }

int orbx_max_keypoints(const orbx_extractor* h) {
    if (!h) return 0;
    HostGeom tmp;
    std::string e;
    orbx_params p = h->p;
    // quotas do not depend on the image size; use any valid size
    if (build_geometry(p, 4096, 4096, tmp, e) != ORBX_OK) return std::max(p.nfeatures, 0) + p.nlevels;
    return tmp.g.nslots;
}

int orbx_extract_batch_device(orbx_extractor* h, const uint8_t* d_imgs, int nframes, int w, int hgt, ptrdiff_t row_stride,
                              ptrdiff_t frame_stride, orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap,
                              int32_t* d_status, void* stream_) {
    return orbx_extract_batch_device_phases(h, d_imgs, nframes, w, hgt, row_stride, frame_stride, d_kps, d_desc, d_n, cap, d_status, stream_, ORBX_PHASE_ALL);
}

int orbx_extract_batch_device_phases(orbx_extractor* h, const uint8_t* d_imgs, int nframes, int w, int hgt, ptrdiff_t row_stride,
                                     ptrdiff_t frame_stride, orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap,
                                     int32_t* d_status, void* stream_, int phases) {
    if (!h) return ORBX_ERR_ARG;
    if (!d_imgs || nframes <= 0 || w <= 0 || hgt <= 0) return ORBX_EMPTY;
    if (!d_kps || !d_desc || !d_n || cap < 1 || row_stride < w) { h->err = "bad argument"; return ORBX_ERR_ARG; }
    if (phases < 1 || phases > ORBX_PHASE_ALL || phases == (ORBX_PHASE_PYRAMID | ORBX_PHASE_DESCRIBE)) {
        h->err = "bad phase mask (the parts of one call must be consecutive)";
        return ORBX_ERR_ARG;
    }
    if (phases != ORBX_PHASE_ALL && nframes > h->p.max_batch) { h->err = "a phased call covers one launch group: nframes <= max_batch"; return ORBX_ERR_ARG; }
    // a part may only follow the parts in front of it, queued for the SAME batch (same arguments, same stream): the detection reads the
    // pyramid of this batch from the handle's scratch, the description reads its selections and blurred planes.  Repeating a part is fine.
    // The bookkeeping is committed only when the call has queued its launches (a failed PYRAMID call must not let a DETECT pass the check).
    const orbx_extractor::PhaseKey key = {d_imgs, d_kps, d_desc, d_n, stream_, nframes, w, hgt, cap, row_stride, frame_stride};
    {
        const int first = phases & -phases;                       // lowest part of this call
        const int before = first - 1;                             // every part in front of it
        if (!(phases & ORBX_PHASE_PYRAMID) && (!(key == h->ph_key) || (h->ph_done & before) != before)) {
            h->err = "phase queued out of order: the parts in front of it were not queued for this batch (same arguments, same stream)";
            return ORBX_ERR_ARG;
        }
    }
    if (phases & ORBX_PHASE_PYRAMID) h->ph_done = 0;              // a new batch starts: whatever was queued before no longer counts
    HIPCHK(h, hipSetDevice(h->p.device));
    int rc = ensure_geometry(h, w, hgt);
    if (rc != ORBX_OK) return rc;
    if (cap < h->hg.g.nslots) { h->err = "cap < orbx_max_keypoints()"; return ORBX_ERR_CAPACITY; }
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nframes; f0 += h->p.max_batch) {
        Batch b;
        group_batch(h, b, f0, std::min(h->p.max_batch, nframes - f0), d_kps, d_desc, d_n, cap, d_status);
        b.img = d_imgs + (ptrdiff_t)f0 * frame_stride;
        b.img_row_stride = row_stride;
        b.img_frame_stride = frame_stride;
        if ((rc = launch_group(h, b, stream, phases)) != ORBX_OK) return rc;
    }
    if (phases & ORBX_PHASE_PYRAMID) h->ph_key = key;
    h->ph_done |= phases;
    return ORBX_OK;
}

int orbx_extract_batch(orbx_extractor* h, const uint8_t* const* imgs, const ptrdiff_t* row_strides, int nframes, int w, int hgt, int where,
                       orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, int32_t* d_status, void* stream_) {
    if (!h) return ORBX_ERR_ARG;
    if (nframes <= 0 || w <= 0 || hgt <= 0) return ORBX_EMPTY;
    if (!imgs || (where != ORBX_FRAMES_ON_DEVICE && where != ORBX_FRAMES_ON_HOST) || !d_kps || !d_desc || !d_n || cap < 1) {
        h->err = "bad argument";
        return ORBX_ERR_ARG;
    }
    for (int f = 0; f < nframes; f++) {
        const ptrdiff_t s = row_strides ? row_strides[f] : (ptrdiff_t)w;
        if (!imgs[f] || s < w || s >= ((ptrdiff_t)1 << 24)) { h->err = "bad frame pointer or row stride"; return ORBX_ERR_ARG; }
    }
    HIPCHK(h, hipSetDevice(h->p.device));
    int rc = ensure_geometry(h, w, hgt);
    if (rc != ORBX_OK) return rc;
    if (cap < h->hg.g.nslots) { h->err = "cap < orbx_max_keypoints()"; return ORBX_ERR_CAPACITY; }
    h->ph_done = 0;                                              // the handle's scratch now holds this call's groups: no phased call may continue
    hipStream_t stream = (hipStream_t)stream_;
    if (where == ORBX_FRAMES_ON_HOST) return extract_host(h, h->hup, ORBX_PIX_GRAY8, imgs, row_strides, nframes, w, hgt, d_kps, d_desc, d_n, cap, d_status, stream);
    return extract_gather(h, ORBX_PIX_GRAY8, imgs, row_strides, nframes, w, hgt, d_kps, d_desc, d_n, cap, d_status, stream);
}

int orbx_extract(orbx_extractor* h, const uint8_t* img, int w, int hgt, ptrdiff_t stride, orbx_keypoint* kps, uint8_t* desc, int cap,
                 int* n_out) {
    if (!h) return ORBX_ERR_ARG;
    if (!img || w <= 0 || hgt <= 0) return ORBX_EMPTY;   // reference: silent return, outputs untouched
    if (!kps || !desc || !n_out || stride < w) { h->err = "bad argument"; return ORBX_ERR_ARG; }
    HIPCHK(h, hipSetDevice(h->p.device));
    int rc = ensure_geometry(h, w, hgt);
    if (rc != ORBX_OK) return rc;
    const int need = h->hg.g.nslots;
    if (cap < need) { h->err = "cap < orbx_max_keypoints()"; return ORBX_ERR_CAPACITY; }
    const int dstride = (w + 63) / 64 * 64;
    const size_t bytes = (size_t)dstride * hgt;
    const size_t kps_off = 64, desc_off = kps_off + ((size_t)need * sizeof(orbx_keypoint) + 63) / 64 * 64, out_bytes = desc_off + (size_t)need * 32;
    HIPCHK(h, h->d_img1.ensure(bytes));
    HIPCHK(h, h->h_img1.ensure(bytes, hipHostMallocMapped));
    HIPCHK(h, h->d_out1.ensure(out_bytes));
    HIPCHK(h, h->h_out1.ensure(out_bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(h, h->s1.ensure());
    // In: small frames are staged in pinned memory and fetched from there by a kernel (k_ingest: no copy engine, no queue switch before
    // the first pyramid launch); large ones go through the runtime's pipelined copy.  Out: k_describe, the only writer of the results,
    // stores n / status / keypoints / descriptors straight into the pinned, device-mapped block (posted PCIe writes, visible to the
    // host once the stream has drained) - the D2H copy and the kernel -> copy dependency in front of it (~15 us) are gone.
    h->pend_color = StagePlan();
    h->pend_ingest = plan_ingest(bytes, h->zero_copy);
    if (bytes <= INGEST_MAX_BYTES) {
        for (int y = 0; y < hgt; y++) memcpy(h->h_img1.as() + (size_t)y * dstride, img + (ptrdiff_t)y * stride, (size_t)w);
        if (h->pend_ingest.id >= 0) { if ((rc = launch_ingest(h->d_img1.as(), h->h_img1.mapped(), bytes, h->s1)) != ORBX_OK) { h->err = "kernel launch failed (no gfx950 code object for this device?)"; return rc; } }
        else HIPCHK(h, hipMemcpyAsync(h->d_img1, h->h_img1, bytes, hipMemcpyHostToDevice, h->s1));
    } else {
        HIPCHK(h, hipMemcpy2DAsync(h->d_img1, dstride, img, stride, w, hgt, hipMemcpyHostToDevice, h->s1));
    }
    return extract_one(h, w, hgt, dstride, bytes, kps, desc, n_out);
}

}  // extern "C"

// the rest of the one-frame call once its gray frame is queued into d_img1 (pitch dstride) on s1: the launch group, the results
static int extract_one(orbx_extractor* h, int w, int hgt, int dstride, size_t bytes, orbx_keypoint* kps, uint8_t* desc, int* n_out) {
    const int need = h->hg.g.nslots;
    const size_t kps_off = 64, desc_off = kps_off + ((size_t)need * sizeof(orbx_keypoint) + 63) / 64 * 64, out_bytes = desc_off + (size_t)need * 32;
    int rc;
    uint8_t* out = h->zero_copy ? h->h_out1.mapped() : h->d_out1.as();
    int32_t* d_n = reinterpret_cast<int32_t*>(out);
    // (Replaying the launch group from a HIP graph was measured and does not help: 188 vs 181 us - the latency is the
    //  chain of dependent small kernels, not the launch calls.)
    rc = orbx_extract_batch_device(h, h->d_img1.as(), 1, w, hgt, dstride, (ptrdiff_t)bytes, reinterpret_cast<orbx_keypoint*>(out + kps_off),
                                   out + desc_off, d_n, need, d_n + 1, h->s1);
    if (rc != ORBX_OK) return rc;
    if (!h->zero_copy) HIPCHK(h, hipMemcpyAsync(h->h_out1, h->d_out1, out_bytes, hipMemcpyDeviceToHost, h->s1));
    HIPCHK(h, hipStreamSynchronize(h->s1));
    const int32_t* res = h->h_out1.as<int32_t>();
    if (h->stop_after >= 0) { *n_out = 0; return ORBX_OK; }
    if (res[1] != ORBX_OK) { h->err = "internal list capacity exceeded"; return res[1]; }
    const int n = res[0];
    if (n > 0) {
        memcpy(kps, h->h_out1.as() + kps_off, (size_t)n * sizeof(orbx_keypoint));
        memcpy(desc, h->h_out1.as() + desc_off, (size_t)n * 32);
    }
    *n_out = n;
    return ORBX_OK;
}

extern "C" {

// ---- colour frames (src/Tracking.cc:185-195) ------------------------------------------------------
static int color_args(int fmt, int w, ptrdiff_t row_stride) {
    const int ch = pix_channels(fmt);
    if (ch == 0) return ORBX_ERR_ARG;
    return row_stride < (ptrdiff_t)w * ch ? ORBX_ERR_ARG : ORBX_OK;
}

int orbx_to_gray_device(const uint8_t* d_src, int nframes, int w, int hgt, ptrdiff_t src_row_stride, ptrdiff_t src_frame_stride, int fmt,
                        uint8_t* d_gray, ptrdiff_t gray_row_stride, ptrdiff_t gray_frame_stride, void* stream) {
    if (pix_channels(fmt) == 0) return ORBX_ERR_ARG;
    if (nframes <= 0 || w <= 0 || hgt <= 0) return ORBX_EMPTY;
    if (!d_src || !d_gray || color_args(fmt, w, src_row_stride) != ORBX_OK || gray_row_stride < w || src_frame_stride < 0 || gray_frame_stride < 0 ||
        (nframes > 1 && gray_frame_stride < gray_row_stride * (hgt - 1) + w))
        return ORBX_ERR_ARG;
    int dev = 0, ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return ORBX_ERR_DEVICE;
    ColorArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d_src; a.src_row_stride = src_row_stride; a.src_frame_stride = src_frame_stride;
    a.dst = d_gray; a.dst_row_stride = gray_row_stride; a.dst_frame_stride = gray_frame_stride; a.w = w; a.h = hgt;
    return launch_to_gray(a, nframes, fmt, (hipStream_t)stream);
}

int orbx_extract_color(orbx_extractor* h, const uint8_t* img, int w, int hgt, ptrdiff_t stride, int fmt, orbx_keypoint* kps, uint8_t* desc, int cap,
                       int* n_out, uint8_t* gray_out) {
    if (!h) return ORBX_ERR_ARG;
    if (pix_channels(fmt) == 0) { h->err = "unknown pixel format"; return ORBX_ERR_ARG; }
    if (!img || w <= 0 || hgt <= 0) return ORBX_EMPTY;   // reference: silent return, outputs untouched
    if (!kps || !desc || !n_out || color_args(fmt, w, stride) != ORBX_OK) { h->err = "bad argument"; return ORBX_ERR_ARG; }
    if (fmt == ORBX_PIX_GRAY8) {                          // GrabImage's copyTo, then the gray call
        const int rc = orbx_extract(h, img, w, hgt, stride, kps, desc, cap, n_out);
        if (rc == ORBX_OK && gray_out)
            for (int y = 0; y < hgt; y++) memcpy(gray_out + (size_t)y * w, img + (ptrdiff_t)y * stride, (size_t)w);
        return rc;
    }
    HIPCHK(h, hipSetDevice(h->p.device));
    int rc = ensure_geometry(h, w, hgt);
    if (rc != ORBX_OK) return rc;
    const int need = h->hg.g.nslots;
    if (cap < need) { h->err = "cap < orbx_max_keypoints()"; return ORBX_ERR_CAPACITY; }
    const int dstride = (w + 63) / 64 * 64;
    const size_t bytes = (size_t)dstride * hgt;
    const size_t rowb = (size_t)w * pix_channels(fmt), cpitch = (rowb + 15) & ~(size_t)15;
    const size_t kps_off = 64, desc_off = kps_off + ((size_t)need * sizeof(orbx_keypoint) + 63) / 64 * 64, out_bytes = desc_off + (size_t)need * 32;
    HIPCHK(h, h->d_img1.ensure(bytes));
    HIPCHK(h, h->h_cimg1.ensure(cpitch * hgt, hipHostMallocMapped));
    if (gray_out) HIPCHK(h, h->h_gray1.ensure(bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(h, h->d_out1.ensure(out_bytes));
    HIPCHK(h, h->h_out1.ensure(out_bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(h, h->s1.ensure());
    // the colour frame is staged in pinned memory; the conversion kernel fetches it from there (device-mapped, k_ingest's job) and writes
    // the gray level 0 (and, if wanted, the same bytes into the pinned, device-mapped gray copy)
    for (int y = 0; y < hgt; y++) memcpy(h->h_cimg1.as() + (size_t)y * cpitch, img + (ptrdiff_t)y * stride, rowb);
    const uint8_t* src = h->h_cimg1.mapped();
    if (!h->zero_copy) {
        HIPCHK(h, h->d_cimg1.ensure(cpitch * hgt));
        HIPCHK(h, hipMemcpyAsync(h->d_cimg1, h->h_cimg1, cpitch * hgt, hipMemcpyHostToDevice, h->s1));
        src = h->d_cimg1.as();
    }
    if ((rc = convert(h, src, (ptrdiff_t)cpitch, 0, nullptr, 0, 1, w, hgt, fmt, h->d_img1.as(), dstride, 0, gray_out ? h->h_gray1.mapped() : nullptr, h->s1)) != ORBX_OK)
        return rc;
    rc = extract_one(h, w, hgt, dstride, bytes, kps, desc, n_out);
    if (rc == ORBX_OK && gray_out)
        for (int y = 0; y < hgt; y++) memcpy(gray_out + (size_t)y * w, h->h_gray1.as() + (size_t)y * dstride, (size_t)w);
    return rc;
}

int orbx_extract_batch_device_color(orbx_extractor* h, const uint8_t* d_imgs, int nframes, int w, int hgt, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                    int fmt, orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, int32_t* d_status, uint8_t* d_gray,
                                    ptrdiff_t gray_row_stride, ptrdiff_t gray_frame_stride, void* stream_) {
    if (!h) return ORBX_ERR_ARG;
    if (pix_channels(fmt) == 0) { h->err = "unknown pixel format"; return ORBX_ERR_ARG; }
    if (!d_imgs || nframes <= 0 || w <= 0 || hgt <= 0) return ORBX_EMPTY;
    if (!d_kps || !d_desc || !d_n || cap < 1 || color_args(fmt, w, row_stride) != ORBX_OK || frame_stride < 0 ||
        (d_gray && (gray_row_stride < w || gray_frame_stride < 0 || (nframes > 1 && gray_frame_stride < gray_row_stride * (hgt - 1) + w)))) {
        h->err = "bad argument";
        return ORBX_ERR_ARG;
    }
    if (fmt == ORBX_PIX_GRAY8 && !d_gray) return orbx_extract_batch_device(h, d_imgs, nframes, w, hgt, row_stride, frame_stride, d_kps, d_desc, d_n, cap, d_status, stream_);
    HIPCHK(h, hipSetDevice(h->p.device));
    int rc = ensure_geometry(h, w, hgt);
    if (rc != ORBX_OK) return rc;
    if (cap < h->hg.g.nslots) { h->err = "cap < orbx_max_keypoints()"; return ORBX_ERR_CAPACITY; }
    size_t gp = 0;
    if (!d_gray && (rc = ensure_cring(h, w, hgt, gp)) != ORBX_OK) return rc;
    h->ph_done = 0;                                              // the handle's scratch now holds this call's groups: no phased call may continue
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nframes; f0 += h->p.max_batch) {
        const int n = std::min(h->p.max_batch, nframes - f0);
        uint8_t* g = d_gray ? d_gray + (ptrdiff_t)f0 * gray_frame_stride : h->d_cring.as();
        const ptrdiff_t grs = d_gray ? gray_row_stride : (ptrdiff_t)gp, gfs = d_gray ? gray_frame_stride : (ptrdiff_t)(gp * hgt);
        if ((rc = convert(h, d_imgs + (ptrdiff_t)f0 * frame_stride, row_stride, frame_stride, nullptr, 0, n, w, hgt, fmt, g, grs, gfs, nullptr, stream)) != ORBX_OK)
            return rc;
        Batch b;
        group_batch(h, b, f0, n, d_kps, d_desc, d_n, cap, d_status);
        b.img = g;
        b.img_row_stride = grs;
        b.img_frame_stride = gfs;
        if ((rc = launch_group(h, b, stream)) != ORBX_OK) return rc;
    }
    return ORBX_OK;
}

int orbx_extract_batch_color(orbx_extractor* h, const uint8_t* const* imgs, const ptrdiff_t* row_strides, int nframes, int w, int hgt, int where, int fmt,
                             orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_n, int cap, int32_t* d_status, void* stream_) {
    if (!h) return ORBX_ERR_ARG;
    const int ch = pix_channels(fmt);
    if (ch == 0) { h->err = "unknown pixel format"; return ORBX_ERR_ARG; }
    if (nframes <= 0 || w <= 0 || hgt <= 0) return ORBX_EMPTY;
    if (!imgs || (where != ORBX_FRAMES_ON_DEVICE && where != ORBX_FRAMES_ON_HOST) || !d_kps || !d_desc || !d_n || cap < 1) {
        h->err = "bad argument";
        return ORBX_ERR_ARG;
    }
    if (fmt == ORBX_PIX_GRAY8) return orbx_extract_batch(h, imgs, row_strides, nframes, w, hgt, where, d_kps, d_desc, d_n, cap, d_status, stream_);
    for (int f = 0; f < nframes; f++) {
        const ptrdiff_t s = row_strides ? row_strides[f] : (ptrdiff_t)w * ch;
        if (!imgs[f] || s < (ptrdiff_t)w * ch || s >= ((ptrdiff_t)1 << 24)) { h->err = "bad frame pointer or row stride"; return ORBX_ERR_ARG; }
    }
    HIPCHK(h, hipSetDevice(h->p.device));
    int rc = ensure_geometry(h, w, hgt);
    if (rc != ORBX_OK) return rc;
    if (cap < h->hg.g.nslots) { h->err = "cap < orbx_max_keypoints()"; return ORBX_ERR_CAPACITY; }
    h->ph_done = 0;
    hipStream_t stream = (hipStream_t)stream_;
    if (where == ORBX_FRAMES_ON_HOST) return extract_host(h, h->cup, fmt, imgs, row_strides, nframes, w, hgt, d_kps, d_desc, d_n, cap, d_status, stream);
    return extract_gather(h, fmt, imgs, row_strides, nframes, w, hgt, d_kps, d_desc, d_n, cap, d_status, stream);
}

// ---- diagnostics ---------------------------------------------------------------------------------
int orbx_debug_set_blur_on_demand(orbx_extractor* h, int mode) {
    if (!h || mode < 0 || mode > 1) return ORBX_ERR_ARG;
    h->blur_on_demand = mode;
    return ORBX_OK;
}

int orbx_debug_set_stop_after(orbx_extractor* h, int stage) {
    if (!h) return ORBX_ERR_ARG;
    h->stop_after = stage;
    return ORBX_OK;
}

int orbx_debug_stage_timing(orbx_extractor* h, int enable) {
    if (!h) return ORBX_ERR_ARG;
    if (hipSetDevice(h->p.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ORBX_ERR_DEVICE;
    stage_timer_collect(h->timer);
    h->timer.enabled = enable != 0;
    if (enable == 2) { memset(h->timer.ms, 0, sizeof(h->timer.ms)); memset(h->timer.launches, 0, sizeof(h->timer.launches)); }
    return ORBX_OK;
}

int orbx_debug_stage_time(orbx_extractor* h, int stage, double* total_ms, long* launches) {
    if (!h || stage < 0 || stage >= ST_COUNT) return ORBX_ERR_ARG;
    if (hipSetDevice(h->p.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ORBX_ERR_DEVICE;
    stage_timer_collect(h->timer);
    *total_ms = h->timer.ms[stage];
    *launches = h->timer.launches[stage];
    return ORBX_OK;
}

int orbx_debug_level_size(const orbx_extractor* h, int level, int* w, int* hgt) {
    if (!h || h->gw == 0 || level < 0 || level >= h->hg.g.nlevels) return ORBX_ERR_ARG;
    *w = h->hg.g.lv[level].w;
    *hgt = h->hg.g.lv[level].h;
    return ORBX_OK;
}

int orbx_debug_resize_form(const orbx_extractor* h, int level, int* form, int* rows_out) {
    if (!h || !h->have_last || !form || !rows_out || level < 1 || level >= h->hg.g.nlevels) return ORBX_ERR_ARG;
    StripChoice sc;
    *form = resize_form(h->last, h->hg, level, sc);
    *rows_out = sc.rows_out;
    return ORBX_OK;
}

int orbx_debug_launch_variant(const orbx_extractor* h, int stage, orbx_stage_variant* out, char* name, int name_cap) {
    if (!h || !h->have_last || !out || stage < 0 || stage >= VS_COUNT) return ORBX_ERR_ARG;
    const StagePlan& s = h->last_plan.st[stage];
    out->id = s.id; out->flags = s.flags; out->mask = s.mask;
    if (name && name_cap > 0) snprintf(name, (size_t)name_cap, "%s", s.id < 0 ? "" : variant_name(stage, s.id));
    return ORBX_OK;
}

int orbx_debug_variant_count(int stage) { return variant_count(stage); }
const char* orbx_debug_variant_name(int stage, int id) { return variant_name(stage, id); }

int orbx_debug_plan(const orbx_params* p, const orbx_plan_args* a, orbx_stage_variant* out) {
    if (!p || !a || !out || a->nframes < 1 || a->row_stride < a->w) return ORBX_ERR_ARG;
    HostGeom hg;
    std::string err;
    const int rc = build_geometry(*p, a->w, a->h, hg, err);
    if (rc != ORBX_OK) return rc;
    // the group as launch_group sees it: only the fields the decisions read (no pointer is followed)
    Batch b;
    memset(&b, 0, sizeof(b));
    b.g = hg.g;
    b.nframes = a->nframes;
    b.xcd_affinity = a->xcd_affinity ? 1 : 0;
    b.blur_on_demand = a->on_demand ? 1 : 0;
    b.od_min_frames = a->od_min_frames;
    b.img_row_stride = a->row_stride;
    ImgSrc none = {nullptr, 0};
    if (a->gather) {
        b.img_tab = &none;
        b.img_tab_bits = (unsigned long long)a->base_bits | (unsigned long long)a->row_stride;
        b.img_tab_min_stride = b.img_tab_max_stride = a->row_stride;
    } else {
        b.img = reinterpret_cast<const uint8_t*>((uintptr_t)a->base_bits);
        b.img_frame_stride = a->frame_stride;
    }
    LaunchPlan plan = plan_extract(b, hg, a->stop_after, a->side_stream != 0, ORBX_PHASE_ALL);
    if (a->color_fmt >= 0) {
        ColorArgs c;
        memset(&c, 0, sizeof(c));
        ImgSrc cnone = {nullptr, 0};
        if (a->color_gather) { c.tab = &cnone; c.tab_bits = a->color_bits; }
        else c.src = reinterpret_cast<const uint8_t*>((uintptr_t)a->color_bits);
        plan.st[VS_COLOR] = plan_to_gray(c, a->color_fmt);
    }
    if (a->one_frame) plan.st[VS_INGEST] = plan_ingest((size_t)a->one_frame_bytes, true);
    for (int s = 0; s < VS_COUNT; s++) { out[s].id = plan.st[s].id; out[s].flags = plan.st[s].flags; out[s].mask = plan.st[s].mask; }
    return ORBX_OK;
}

long orbx_debug_fetch(orbx_extractor* h, int what, int frame, int level, void* host_out, long cap_bytes) {
    if (!h || !h->have_last || frame < 0 || frame >= h->last.nframes || level < 0 || level >= h->hg.g.nlevels) return ORBX_ERR_ARG;
    if (hipSetDevice(h->p.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ORBX_ERR_DEVICE;
    const DevGeom& g = h->hg.g;
    const LevelGeom& L = g.lv[level];
    const Batch& b = h->last;
    if (what == ORBX_DBG_NMS) {
        // rebuilt on the host from the per-cell survivor lists (valid while they are untouched, i.e. when the
        // last run stopped after stage 1: the retainBest kernels filter and permute the lists in place)
        const long need = (long)L.w * L.h;
        if (cap_bytes < need) return ORBX_ERR_CAPACITY;
        memset(host_out, 0, need);
        std::vector<CellState> st(g.nbands_total);
        if (hipMemcpy(st.data(), b.cstate + (size_t)frame * g.nbands_total, g.nbands_total * sizeof(CellState), hipMemcpyDeviceToHost) != hipSuccess)
            return ORBX_ERR_DEVICE;
        std::vector<Cand> tmp;
        for (int it = 0; it < g.nbands_total; it++) {
            const BandGeom& bgm = h->hg.bands[it];
            if (bgm.level != level) continue;
            const int n = st[it].n_all;
            if (n <= 0) continue;
            if (n > bgm.cand_cap) return ORBX_ERR_CAPACITY;
            tmp.resize(n);
            if (hipMemcpy(tmp.data(), b.cand + (size_t)frame * g.frame_cands + L.cand_base + bgm.cand_off, (size_t)n * sizeof(Cand), hipMemcpyDeviceToHost) != hipSuccess)
                return ORBX_ERR_DEVICE;
            for (int i = 0; i < n; i++) ((uint8_t*)host_out)[(size_t)(tmp[i].pos >> 16) * L.w + (tmp[i].pos & 0xFFFF)] = (uint8_t)tmp[i].resp;
        }
        return need;
    }
    if (what == ORBX_DBG_BANDS) {
        std::vector<CellState> st(g.nbands_total);
        if (hipMemcpy(st.data(), b.cstate + (size_t)frame * g.nbands_total, g.nbands_total * sizeof(CellState), hipMemcpyDeviceToHost) != hipSuccess)
            return ORBX_ERR_DEVICE;
        long n = 0;
        for (int it = 0; it < g.nbands_total; it++) {
            const BandGeom& bgm = h->hg.bands[it];
            if (bgm.level != level) continue;
            if ((n + 1) * 32 > cap_bytes) return ORBX_ERR_CAPACITY;
            int32_t* o = (int32_t*)host_out + 8 * n++;
            o[0] = bgm.x0; o[1] = bgm.x1; o[2] = bgm.y0; o[3] = bgm.y1;
            o[4] = st[it].n_all; o[5] = st[it].n_hi; o[6] = st[it].n_lo;
            o[7] = st[it].thr & 0xFF;          // the threshold the band's list was made at (fastTh; 7 after the second pass or on the fallback hint)
        }
        return n * 32;
    }
    if (what == ORBX_DBG_PLANE || what == ORBX_DBG_BLUR) {
        const long need = (long)L.w * L.h;
        if (cap_bytes < need) return ORBX_ERR_CAPACITY;
        const uint8_t* src;
        size_t spitch;
        if (what == ORBX_DBG_PLANE && level == 0) {
            if (b.img_tab) {
                src = h->last_tab[frame].data;
                spitch = (size_t)h->last_tab[frame].row_stride;
            } else {
                src = b.img + (ptrdiff_t)frame * b.img_frame_stride;
                spitch = (size_t)b.img_row_stride;
            }
        } else {
            const uint8_t* base = what == ORBX_DBG_PLANE ? b.pyr : b.blur;
            src = base + (size_t)frame * g.frame_plane_bytes + L.plane_off;
            spitch = (size_t)L.stride;
        }
        if (hipMemcpy2D(host_out, L.w, src, spitch, L.w, L.h, hipMemcpyDeviceToHost) != hipSuccess) return ORBX_ERR_DEVICE;
        return need;
    }
    if (what == ORBX_DBG_LEVEL_KPS) {
        int32_t n = 0;
        if (hipMemcpy(&n, b.level_count + frame * MAX_LEVELS + level, 4, hipMemcpyDeviceToHost) != hipSuccess) return ORBX_ERR_DEVICE;
        const long need = (long)n * 12;
        if (cap_bytes < need) return ORBX_ERR_CAPACITY;
        std::vector<Cand> tmp(std::max(n, 1));
        if (n > 0 && hipMemcpy(tmp.data(), b.sel + (size_t)frame * g.frame_sel + L.sel_base, (size_t)n * sizeof(Cand), hipMemcpyDeviceToHost) != hipSuccess)
            return ORBX_ERR_DEVICE;
        int32_t* o = (int32_t*)host_out;
        for (int i = 0; i < n; i++) {
            o[3 * i] = tmp[i].pos & 0xFFFF;
            o[3 * i + 1] = tmp[i].pos >> 16;
            memcpy(&o[3 * i + 2], &tmp[i].resp, 4);
        }
        return need;
    }
    return ORBX_ERR_ARG;
}

int orbx_debug_geometry(const orbx_params* p, int w, int hgt, int32_t* out, int cap_levels) {
    if (!p || !out) return ORBX_ERR_ARG;
    HostGeom hg;
    std::string err;
    const int rc = build_geometry(*p, w, hgt, hg, err);
    if (rc != ORBX_OK) {
        if (getenv("ORBX_DBG_GEOM")) fprintf(stderr, "orbx geometry: %s\n", err.c_str());
        return rc;
    }
    if (cap_levels < hg.g.nlevels) return ORBX_ERR_CAPACITY;
    if (getenv("ORBX_DBG_GEOM"))
        fprintf(stderr, "orbx geometry: fast_lds_bytes %d (band image %d B, chunks %d), sel_lds %d, bands %d, cells %d\n", hg.g.fast_lds_bytes, hg.g.fast_max_img,
                hg.g.fast_max_chunks, hg.g.sel_lds_cell, (int)hg.bands.size(), (int)hg.cells.size());
    for (int l = 0; l < hg.g.nlevels; l++) {
        const LevelGeom& L = hg.g.lv[l];
        int nb = 0;
        for (const BandGeom& b : hg.bands) nb += b.level == l;
        int32_t* o = out + 8 * l;
        o[0] = L.w; o[1] = L.h; o[2] = L.ndesired; o[3] = L.gcols; o[4] = L.grows; o[5] = L.cellW; o[6] = L.cellH; o[7] = nb;
    }
    return hg.g.nlevels;
}

int orbx_debug_nth_element(const float* resp, int n, int nth, int32_t* out_perm, int device) {
    if (!resp || !out_perm || n < 1 || nth < 0 || nth > n || n > 13000) return ORBX_ERR_ARG;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto r = s.in(resp, n);
    const auto o = s.out<int>(n);
    HIPTRY(s.alloc());
    const int rc = launch_debug_nth(s[r], n, nth, s[o]);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(out_perm, o, n));
    return ORBX_OK;
}

int orbx_debug_eval_math(int kind, const float* in0, const float* in1, float* out0, float* out1, int n, int device) {
    if (n <= 0) return ORBX_OK;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto i0 = s.in(in0, n), i1 = s.in(in1 ? in1 : in0, n);
    const auto o0 = s.out<float>(n), o1 = s.out<float>(n);
    HIPTRY(s.alloc());
    const int rc = launch_eval_math(kind, s[i0], s[i1], s[o0], s[o1], n);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(out0, o0, n));
    if (out1) HIPTRY(s.get(out1, o1, n));
    return ORBX_OK;
}

int orbx_debug_eval_compass(const uint32_t* c, const uint32_t* e, const uint32_t* w, const uint32_t* nn, const uint32_t* ss, uint32_t* out, int n, int t, int device) {
    if (n <= 0) return ORBX_OK;
    if (!c || !e || !w || !nn || !ss || !out || t < 0) return ORBX_ERR_ARG;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto ic = s.in(c, n), ie = s.in(e, n), iw = s.in(w, n), in_ = s.in(nn, n), is = s.in(ss, n);
    const auto o = s.out<uint32_t>(n);
    HIPTRY(s.alloc());
    const int rc = launch_eval_compass(s[ic], s[ie], s[iw], s[in_], s[is], s[o], n, t);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(out, o, n));
    return ORBX_OK;
}

int orbx_debug_eval_score(const uint8_t* centre, const uint8_t* ring16, uint8_t* score, uint8_t* pair, int n, int tmin, int device) {
    if (n <= 0) return ORBX_OK;
    if (!centre || !ring16 || !score || !pair || tmin < 0 || n > (1 << 26)) return ORBX_ERR_ARG;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto ic = s.in(centre, n), ir = s.in(ring16, (size_t)n * 16);
    const auto os = s.out<uint8_t>(n), op = s.out<uint8_t>(n);
    HIPTRY(s.alloc());
    const int rc = launch_eval_score(s[ic], s[ir], s[os], s[op], n, tmin);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(score, os, n));
    HIPTRY(s.get(pair, op, n));
    return ORBX_OK;
}

int orbx_debug_eval_blur_window(const uint8_t* windows, uint8_t* out, int n, int rounding, int general, int device) {
    if (n <= 0) return ORBX_OK;
    if (!windows || !out || (rounding != ORBX_BLUR_X86_SSE2 && rounding != ORBX_BLUR_HALF_UP)) return ORBX_ERR_ARG;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto iw = s.in(windows, (size_t)n * 43 * 48);
    const auto o = s.out<uint8_t>((size_t)n * 37 * 40);
    HIPTRY(s.alloc());
    const int rc = launch_eval_blur_window(s[iw], s[o], n, rounding == ORBX_BLUR_X86_SSE2, general);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(out, o, (size_t)n * 37 * 40));
    return ORBX_OK;
}

int orbx_device_alloc(int device, size_t bytes, void** d_ptr) {
    if (!d_ptr || bytes == 0) return ORBX_ERR_ARG;
    HIPTRY(hipSetDevice(device));
    DevBuf p;
    HIPTRY(p.ensure(bytes));
    HIPTRY(hipMemset(p, 0, bytes));
    *d_ptr = p.release();
    return ORBX_OK;
}

int orbx_device_free(int device, void* d_ptr) {
    if (!d_ptr) return ORBX_OK;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_DEVICE;
    return hipFree(d_ptr) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_device_upload(int device, void* d_dst, const void* src, size_t bytes) {
    if (bytes == 0) return ORBX_OK;
    if (!d_dst || !src) return ORBX_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_DEVICE;
    return hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_device_download(int device, void* dst, const void* d_src, size_t bytes) {
    if (bytes == 0) return ORBX_OK;
    if (!dst || !d_src) return ORBX_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ORBX_ERR_DEVICE;
    return hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_stream_create(int device, void** stream) {
    if (!stream) return ORBX_ERR_ARG;
    hipStream_t s = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return ORBX_ERR_DEVICE;
    *stream = s;
    return ORBX_OK;
}

int orbx_stream_create_priority(int device, int priority, void** stream) {
    if (!stream) return ORBX_ERR_ARG;
    hipStream_t s = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority) != hipSuccess) return ORBX_ERR_DEVICE;
    *stream = s;
    return ORBX_OK;
}

int orbx_stream_destroy(int device, void* stream) {
    if (!stream) return ORBX_OK;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_DEVICE;
    return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_stream_synchronize(int device, void* stream) {
    if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_DEVICE;
    const hipError_t e = stream ? hipStreamSynchronize((hipStream_t)stream) : hipDeviceSynchronize();
    return e == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_event_create(int device, void** event) {
    if (!event) return ORBX_ERR_ARG;
    hipEvent_t e = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return ORBX_ERR_DEVICE;
    *event = e;
    return ORBX_OK;
}

int orbx_event_destroy(int device, void* event) {
    if (!event) return ORBX_OK;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_DEVICE;
    return hipEventDestroy((hipEvent_t)event) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_event_record(void* event, void* stream) {
    if (!event) return ORBX_ERR_ARG;
    return hipEventRecord((hipEvent_t)event, (hipStream_t)stream) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_stream_wait_event(void* stream, void* event) {
    if (!event) return ORBX_ERR_ARG;
    return hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_device_copy_async(void* d_dst, const void* d_src, size_t bytes, void* stream) {
    if (bytes == 0) return ORBX_OK;
    if (!d_dst || !d_src) return ORBX_ERR_ARG;
    return hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_host_alloc(int device, size_t bytes, void** h_ptr) {
    if (!h_ptr || bytes == 0) return ORBX_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_DEVICE;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return ORBX_ERR_DEVICE;
    *h_ptr = p;
    return ORBX_OK;
}

int orbx_host_free(int device, void* h_ptr) {
    if (!h_ptr) return ORBX_OK;
    if (hipSetDevice(device) != hipSuccess) return ORBX_ERR_DEVICE;
    return hipHostFree(h_ptr) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_device_upload_async(void* d_dst, const void* h_src, size_t bytes, void* stream) {
    if (bytes == 0) return ORBX_OK;
    if (!d_dst || !h_src) return ORBX_ERR_ARG;
    return hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbx_device_download_async(void* h_dst, const void* d_src, size_t bytes, void* stream) {
    if (bytes == 0) return ORBX_OK;
    if (!h_dst || !d_src) return ORBX_ERR_ARG;
    return hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

}  // extern "C"
