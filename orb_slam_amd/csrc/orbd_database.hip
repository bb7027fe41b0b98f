// Key-frame database on gfx950: the inverted-file walk, the common-word threshold and the scores of reference
// src/KeyFrameDatabase.cc (DetectLoopCandidates :75-134, DetectRelocalisationCandidates :191-250) for many queries per
// launch.  include/orbd.h is the boundary; the host C++ that walks KeyFrame objects is orb_slam_amd/cpp/KeyFrameDatabase.cc.
//
// Data layout in HBM.
//   arena      every stored BowVector, one contiguous segment per add (ent_id / ent_val ascending by word, ent_slot = the
//              slot that owns the entry or -1 for reserved room), appended in add order.  A segment is live while
//              slot_off[slot] points at it; erase sets slot_n[slot] = -1, so erased and replaced segments go dead in place.
//              When an add does not fit, the live segments are copied, in order, into a new arena twice the live size.
//   slot_*     per slot: segment offset, word count (-1 = absent), add sequence (the order of the reference's push_back).
//   inverted   word -> slots, CSR, rebuilt lazily on the query's stream after adds and erases: histogram of the live
//              entries, one exclusive scan over the words, scatter.  The order inside one word's list is free: a query
//              keeps each slot's first-touch rank and orders its result by (rank, add sequence), the reference's
//              lKFsSharingWords order.
//
// Kernels:
//   k_add      one workgroup per added frame: checks the words (range, strictly ascending), copies the segment, sets the slot.
//   k_hist / k_scan / k_scatter   the inverted-file rebuild.
//   k_query<LDS>  one workgroup per query (a grid-stride loop over the queries): every wave takes a query word and its
//              lanes walk that word's list, counting hits per slot and keeping the smallest query-word rank with atomics
//              (integer: exact whatever the order); then the exclusions, the max count and threshold, the touched slots
//              compacted and bitonic-sorted by (rank, add sequence), and the score of each slot above the threshold by one
//              lane in ascending word order (orbv_score.h, the code orbv_score runs on the host).  Counts and ranks sit in
//              LDS up to LDS_SLOTS slots, in a per-workgroup global row above that.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <mutex>
#include <vector>

#include "orbd.h"
#include "orbv.h"
#include "orbv_score.h"
#include "orbx.h"
#include "orbx_host.h"

namespace orbd {

constexpr int TPB = 256;              // one workgroup: four waves
constexpr int LDS_SLOTS = 16384;      // count + rank of 16384 slots = 128 KiB of LDS
constexpr int RANK_NONE = INT_MAX;

__global__ __launch_bounds__(TPB) void k_add(int nframes, const int32_t* tab_slot, long long base, int cap, uint32_t seq0,
                                             const uint32_t* bow_id, const double* bow_val, const int32_t* n_bow, int n_words,
                                             uint32_t* ent_id, double* ent_val, int32_t* ent_slot, int32_t* slot_off, int32_t* slot_n,
                                             uint32_t* slot_seq, int32_t* status) {
    const int f = blockIdx.x;
    if (f >= nframes) return;
    __shared__ int bad;
    const int n = n_bow[f];
    if (threadIdx.x == 0) bad = (n < 0 || n > cap);
    __syncthreads();
    const uint32_t* id = bow_id + (size_t)f * cap;
    if (!bad)
        for (int i = threadIdx.x; i < n; i += TPB)
            if (id[i] >= (uint32_t)n_words || (i > 0 && id[i - 1] >= id[i])) atomicOr(&bad, 1);
    __syncthreads();
    const int m = bad ? 0 : n;
    const long long off = base + (long long)f * cap;
    const int slot = tab_slot[f];
    for (int e = threadIdx.x; e < cap; e += TPB) {
        if (e < m) {
            ent_id[off + e] = id[e];
            ent_val[off + e] = bow_val[(size_t)f * cap + e];
            ent_slot[off + e] = slot;
        } else {
            ent_slot[off + e] = -1;
        }
    }
    if (threadIdx.x == 0) {
        slot_off[slot] = (int32_t)off;
        slot_n[slot] = m;
        slot_seq[slot] = seq0 + (uint32_t)f;
        if (status) status[f] = bad ? ORBX_ERR_ARG : ORBX_OK;
    }
}

// the live segments, in order, into a fresh arena (the table: slot, new offset, reserved length per live segment)
__global__ __launch_bounds__(TPB) void k_compact(int nseg, const int32_t* tab, const uint32_t* id0, const double* val0, const int32_t* slot0,
                                                 uint32_t* id1, double* val1, int32_t* slot1, int32_t* slot_off) {
    const int k = blockIdx.x;
    if (k >= nseg) return;
    const int slot = tab[3 * k], dst = tab[3 * k + 1], len = tab[3 * k + 2];
    const int src = slot_off[slot];
    __syncthreads();
    for (int e = threadIdx.x; e < len; e += TPB) {
        id1[dst + e] = id0[src + e];
        val1[dst + e] = val0[src + e];
        slot1[dst + e] = slot0[src + e];
    }
    if (threadIdx.x == 0) slot_off[slot] = dst;
}

__device__ inline bool live(int e, const int32_t* ent_slot, const int32_t* slot_off, const int32_t* slot_n, int* s) {
    *s = ent_slot[e];
    if (*s < 0) return false;
    const int o = slot_off[*s];
    return e >= o && e < o + slot_n[*s];
}

__global__ __launch_bounds__(TPB) void k_hist(int n_ent, const uint32_t* ent_id, const int32_t* ent_slot, const int32_t* slot_off,
                                              const int32_t* slot_n, int32_t* word_cnt) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    int s;
    if (e < n_ent && live(e, ent_slot, slot_off, slot_n, &s)) atomicAdd(&word_cnt[ent_id[e]], 1);
}

// exclusive scan of n counts (in place into off) and a copy into cursor: one workgroup, one contiguous chunk per thread
constexpr int SCAN_TPB = 1024;
__global__ __launch_bounds__(SCAN_TPB) void k_scan(int n, int32_t* off, int32_t* cursor) {
    __shared__ int32_t part[SCAN_TPB];
    const int chunk = (n + SCAN_TPB - 1) / SCAN_TPB;
    const int lo = min(n, (int)threadIdx.x * chunk), hi = min(n, lo + chunk);
    int32_t sum = 0;
    for (int i = lo; i < hi; i++) sum += off[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < SCAN_TPB; d <<= 1) {
        const int32_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int32_t run = part[threadIdx.x] - sum;
    for (int i = lo; i < hi; i++) {
        const int32_t c = off[i];
        off[i] = run;
        if (i < n - 1) cursor[i] = run;
        run += c;
    }
}

__global__ __launch_bounds__(TPB) void k_scatter(int n_ent, const uint32_t* ent_id, const int32_t* ent_slot, const int32_t* slot_off,
                                                 const int32_t* slot_n, int32_t* cursor, int32_t* list) {
    const int e = blockIdx.x * TPB + threadIdx.x;
    int s;
    if (e < n_ent && live(e, ent_slot, slot_off, slot_n, &s)) list[atomicAdd(&cursor[ent_id[e]], 1)] = s;
}

struct QueryArgs {
    int nq, qcap, n_words, capacity, slot_hi, sort_cap, scoring, out_cap;
    const uint32_t* q_id;
    const double* q_val;
    const int32_t* q_n;
    const int32_t* excl_off;
    const int32_t* excl_slot;
    int32_t* excl_words;
    int32_t* share_slot;
    int32_t* share_words;
    double* share_score;
    int32_t* n_share;
    int32_t* min_common;
    int32_t* status;
    // the database
    const int32_t* word_off;
    const int32_t* list;
    const uint32_t* ent_id;
    const double* ent_val;
    const int32_t* slot_off;
    const int32_t* slot_n;
    const uint32_t* slot_seq;
    // per-workgroup scratch rows: sort_cap keys + sort_cap slots; count + rank (capacity each) when not in LDS
    unsigned long long* keys;
    int32_t* vals;
    int32_t* cnt_rank;
};

template <bool IN_LDS>
__global__ __launch_bounds__(TPB) void k_query(QueryArgs a) {
    extern __shared__ int32_t lds[];
    __shared__ int s_bad, s_max, s_nt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot_hi = a.slot_hi;
    int32_t* cnt = IN_LDS ? lds : a.cnt_rank + (size_t)blockIdx.x * 2 * a.capacity;
    int32_t* rnk = cnt + (IN_LDS ? slot_hi : a.capacity);
    unsigned long long* keys = a.keys + (size_t)blockIdx.x * a.sort_cap;
    int32_t* vals = a.vals + (size_t)blockIdx.x * a.sort_cap;
    for (int q = blockIdx.x; q < a.nq; q += gridDim.x) {
        const int n = a.q_n[q];
        const uint32_t* qid = a.q_id + (size_t)q * a.qcap;
        const int x0 = a.excl_off ? a.excl_off[q] : 0, x1 = a.excl_off ? a.excl_off[q + 1] : 0;
        if (tid == 0) { s_bad = (n < 0 || n > a.qcap || x1 < x0); s_max = 0; s_nt = 0; }
        for (int s = tid; s < slot_hi; s += TPB) { cnt[s] = 0; rnk[s] = RANK_NONE; }
        __syncthreads();
        if (!s_bad) {
            for (int i = tid; i < n; i += TPB)
                if (qid[i] >= (uint32_t)a.n_words || (i > 0 && qid[i - 1] >= qid[i])) atomicOr(&s_bad, 1);
            for (int k = x0 + tid; k < x1; k += TPB)
                if (a.excl_slot[k] < 0 || a.excl_slot[k] >= a.capacity) atomicOr(&s_bad, 1);
        }
        __syncthreads();
        if (s_bad) {
            if (tid == 0) { a.status[q] = ORBX_ERR_ARG; a.n_share[q] = 0; a.min_common[q] = 0; }
            __syncthreads();
            continue;
        }
        // 1. the inverted-file walk (:88-104, :205-222): hits per slot and the rank of the first shared query word
        for (int i = wave; i < n; i += TPB / 64) {
            const uint32_t w = qid[i];
            const int b = a.word_off[w], e = a.word_off[w + 1];
            for (int j = b + lane; j < e; j += 64) {
                const int s = a.list[j];
                atomicAdd(&cnt[s], 1);
                atomicMin(&rnk[s], i);
            }
        }
        __syncthreads();
        // 2. exclusions: their counts go out, then they leave the list
        for (int k = x0 + tid; k < x1; k += TPB) {
            const int s = a.excl_slot[k];
            a.excl_words[k] = s < slot_hi ? cnt[s] : 0;
        }
        __syncthreads();
        for (int k = x0 + tid; k < x1; k += TPB) {
            const int s = a.excl_slot[k];
            if (s < slot_hi) cnt[s] = 0;
        }
        __syncthreads();
        // 3. max count (:113-118, :228-233) and the touched slots, keyed by (first-touch rank, add sequence)
        for (int s = tid; s < slot_hi; s += TPB) {
            const int c = cnt[s];
            if (c > 0) {
                atomicMax(&s_max, c);
                const int p = atomicAdd(&s_nt, 1);
                keys[p] = ((unsigned long long)(uint32_t)rnk[s] << 32) | a.slot_seq[s];
                vals[p] = s;
            }
        }
        __syncthreads();
        const int nt = s_nt;
        const int minc = (int)((float)s_max * 0.8f);      // int minCommonWords = maxCommonWords*0.8f  (:120, :234)
        if (tid == 0) {
            a.n_share[q] = nt;
            a.min_common[q] = minc;
            a.status[q] = nt > a.out_cap ? ORBX_ERR_CAPACITY : ORBX_OK;
        }
        if (nt > a.out_cap) { __syncthreads(); continue; }
        // 4. bitonic sort of the nt keys (padded to a power of two) in the workgroup's row
        int P = 1;
        while (P < nt) P <<= 1;
        for (int p = nt + tid; p < P; p += TPB) keys[p] = ~0ull;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < P / 2; i += TPB) {
                    const int lo = 2 * i - (i & (j - 1)), hi = lo + j;
                    const bool up = (lo & k) == 0;
                    const unsigned long long kl = keys[lo], kh = keys[hi];
                    if ((kl > kh) == up) {
                        keys[lo] = kh; keys[hi] = kl;
                        const int32_t t = vals[lo]; vals[lo] = vals[hi]; vals[hi] = t;
                    }
                }
                __syncthreads();
            }
        }
        // 5. the list, the counts, and the scores above the threshold (:122-134, :238-250): one lane per slot, one
        //    sequential sum in ascending word order
        for (int j = tid; j < nt; j += TPB) {
            const int s = vals[j];
            const int c = cnt[s];
            const size_t o = (size_t)q * a.out_cap + j;
            a.share_slot[o] = s;
            a.share_words[o] = c;
            double sc = 0.0;
            if (c > minc) {
                const int off = a.slot_off[s];
                sc = orbv::score_walk(a.scoring, qid, a.q_val + (size_t)q * a.qcap, n, a.ent_id + off, a.ent_val + off, a.slot_n[s]);
            }
            a.share_score[o] = sc;
        }
        __syncthreads();
    }
}

}  // namespace orbd

// ------------------------------------------------------------------------------------------------ host side
namespace {

using orbx::DeviceScope;

struct SlotHost {
    int32_t off = 0, res = 0;    // segment offset and reserved length in the arena
    uint32_t seq = 0;
    bool present = false;
};

}  // namespace

struct __attribute__((visibility("hidden"))) orbd_database {
    int device = 0, capacity = 0, n_words = 0, scoring = 0;
    int sort_cap = 1, rows = 1;          // query scratch: rows workgroups of sort_cap keys each
    std::mutex mu;
    std::vector<SlotHost> slots;
    int n_present = 0, slot_hi = 0;
    long long arena_hi = 0, arena_cap = 0, live_res = 0;
    uint32_t next_seq = 0;
    bool dirty = true;
    orbx::DevBuf ent_id, ent_val, ent_slot, list;
    orbx::DevBuf slot_off, slot_n, slot_seq;
    orbx::DevBuf word_off, cursor;
    orbx::DevBuf keys, vals, cnt_rank;
    orbx::DevBuf d_tab, stage, q_stage;
    orbx::PinnedBuf h_tab;
    orbx::Stream own;
    orbx::Chain chain;                   // every piece of device work on the database waits for the previous one, whichever stream carried it
    orbx::Event tab_done;
    bool tab_pending = false;
};

namespace {

hipError_t alloc_arena(orbd_database* db, long long cap, orbx::DevBuf& id, orbx::DevBuf& val, orbx::DevBuf& slot) {
    hipError_t e = id.ensure((size_t)cap * 4);
    if (e == hipSuccess) e = val.ensure((size_t)cap * 8);
    if (e == hipSuccess) e = slot.ensure((size_t)cap * 4);
    return e;
}

// room for `need` more entries at arena_hi: grows the arena (live segments copied in add order) when it does not fit.
// Synchronous: it runs inside an add.
int reserve(orbd_database* db, long long need, hipStream_t st) {
    if (db->arena_hi + need <= db->arena_cap) return ORBX_OK;
    const long long cap = std::max<long long>(2 * (db->live_res + need), 1 << 16);
    if (cap > INT_MAX) return ORBX_ERR_CAPACITY;
    orbx::DevBuf id, val, slot;
    HIPTRY(alloc_arena(db, cap, id, val, slot));
    std::vector<int> order;
    for (int s = 0; s < db->capacity; s++) if (db->slots[s].present) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return db->slots[a].off < db->slots[b].off; });
    std::vector<int32_t> tab;
    int32_t pos = 0;
    for (int s : order) { tab.insert(tab.end(), {s, pos, db->slots[s].res}); db->slots[s].off = pos; pos += db->slots[s].res; }
    HIPTRY(db->chain.begin(st));
    if (!order.empty()) {
        orbx::DevBuf d;
        HIPTRY(d.ensure(tab.size() * 4));
        HIPTRY(hipMemcpyAsync(d.as(), tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        orbd::k_compact<<<(int)order.size(), orbd::TPB, 0, st>>>((int)order.size(), d.as<int32_t>(), db->ent_id.as<uint32_t>(),
                                                                 db->ent_val.as<double>(), db->ent_slot.as<int32_t>(), id.as<uint32_t>(),
                                                                 val.as<double>(), slot.as<int32_t>(), db->slot_off.as<int32_t>());
        HIPTRY(hipGetLastError());
        HIPTRY(hipStreamSynchronize(st));
    }
    db->ent_id = std::move(id);
    db->ent_val = std::move(val);
    db->ent_slot = std::move(slot);
    HIPTRY(db->list.ensure((size_t)cap * 4));
    HIPTRY(db->chain.end(st));
    db->arena_cap = cap;
    db->arena_hi = pos;
    db->dirty = true;
    return ORBX_OK;
}

// the inverted file from the live entries (on the query's stream, inside its chain link)
hipError_t rebuild(orbd_database* db, hipStream_t st) {
    const int nw = db->n_words;
    hipError_t e = hipMemsetAsync(db->word_off.as(), 0, ((size_t)nw + 1) * 4, st);
    const int n_ent = (int)db->arena_hi;
    if (e == hipSuccess && n_ent > 0) {
        orbd::k_hist<<<(n_ent + orbd::TPB - 1) / orbd::TPB, orbd::TPB, 0, st>>>(n_ent, db->ent_id.as<uint32_t>(), db->ent_slot.as<int32_t>(),
                                                                               db->slot_off.as<int32_t>(), db->slot_n.as<int32_t>(),
                                                                               db->word_off.as<int32_t>());
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        orbd::k_scan<<<1, orbd::SCAN_TPB, 0, st>>>(nw + 1, db->word_off.as<int32_t>(), db->cursor.as<int32_t>());
        e = hipGetLastError();
    }
    if (e == hipSuccess && n_ent > 0) {
        orbd::k_scatter<<<(n_ent + orbd::TPB - 1) / orbd::TPB, orbd::TPB, 0, st>>>(n_ent, db->ent_id.as<uint32_t>(), db->ent_slot.as<int32_t>(),
                                                                                  db->slot_off.as<int32_t>(), db->slot_n.as<int32_t>(),
                                                                                  db->cursor.as<int32_t>(), db->list.as<int32_t>());
        e = hipGetLastError();
    }
    if (e == hipSuccess) db->dirty = false;
    return e;
}

int usable_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return ORBX_ERR_DEVICE;
    return ORBX_OK;
}

// the add path shared by both forms: frames already checked on the host, slot table in db->d_tab, `res` entries reserved each
int launch_add(orbd_database* db, const int32_t* slots, int nframes, const uint32_t* d_id, const double* d_val, const int32_t* d_n, int cap,
               int32_t* d_status, hipStream_t st) {
    const int rc = reserve(db, (long long)nframes * cap, st);
    if (rc != ORBX_OK) return rc;
    if (db->tab_pending) HIPTRY(hipEventSynchronize(db->tab_done));
    std::copy(slots, slots + nframes, db->h_tab.as<int32_t>());
    HIPTRY(db->chain.begin(st));
    HIPTRY(hipMemcpyAsync(db->d_tab.as(), db->h_tab.as(), (size_t)nframes * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipEventRecord(db->tab_done, st));
    db->tab_pending = true;
    orbd::k_add<<<nframes, orbd::TPB, 0, st>>>(nframes, db->d_tab.as<int32_t>(), db->arena_hi, cap, db->next_seq, d_id, d_val, d_n, db->n_words,
                                               db->ent_id.as<uint32_t>(), db->ent_val.as<double>(), db->ent_slot.as<int32_t>(),
                                               db->slot_off.as<int32_t>(), db->slot_n.as<int32_t>(), db->slot_seq.as<uint32_t>(), d_status);
    HIPTRY(hipGetLastError());
    HIPTRY(db->chain.end(st));
    for (int f = 0; f < nframes; f++) {
        SlotHost& h = db->slots[slots[f]];
        h.present = true;
        h.off = (int32_t)(db->arena_hi + (long long)f * cap);
        h.res = cap;
        h.seq = db->next_seq + f;
        db->slot_hi = std::max(db->slot_hi, slots[f] + 1);
    }
    db->n_present += nframes;
    db->live_res += (long long)nframes * cap;
    db->arena_hi += (long long)nframes * cap;
    db->next_seq += nframes;
    db->dirty = true;
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbd_create(const orbv_vocabulary* voc, int capacity, int device, orbd_database** out) {
    if (!out || capacity < 1 || capacity > ORBD_MAX_CAPACITY) return ORBX_ERR_ARG;
    *out = nullptr;
    if (usable_device(device) != ORBX_OK) return ORBX_ERR_DEVICE;
    int k, L, sc, wt, nw, nn;
    if (!voc || orbv_info(voc, &k, &L, &sc, &wt, &nw, &nn) != ORBX_OK) return ORBX_ERR_ARG;
    if (sc == ORBV_KL || sc < 0 || sc > ORBV_DOT_PRODUCT) return ORBX_ERR_ARG;
    DeviceScope ds(device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    orbd_database* db = new orbd_database;
    db->device = device;
    db->capacity = capacity;
    db->n_words = nw;
    db->scoring = sc;
    db->slots.resize(capacity);
    while (db->sort_cap < capacity) db->sort_cap <<= 1;
    // query scratch: up to 512 workgroups, about 64 MiB at the largest capacities
    const size_t row = (size_t)db->sort_cap * 12 + (capacity > orbd::LDS_SLOTS ? (size_t)capacity * 8 : 0);
    db->rows = (int)std::max<size_t>(16, std::min<size_t>(512, ((size_t)64 << 20) / row));
    auto fail = [&](int rc) { delete db; return rc; };
    if (db->slot_off.ensure((size_t)capacity * 4) != hipSuccess || db->slot_n.ensure((size_t)capacity * 4) != hipSuccess ||
        db->slot_seq.ensure((size_t)capacity * 4) != hipSuccess || db->d_tab.ensure((size_t)capacity * 4) != hipSuccess ||
        db->h_tab.ensure((size_t)capacity * 4, hipHostMallocDefault) != hipSuccess ||
        db->word_off.ensure(((size_t)nw + 1) * 4) != hipSuccess || db->cursor.ensure(((size_t)nw + 1) * 4) != hipSuccess ||
        db->keys.ensure((size_t)db->rows * db->sort_cap * 8) != hipSuccess || db->vals.ensure((size_t)db->rows * db->sort_cap * 4) != hipSuccess ||
        (capacity > orbd::LDS_SLOTS && db->cnt_rank.ensure((size_t)db->rows * capacity * 8) != hipSuccess) ||
        db->list.ensure(4) != hipSuccess || db->own.ensure() != hipSuccess || db->chain.ev.ensure() != hipSuccess ||
        db->tab_done.ensure() != hipSuccess)
        return fail(ORBX_ERR_DEVICE);
    if (hipMemset(db->slot_off.as(), 0, (size_t)capacity * 4) != hipSuccess ||
        hipMemset(db->slot_n.as(), 0xff, (size_t)capacity * 4) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&orbd::k_query<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            orbd::LDS_SLOTS * 8) != hipSuccess)
        return fail(ORBX_ERR_DEVICE);
    *out = db;
    return ORBX_OK;
}

void orbd_destroy(orbd_database* db) {
    if (!db) return;
    DeviceScope ds(db->device);
    (void)db->chain.wait();                                     // the last piece of device work on the database
    delete db;
}

int orbd_size(const orbd_database* db) { return db ? db->n_present : 0; }

int orbd_add(orbd_database* db, int slot, const uint32_t* ids, const double* vals, int n) {
    if (!db || slot < 0 || slot >= db->capacity || n < 0 || (n > 0 && (!ids || !vals))) return ORBX_ERR_ARG;
    for (int i = 0; i < n; i++)
        if (ids[i] >= (uint32_t)db->n_words || (i > 0 && ids[i - 1] >= ids[i])) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    if (db->slots[slot].present) return ORBX_ERR_ARG;
    DeviceScope ds(db->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = db->own;
    // one staging block: n ids, n values, the count (reused across adds; the add is synchronous)
    const size_t o_val = ((size_t)n * 4 + 7) & ~(size_t)7, o_n = o_val + (size_t)n * 8;
    HIPTRY(db->chain.begin(st));
    HIPTRY(hipStreamSynchronize(st));
    HIPTRY(db->stage.ensure(o_n + 4));
    const int32_t nn = n;
    if (n > 0) {
        HIPTRY(hipMemcpyAsync(db->stage.as(), ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPTRY(hipMemcpyAsync(db->stage.as() + o_val, vals, (size_t)n * 8, hipMemcpyHostToDevice, st));
    }
    HIPTRY(hipMemcpyAsync(db->stage.as() + o_n, &nn, 4, hipMemcpyHostToDevice, st));
    const int rc = launch_add(db, &slot, 1, db->stage.as<uint32_t>(), reinterpret_cast<const double*>(db->stage.as() + o_val),
                              reinterpret_cast<const int32_t*>(db->stage.as() + o_n), n, nullptr, st);
    if (rc != ORBX_OK) return rc;
    HIPTRY(hipStreamSynchronize(st));
    return ORBX_OK;
}

int orbd_add_batch_device(orbd_database* db, const int32_t* slots, int nframes, const uint32_t* d_bow_id, const double* d_bow_val,
                          const int32_t* d_n_bow, int cap, int32_t* d_status, void* stream) {
    if (!db || nframes < 0 || cap < 0 || (nframes > 0 && (!slots || !d_n_bow || (cap > 0 && (!d_bow_id || !d_bow_val)))))
        return ORBX_ERR_ARG;
    if (nframes == 0) return ORBX_OK;
    std::lock_guard<std::mutex> lock(db->mu);
    std::vector<char> seen(db->capacity, 0);
    for (int f = 0; f < nframes; f++) {
        const int s = slots[f];
        if (s < 0 || s >= db->capacity || db->slots[s].present || seen[s]) return ORBX_ERR_ARG;
        seen[s] = 1;
    }
    DeviceScope ds(db->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    return launch_add(db, slots, nframes, d_bow_id, d_bow_val, d_n_bow, cap, d_status, static_cast<hipStream_t>(stream));
}

int orbd_erase(orbd_database* db, int slot) {
    if (!db || slot < 0 || slot >= db->capacity) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    SlotHost& h = db->slots[slot];
    if (!h.present) return ORBX_OK;
    DeviceScope ds(db->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = db->own;
    HIPTRY(db->chain.begin(st));
    HIPTRY(hipMemsetAsync(db->slot_n.as<int32_t>() + slot, 0xff, 4, st));
    HIPTRY(db->chain.end(st));
    h.present = false;
    db->n_present--;
    db->live_res -= h.res;
    db->dirty = true;
    return ORBX_OK;
}

int orbd_clear(orbd_database* db) {
    if (!db) return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    DeviceScope ds(db->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = db->own;
    HIPTRY(db->chain.begin(st));
    HIPTRY(hipMemsetAsync(db->slot_n.as(), 0xff, (size_t)db->capacity * 4, st));
    HIPTRY(db->chain.end(st));
    for (SlotHost& h : db->slots) h = SlotHost{};
    db->n_present = 0;
    db->slot_hi = 0;
    db->arena_hi = 0;
    db->live_res = 0;
    db->dirty = true;
    return ORBX_OK;
}

static int query_locked(orbd_database* db, int nq, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_n_bow, int qcap,
                        const int32_t* d_excl_off, const int32_t* d_excl_slot, int32_t* d_excl_words, int32_t* d_share_slot,
                        int32_t* d_share_words, double* d_share_score, int out_cap, int32_t* d_n_share, int32_t* d_min_common,
                        int32_t* d_status, hipStream_t st) {
    HIPTRY(db->chain.begin(st));
    if (db->dirty) HIPTRY(rebuild(db, st));
    orbd::QueryArgs a;
    a.nq = nq; a.qcap = qcap; a.n_words = db->n_words; a.capacity = db->capacity; a.slot_hi = db->slot_hi;
    a.sort_cap = db->sort_cap; a.scoring = db->scoring; a.out_cap = out_cap;
    a.q_id = d_bow_id; a.q_val = d_bow_val; a.q_n = d_n_bow;
    a.excl_off = d_excl_off; a.excl_slot = d_excl_slot; a.excl_words = d_excl_words;
    a.share_slot = d_share_slot; a.share_words = d_share_words; a.share_score = d_share_score;
    a.n_share = d_n_share; a.min_common = d_min_common; a.status = d_status;
    a.word_off = db->word_off.as<int32_t>(); a.list = db->list.as<int32_t>();
    a.ent_id = db->ent_id.as<uint32_t>(); a.ent_val = db->ent_val.as<double>();
    a.slot_off = db->slot_off.as<int32_t>(); a.slot_n = db->slot_n.as<int32_t>(); a.slot_seq = db->slot_seq.as<uint32_t>();
    a.keys = db->keys.as<unsigned long long>(); a.vals = db->vals.as<int32_t>(); a.cnt_rank = db->cnt_rank.as<int32_t>();
    const int grid = std::min(nq, db->rows);
    if (db->slot_hi <= orbd::LDS_SLOTS)
        orbd::k_query<true><<<grid, orbd::TPB, (size_t)std::max(db->slot_hi, 1) * 8, st>>>(a);
    else
        orbd::k_query<false><<<grid, orbd::TPB, 0, st>>>(a);
    HIPTRY(hipGetLastError());
    HIPTRY(db->chain.end(st));
    return ORBX_OK;
}

int orbd_query_batch_device(orbd_database* db, int nq, const uint32_t* d_bow_id, const double* d_bow_val, const int32_t* d_n_bow, int qcap,
                            const int32_t* d_excl_off, const int32_t* d_excl_slot, int32_t* d_excl_words, int32_t* d_share_slot,
                            int32_t* d_share_words, double* d_share_score, int out_cap, int32_t* d_n_share, int32_t* d_min_common,
                            int32_t* d_status, void* stream) {
    if (!db || nq < 0 || qcap < 0 || out_cap < 0 || (d_excl_off && (!d_excl_slot || !d_excl_words))) return ORBX_ERR_ARG;
    if (nq == 0) return ORBX_OK;
    if (!d_n_bow || (qcap > 0 && (!d_bow_id || !d_bow_val)) || !d_n_share || !d_min_common || !d_status ||
        (out_cap > 0 && (!d_share_slot || !d_share_words || !d_share_score)))
        return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    DeviceScope ds(db->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    return query_locked(db, nq, d_bow_id, d_bow_val, d_n_bow, qcap, d_excl_off, d_excl_slot, d_excl_words, d_share_slot, d_share_words,
                        d_share_score, out_cap, d_n_share, d_min_common, d_status, static_cast<hipStream_t>(stream));
}

int orbd_query(orbd_database* db, const uint32_t* ids, const double* vals, int n, const int32_t* excl_slot, int n_excl, int32_t* excl_words,
               int32_t* share_slot, int32_t* share_words, double* share_score, int out_cap, int* n_share, int* min_common, void* stream) {
    if (!db || n < 0 || n_excl < 0 || out_cap < 0 || !n_share || !min_common || (n > 0 && (!ids || !vals)) ||
        (n_excl > 0 && (!excl_slot || !excl_words)) || (out_cap > 0 && (!share_slot || !share_words || !share_score)))
        return ORBX_ERR_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    DeviceScope ds(db->device);
    if (!ds.ok) return ORBX_ERR_DEVICE;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(db->own);
    // one staging block, kept by the database (it grows, never shrinks): the query (ids, values, count), the exclusion CSR, the outputs
    orbx::Layout L;
    const auto s_val = L.add<double>(n);
    const auto s_id = L.add<uint32_t>(n);
    const auto s_n = L.add<int32_t>(1), s_xoff = L.add<int32_t>(2), s_xs = L.add<int32_t>(n_excl), s_xw = L.add<int32_t>(n_excl);
    const auto s_score = L.add<double>(out_cap);
    const auto s_slot = L.add<int32_t>(out_cap), s_words = L.add<int32_t>(out_cap), s_res = L.add<int32_t>(3);
    HIPTRY(db->chain.begin(st));
    HIPTRY(hipStreamSynchronize(st));       // the staging block is free once earlier work on the database is done
    HIPTRY(db->q_stage.ensure(L.total()));
    uint8_t* base = db->q_stage.as();
    uint32_t* q_id = L.at(base, s_id);
    double* q_val = L.at(base, s_val);
    double* r_score = L.at(base, s_score);
    int32_t* q_n = L.at(base, s_n);
    int32_t* x_off = L.at(base, s_xoff);
    int32_t* x_slot = L.at(base, s_xs);
    int32_t* x_words = L.at(base, s_xw);
    int32_t* r_slot = L.at(base, s_slot);
    int32_t* r_words = L.at(base, s_words);
    int32_t* res = L.at(base, s_res);       // n_share, min_common, status
    const int32_t hn = n, hx[2] = {0, n_excl};
    if (n > 0) {
        HIPTRY(hipMemcpyAsync(q_id, ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPTRY(hipMemcpyAsync(q_val, vals, (size_t)n * 8, hipMemcpyHostToDevice, st));
    }
    HIPTRY(hipMemcpyAsync(q_n, &hn, 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(x_off, hx, 8, hipMemcpyHostToDevice, st));
    if (n_excl > 0) HIPTRY(hipMemcpyAsync(x_slot, excl_slot, (size_t)n_excl * 4, hipMemcpyHostToDevice, st));
    const int rc = query_locked(db, 1, q_id, q_val, q_n, n, x_off, x_slot, x_words, r_slot, r_words, r_score, out_cap, res, res + 1, res + 2, st);
    if (rc != ORBX_OK) return rc;
    int32_t h[3] = {0, 0, 0};
    HIPTRY(hipMemcpyAsync(h, res, 12, hipMemcpyDeviceToHost, st));
    HIPTRY(hipStreamSynchronize(st));
    *n_share = h[0];
    *min_common = h[1];
    if (h[2] != ORBX_OK) return h[2];
    if (n_excl > 0) HIPTRY(hipMemcpyAsync(excl_words, x_words, (size_t)n_excl * 4, hipMemcpyDeviceToHost, st));
    if (h[0] > 0) {
        HIPTRY(hipMemcpyAsync(share_slot, r_slot, (size_t)h[0] * 4, hipMemcpyDeviceToHost, st));
        HIPTRY(hipMemcpyAsync(share_words, r_words, (size_t)h[0] * 4, hipMemcpyDeviceToHost, st));
        HIPTRY(hipMemcpyAsync(share_score, r_score, (size_t)h[0] * 8, hipMemcpyDeviceToHost, st));
    }
    HIPTRY(hipStreamSynchronize(st));
    return ORBX_OK;
}

}  // extern "C"
