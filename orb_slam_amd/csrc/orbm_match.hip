// Brute-force 256-bit Hamming matching for gfx950: the inner loop of every ORBmatcher search
// (reference src/ORBmatcher.cc:201-222 and siblings: DescriptorDistance + running best/second-best
// with strict '<') lifted to a dense N x M kernel.
//
// Mapping (integer/bitwise work, no MFMA): a lane owns QPL query descriptors in VGPRs (8 dwords
// each).  The train descriptor of the current step is the same for the whole wave, so it is read
// with wave-uniform (scalar, SGPR) loads and costs no VGPRs, no LDS and no per-lane memory traffic.
// Per pair: 8 v_xor + 8 v_bcnt_u32_b32 (accumulating popcount) + 3 ops for the top-2 update.
//
// Top-2 with the reference's tie rules as ONE associative reduction: key = (distance << 22) | index.
// Keys are unique, min(key) is the smallest distance at its FIRST index, and the second-smallest
// key carries the second-smallest distance counted with multiplicity — exactly what the
// `if(d<best){best2=best;best=d;idx=i}else if(d<best2)best2=d` scan produces.  Because it is a
// plain two-smallest reduction, the train set can be split across workgroups and merged in any order.
#include <atomic>
#include <climits>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "orb_math.h"
#include "orbx_internal.h"

namespace orbx {

constexpr int KEY_SHIFT = 22;                       // index bits; distance (<=256) sits above
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;
#ifndef ORBX_MATCH_BLOCK
#define ORBX_MATCH_BLOCK 256
#endif
constexpr int MATCH_BLOCK = ORBX_MATCH_BLOCK;

// k1 <= k2 are the two smallest keys so far: the new second-smallest is the median of (k1, k2, key)
__device__ __forceinline__ void top2_update(uint32_t& k1, uint32_t& k2, uint32_t key) {
    uint32_t m;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(m) : "v"(k1), "v"(k2), "v"(key));
    k2 = m;
    k1 = min(k1, key);
}

// popcount(x) + acc in ONE VALU op (v_bcnt_u32_b32 accumulates); the compiler otherwise builds an add tree
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// Scan train descriptors [t0, t1) for the block's queries.  T must be wave-uniform readable.
template <int QPL>
__device__ __forceinline__ void scan_range(const uint32_t* __restrict__ T, int t0, int t1, const uint32_t (&q)[QPL][8],
                                           uint32_t (&k1)[QPL], uint32_t (&k2)[QPL]) {
    auto one = [&](const uint32_t (&tw)[8], int t) {
#pragma unroll
        for (int j = 0; j < QPL; j++) {
            uint32_t d = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) d = bcnt_acc(q[j][i] ^ tw[i], d);
            top2_update(k1[j], k2[j], (d << KEY_SHIFT) | (uint32_t)t);
        }
    };
    int t = t0;
    // 4 train descriptors per trip: their scalar loads are issued together, so the s_load latency is paid once per 4
    for (; t + 4 <= t1; t += 4) {
        uint32_t tw[4][8];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t* tp = T + (long long)(t + u) * 8;
#pragma unroll
            for (int i = 0; i < 8; i++) tw[u][i] = tp[i];   // uniform address -> s_load_dwordx8
        }
#pragma unroll
        for (int u = 0; u < 4; u++) one(tw[u], t + u);
    }
    for (; t < t1; t++) {
        const uint32_t* tp = T + (long long)t * 8;
        uint32_t tw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) tw[i] = tp[i];
        one(tw, t);
    }
}

struct __attribute__((aligned(4))) dwords4 { uint32_t x, y, z, w; };    // a 16-byte load that only assumes dword alignment

template <int QPL>
__device__ __forceinline__ void load_queries(const uint32_t* __restrict__ Q, int nq, int qbase, uint32_t (&q)[QPL][8]) {
#pragma unroll
    for (int j = 0; j < QPL; j++) {
        const int qi = qbase + j * MATCH_BLOCK;
        if (qi < nq) {
            // 16 bytes per load, 4-byte alignment: all the reference asks of a descriptor row (it reads 8 x int32, src/ORBmatcher.cc:1796-1801)
            const dwords4* p = reinterpret_cast<const dwords4*>(Q + (long long)qi * 8);
            const dwords4 a = p[0], c = p[1];
            q[j][0] = a.x; q[j][1] = a.y; q[j][2] = a.z; q[j][3] = a.w;
            q[j][4] = c.x; q[j][5] = c.y; q[j][6] = c.z; q[j][7] = c.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) q[j][i] = 0;
        }
    }
}

__device__ __forceinline__ void write_result(uint32_t k1, uint32_t k2, int32_t* idx, int32_t* best, int32_t* second) {
    *idx = (k1 == KEY_NONE) ? -1 : (int32_t)(k1 & ((1u << KEY_SHIFT) - 1));
    *best = (k1 == KEY_NONE) ? INT_MAX : (int32_t)(k1 >> KEY_SHIFT);
    *second = (k2 == KEY_NONE) ? INT_MAX : (int32_t)(k2 >> KEY_SHIFT);
}

// Large single problem: grid = (query blocks, train splits); partial (k1,k2) per (split, query).
template <int QPL>
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_split(const uint32_t* __restrict__ Q, int nq, const uint32_t* __restrict__ T, int nt,
                                                             int chunk, uint32_t* __restrict__ pk1, uint32_t* __restrict__ pk2) {
    const int qbase = blockIdx.x * (MATCH_BLOCK * QPL) + threadIdx.x;
    const int t0 = blockIdx.y * chunk, t1 = min(nt, t0 + chunk);
    uint32_t q[QPL][8], k1[QPL], k2[QPL];
    load_queries<QPL>(Q, nq, qbase, q);
#pragma unroll
    for (int j = 0; j < QPL; j++) { k1[j] = KEY_NONE; k2[j] = KEY_NONE; }
    scan_range<QPL>(T, t0, t1, q, k1, k2);
#pragma unroll
    for (int j = 0; j < QPL; j++) {
        const int qi = qbase + j * MATCH_BLOCK;
        if (qi < nq) {
            pk1[(long long)blockIdx.y * nq + qi] = k1[j];
            pk2[(long long)blockIdx.y * nq + qi] = k2[j];
        }
    }
}

__global__ __launch_bounds__(256) void k_match_merge(const uint32_t* __restrict__ pk1, const uint32_t* __restrict__ pk2, int nq, int nsplit,
                                                     int32_t* __restrict__ idx, int32_t* __restrict__ best, int32_t* __restrict__ second) {
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    uint32_t k1 = KEY_NONE, k2 = KEY_NONE;
    for (int s = 0; s < nsplit; s++) {
        top2_update(k1, k2, pk1[(long long)s * nq + qi]);
        top2_update(k1, k2, pk2[(long long)s * nq + qi]);
    }
    write_result(k1, k2, idx + qi, best + qi, second + qi);
}

// Many small problems (frame-to-frame matching): blockIdx.y = problem, sizes read on the device.
template <int QPL>
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_batch(const uint32_t* __restrict__ Q, const int32_t* __restrict__ nqs,
                                                             const uint32_t* __restrict__ T, const int32_t* __restrict__ nts, int cap,
                                                             int32_t* __restrict__ idx, int32_t* __restrict__ best, int32_t* __restrict__ second) {
    const int prob = blockIdx.y;
    const int nq = min(nqs[prob], cap), nt = min(nts[prob], cap);
    const int qbase = blockIdx.x * (MATCH_BLOCK * QPL) + threadIdx.x;
    if (blockIdx.x * (MATCH_BLOCK * QPL) >= nq) return;
    const uint32_t* Qp = Q + (long long)prob * cap * 8;
    const uint32_t* Tp = T + (long long)prob * cap * 8;
    uint32_t q[QPL][8], k1[QPL], k2[QPL];
    load_queries<QPL>(Qp, nq, qbase, q);
#pragma unroll
    for (int j = 0; j < QPL; j++) { k1[j] = KEY_NONE; k2[j] = KEY_NONE; }
    scan_range<QPL>(Tp, 0, nt, q, k1, k2);
#pragma unroll
    for (int j = 0; j < QPL; j++) {
        const int qi = qbase + j * MATCH_BLOCK;
        if (qi < nq) {
            const long long o = (long long)prob * cap + qi;
            write_result(k1[j], k2[j], idx + o, best + o, second + o);
        }
    }
}

// ------------------------------------------------------------------------------------ Hamming by MFMA
// Encode bit b of a descriptor as an int8 (b ? +v : -v): for two descriptors the dot product is v_q * v_t * (#agreeing - #differing
// bits) = v_q v_t (256 - 2 hamming), exact in the i32 accumulator.  v_mfma_i32_32x32x32_i8 does a 32 x 32 block of pairs per 8
// instructions (K = 256): ~3.5 pairs per cycle and SIMD against ~0.2 for the xor + popcount form, and the matrix pipe runs beside
// the VALU, which is left with the top-2 bookkeeping (v_med3 + v_min per pair).
//   A (32 trains x 32 k): lane l supplies row l % 32, k-bytes 16 * (l / 32) .. + 15 of the chunk;  B (32 k x 32 queries): likewise
//   with the query as column;  D: lane l holds column (query) l % 32, register r row (train) 8 * (r / 4) + 4 * (l / 32) + r % 4
//   (tools/microbench/mfma_layout.hip checks this on the device).  Both operands use the same bit -> k map, so its order is free.
// Workgroup = 4 waves; wave w keeps QT = 4 tiles of 32 queries as B operands (+-1) in registers for the whole scan.  Train tiles of
// 32 descriptors are expanded cooperatively into LDS (-+64, i.e. negated and scaled) through a 256-entry byte -> 8 bytes table
// and kept in a ring of four; rows are padded to 272 bytes so that the 16-byte operand reads of 16 consecutive lanes cover all
// 64 banks.  Measured (100k x 100k): 1.75 ms = 5.7e12 pairs/s (round 2: 1.99) against 5.2 ms for the popcount kernels; 1024 x
// (1000 x 1000): 0.21 (0.26) against 0.57 ms.  What did not work: a min3 tree per tile with the key updates only behind a wave vote (the vote fires
// for ~half the tiles at these chunk lengths and its branches keep the scheduler from pairing VALU with MFMAs: 3.2 ms).
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x16_t __attribute__((ext_vector_type(16)));
constexpr int MF_PITCH = 272;                      // bytes per expanded train row in LDS (256 + 16)
constexpr int MF_TILE_BYTES = 32 * MF_PITCH;
constexpr int MF_LDS_BYTES = 4096 + 4 * MF_TILE_BYTES;   // two tables + ring of four train tiles
// Query tiles of 32 per wave.  Round 2 ran chunk-major (every chunk's MFMA for all QT tiles, 2 x QT accumulator sets): QT = 2 at 199
// VGPRs was all that fitted two waves per SIMD (QT = 3 / 4 at one wave: 100k x 100k 1.99 / 2.58 / 2.25 ms).  The chain-major loop
// below keeps two accumulator sets whatever QT is, so QT = 4 fits 256 VGPRs (amdgpu_waves_per_eu(2, 2) on the kernels; one B
// register quad is spilled around the first tile, nothing inside the loop): 100k x 100k 1.75 ms, per-frame batches 0.212 ms per 1024
// frames (chain-major with QT = 2: 1.98 / 0.246; QT = 4 at one wave per SIMD: 2.18 / 0.290).
#ifndef ORBX_MF_QT
#define ORBX_MF_QT 4
#endif
constexpr int MF_QT = ORBX_MF_QT;

// Per-query-tile scan state as four named scalars per field: an array here is promoted to a vector register tuple, and every
// conditional update then shuffles the whole tuple (v_mov_b64 x 4 per key).
struct Top2State {
    uint32_t a0, a1, a2, a3;
    template <int I> __device__ __forceinline__ uint32_t& at() {
        if constexpr (I == 0) return a0; else if constexpr (I == 1) return a1; else if constexpr (I == 2) return a2; else return a3;
    }
};
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) { static_for<N - 1>(f); f(std::integral_constant<int, N - 1>{}); }
}

template <int QT>
__device__ __forceinline__ void mfma_scan(const uint32_t* __restrict__ Qp, int nq, int qblock0, const uint32_t* __restrict__ Tp, int t0, int t1,
                                          uint8_t* smem, Top2State& K1, Top2State& K2) {
    static_assert(QT >= 1 && QT <= 4, "Top2State holds four tiles");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, kh = lane >> 5;
    uint2* lut = reinterpret_cast<uint2*>(smem);                // lut[v]: byte j of the pair = bit j of v as +1 (0x01) / -1 (0xFF)   (queries)
    uint2* lut64 = lut + 256;                                   // lut64[v]: ... as +64 (0x40) / -64 (0xC0)                           (trains, looked up with ~v)
    uint8_t* tiles = smem + 4096;
    const int ntiles = (t1 - t0 + 31) >> 5;
    // Every global load of the prologue is requested before anything waits (round 5): the queries' 8 dwords per lane and tile and the
    // first four train tiles, from CLAMPED indices instead of under `if (valid)` — queries past nq are never written, train rows past t1
    // are masked by the last tile's chains, so what they hold does not matter.  (The guarded form compiled to one load + s_waitcnt
    // vmcnt(0) + table lookups per dword: 32 dependent round trips in front of a workgroup's first MFMA — half the life of a
    // workgroup of the per-frame batch form, which scans only 32 train tiles.)
    uint32_t qraw[QT][8];
#pragma unroll
    for (int qt = 0; qt < QT; qt++) {
        const int q = min(qblock0 + (wave * QT + qt) * 32 + n, nq - 1);
#pragma unroll
        for (int c = 0; c < 8; c++) qraw[qt][c] = Qp[(long long)q * 8 + c];
    }
    // expansion of one train dword per thread and tile: row m = tid / 8, dword wd = tid % 8 -> 32 bytes of -(+-1) (the lookup of ~byte)
    const int m_st = tid >> 3, wd_st = tid & 7;
    auto load_raw = [&](int tile_i) -> uint32_t {
        return Tp[(long long)min(t0 + tile_i * 32 + m_st, t1 - 1) * 8 + wd_st];
    };
    uint32_t raw0 = 0, raw1 = 0, raw2 = 0, raw_next = 0;
    if (ntiles > 0) { raw0 = load_raw(0); raw1 = load_raw(1); raw2 = load_raw(2); raw_next = load_raw(3); }
    {
        const uint32_t v = (uint32_t)tid;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int bq = 0; bq < 4; bq++) {
            lo |= (((v >> bq) & 1u) ? 0x01u : 0xFFu) << (8 * bq);
            hi |= (((v >> (4 + bq)) & 1u) ? 0x01u : 0xFFu) << (8 * bq);
        }
        lut[tid] = make_uint2(lo, hi);
        lut64[tid] = make_uint2((lo & 0x01010101u) << 6 | (lo & 0x80808080u), (hi & 0x01010101u) << 6 | (hi & 0x80808080u));   // 0x01 -> 0x40, 0xFF -> 0xC0
    }
    __syncthreads();
    // B operands: QT x 8 chunks x 16 bytes per lane
    i32x4_t breg[QT][8];
#pragma unroll
    for (int qt = 0; qt < QT; qt++) {
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const uint32_t h16 = (qraw[qt][c] >> (16 * kh)) & 0xFFFFu;
            const uint2 e0 = lut[h16 & 255u], e1 = lut[h16 >> 8];
            breg[qt][c] = (i32x4_t){(int)e0.x, (int)e0.y, (int)e1.x, (int)e1.y};
        }
    }
    K1.a0 = K1.a1 = K1.a2 = K1.a3 = KEY_NONE;
    K2.a0 = K2.a1 = K2.a2 = K2.a3 = KEY_NONE;
    if (ntiles <= 0) return;
    auto expand = [&](uint32_t raw, int buf) {
        const uint32_t x = ~raw;
        const uint2 a = lut64[x & 255u], bb = lut64[(x >> 8) & 255u], c = lut64[(x >> 16) & 255u], d = lut64[x >> 24];
        uint4* dst = reinterpret_cast<uint4*>(tiles + buf * MF_TILE_BYTES + m_st * MF_PITCH + 32 * wd_st);
        dst[0] = make_uint4(a.x, a.y, bb.x, bb.y);
        dst[1] = make_uint4(c.x, c.y, d.x, d.y);
    };
    // The MFMA itself builds tile-local keys: with the train bytes scaled to +-64 the product is 64 * (2 * hamming - 256), and the
    // accumulator of register r starts at 16384 + row(r, lane), so it ends as hamming * 128 + row — a 16-bit key whose order within
    // the tile is the reference's (distance, then first index).  The VALU is left with med3 + min per pair; the tile's two smallest
    // keys are widened to (hamming << 22) | index and merged into the running pair once per tile.
    i32x16_t cinit;
#pragma unroll
    for (int r = 0; r < 16; r++) cinit[r] = 16384 + 8 * (r / 4) + (r % 4) + 4 * kh;
    auto load_a = [&](const uint8_t* p) -> i32x4_t {
        const uint4 av = *reinterpret_cast<const uint4*>(p);
        return (i32x4_t){(int)av.x, (int)av.y, (int)av.z, (int)av.w};
    };
    // tile-local pair (k1 <= k2, 16-bit keys) of the tile at tbase -> global keys, merged into the running pair
    auto merge_tile = [&](uint32_t& G1, uint32_t& G2, uint32_t k1, uint32_t k2, uint32_t tbase) {
        const uint32_t g1 = ((k1 >> 7) << KEY_SHIFT) + (k1 & 127u) + tbase;
        const uint32_t g2 = k2 == KEY_NONE ? KEY_NONE : ((k2 >> 7) << KEY_SHIFT) + (k2 & 127u) + tbase;
        const uint32_t hi = max(G1, g1);
        G1 = min(G1, g1);
        G2 = min(hi, min(G2, g2));
    };
    // Chain-major software pipeline (round 3).  A "chain" is the 8 dependent MFMAs (K = 256) of one train tile against ONE of the
    // wave's query tiles; chains alternate between two accumulator sets.  While the matrix pipe works on chain n the VALU runs the
    // top-2 of chain n - 1 (two accumulator registers behind every MFMA, pinned with sched_barrier) — so only 2 x 16 accumulator
    // registers are live whatever QT is, and a wave can keep FOUR query tiles (128 VGPRs of B operands) at two waves per SIMD:
    // every 16-byte A operand read from LDS feeds four MFMAs instead of two, and the train-tile expansion and the barrier are paid
    // once per 32 MFMAs.  (Round 2 ran chunk-major with 2 x QT accumulator sets: QT = 2 was all that fitted.)
    static_assert(QT == 2 || QT == 4, "chains alternate accumulator sets by the parity of the query tile");
    expand(raw0, 0);
    expand(raw1, 1);
    expand(raw2, 2);
    __syncthreads();
    i32x16_t accP, accQ;                                       // chain qt writes accP (qt even) or accQ (qt odd)
    i32x4_t areg[8];
    const uint8_t* lane_tile = tiles + n * MF_PITCH + 16 * kh;
#pragma unroll
    for (int c = 0; c < 8; c++) areg[c] = load_a(lane_tile + 32 * c);
    // one chain: MFMAs of (tile, qt) into `acc`; in their shadow the top-2 of the previous chain `prv` (HAVE: there is one; MASKED:
    // it belongs to the padded last tile); REFILL: the A registers are reloaded for the next tile as their last user issues
    auto chain = [&](auto qc, i32x16_t& acc, const i32x16_t& prv, auto have_c, auto masked_c, uint32_t& pk1, uint32_t& pk2, int prv_tbase,
                     bool refill, const uint8_t* next_tile) {
        constexpr int qt = decltype(qc)::value;
        constexpr bool HAVE = decltype(have_c)::value, MASKED = decltype(masked_c)::value;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(areg[c], breg[qt][c], c == 0 ? cinit : acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (HAVE) {
                if (MASKED) {
                    if (c == 0) { pk1 = KEY_NONE; pk2 = KEY_NONE; }
#pragma unroll
                    for (int r = 2 * c; r < 2 * c + 2; r++)
                        if (prv_tbase + 8 * (r / 4) + (r % 4) + 4 * kh < t1) top2_update(pk1, pk2, (uint32_t)prv[r]);
                } else if (c == 0) {
                    pk1 = min((uint32_t)prv[0], (uint32_t)prv[1]);
                    pk2 = max((uint32_t)prv[0], (uint32_t)prv[1]);
                } else {
                    top2_update(pk1, pk2, (uint32_t)prv[2 * c]);
                    top2_update(pk1, pk2, (uint32_t)prv[2 * c + 1]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (refill) areg[c] = load_a(next_tile + 32 * c);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto finish = [&](auto qc, uint32_t pk1, uint32_t pk2, int tbase) {      // the finished chain's tile-local pair into the query tile's running pair
        constexpr int qt = decltype(qc)::value;
        if (pk1 != KEY_NONE) merge_tile(K1.at<qt>(), K2.at<qt>(), pk1, pk2, (uint32_t)tbase);
    };
    using T = std::true_type;
    using F = std::false_type;
    uint32_t pk1 = KEY_NONE, pk2 = KEY_NONE;
    // one tile: its QT chains; the first one finishes the last chain of the tile before (if any)
    auto tile_pass = [&](int it, auto first_c, auto last_c) {
        constexpr bool FIRST = decltype(first_c)::value, LAST = decltype(last_c)::value;      // no tile before / the padded last tile
        const int tbase = t0 + it * 32;
        const uint8_t* next_tile = lane_tile + ((it + 1) & 3) * MF_TILE_BYTES;
        static_for<QT>([&](auto qc) {
            constexpr int qt = decltype(qc)::value;
            i32x16_t& acc = (qt & 1) ? accQ : accP;
            const i32x16_t& prv = (qt & 1) ? accP : accQ;
            const bool refill = !LAST && qt == QT - 1;
            if constexpr (qt == 0) {
                if constexpr (FIRST) chain(qc, acc, prv, F{}, F{}, pk1, pk2, 0, refill, next_tile);
                else {
                    chain(qc, acc, prv, T{}, F{}, pk1, pk2, tbase - 32, refill, next_tile);
                    finish(std::integral_constant<int, QT - 1>{}, pk1, pk2, tbase - 32);
                }
            } else {
                if constexpr (LAST) chain(qc, acc, prv, T{}, T{}, pk1, pk2, tbase, refill, next_tile);
                else chain(qc, acc, prv, T{}, F{}, pk1, pk2, tbase, refill, next_tile);
                finish(std::integral_constant<int, qt - 1>{}, pk1, pk2, tbase);
            }
        });
    };
    auto advance = [&](int it) {                               // tile it + 3 into the ring, tile it + 4 requested
        expand(raw_next, (it + 3) & 3);
        raw_next = load_raw(it + 4);
        __syncthreads();
    };
    if (ntiles == 1) tile_pass(0, T{}, T{});
    else {
        tile_pass(0, T{}, F{});
        advance(0);
        int it = 1;
        for (; it + 1 < ntiles; ++it) { tile_pass(it, F{}, F{}); advance(it); }
        tile_pass(it, F{}, T{});
    }
    {   // the last chain of the last tile: nothing left to overlap it with
        const int tbase = t0 + (ntiles - 1) * 32;
        const i32x16_t& prv = ((QT - 1) & 1) ? accQ : accP;
        pk1 = KEY_NONE; pk2 = KEY_NONE;
#pragma unroll
        for (int r = 0; r < 16; r++)
            if (tbase + 8 * (r / 4) + (r % 4) + 4 * kh < t1) top2_update(pk1, pk2, (uint32_t)prv[r]);
        finish(std::integral_constant<int, QT - 1>{}, pk1, pk2, tbase);
    }
    // lanes l and l + 32 hold the two row halves of the same query
    static_for<QT>([&](auto qc) {
        constexpr int qt = decltype(qc)::value;
        uint32_t& k1 = K1.at<qt>();
        uint32_t& k2 = K2.at<qt>();
        const uint32_t o1 = (uint32_t)__shfl_xor((int)k1, 32, 64), o2 = (uint32_t)__shfl_xor((int)k2, 32, 64);
        const uint32_t lo = min(k1, o1), hi = max(k1, o1);
        k2 = min(hi, min(k2, o2));
        k1 = lo;
    });
}

// Many small problems (frame-to-frame matching): blockIdx.y = problem, sizes read on the device.
template <int QT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_match_batch_mfma(const uint32_t* __restrict__ Q, const int32_t* __restrict__ nqs, const uint32_t* __restrict__ T,
                                                          const int32_t* __restrict__ nts, int cap, int32_t* __restrict__ idx, int32_t* __restrict__ best,
                                                          int32_t* __restrict__ second) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int prob = blockIdx.y;
    const int nq = min(nqs[prob], cap), nt = min(nts[prob], cap);
    const int qblock0 = blockIdx.x * (128 * QT);
    if (qblock0 >= nq) return;
    Top2State K1, K2;
    mfma_scan<QT>(Q + (long long)prob * cap * 8, nq, qblock0, T + (long long)prob * cap * 8, 0, nt, smem, K1, K2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 32) {
        static_for<QT>([&](auto qc) {
            constexpr int qt = decltype(qc)::value;
            const int q = qblock0 + (wave * QT + qt) * 32 + lane;
            if (q < nq) {
                const long long o = (long long)prob * cap + q;
                write_result(K1.at<qt>(), K2.at<qt>(), idx + o, best + o, second + o);
            }
        });
    }
}

// Large single problem: grid = (query blocks, train splits); partial (k1, k2) per (split, query) for k_match_merge.
template <int QT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_match_split_mfma(const uint32_t* __restrict__ Q, int nq, const uint32_t* __restrict__ T, int nt, int chunk,
                                                          uint32_t* __restrict__ pk1, uint32_t* __restrict__ pk2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int qblock0 = blockIdx.x * (128 * QT);
    const int t0 = blockIdx.y * chunk, t1 = min(nt, t0 + chunk);
    Top2State K1, K2;
    mfma_scan<QT>(Q, nq, qblock0, T, t0, t1, smem, K1, K2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 32) {
        static_for<QT>([&](auto qc) {
            constexpr int qt = decltype(qc)::value;
            const int q = qblock0 + (wave * QT + qt) * 32 + lane;
            if (q < nq) {
                pk1[(long long)blockIdx.y * nq + q] = K1.at<qt>();
                pk2[(long long)blockIdx.y * nq + q] = K2.at<qt>();
            }
        });
    }
}

// ------------------------------------------------------------------------------------ Hamming by FP4 MFMA (round 5, gfx950 only)
// The same scan on v_mfma_scale_f32_32x32x64_f8f6f4 with both operands in FP4 (E2M1): CDNA4's block-scaled matrix instruction runs
// FP4 at twice the int8 rate (guide: 9.1 against 4.4 POP/s measured) and a bit costs a nibble instead of a byte — half the operand
// registers (16 VGPRs per query tile), half the LDS bytes per train tile, half the expansion work.  Exact: bit b -> the nibble 0x2 | b << 3
// (+1.0 / -1.0), trains looked up negated and given the block scale 2^(S-1) (E8M0 byte 126 + S; the queries' scale is 1), so the K = 256
// dot product is 2^(S-1) (2 hamming - 256); with the accumulator of row i of the chunk started at 2^(S+7) + i the result is
// hamming * 2^S + i: an integer below 2^24 (S <= 15), exact in f32, and ordered like its bit pattern.  S = idx_bits is chosen by the
// host as the smallest that holds the chunk's indices (10 for a 1000-feature frame, 13 for the 100k x 100k chunks), i.e. the sums stay
// well inside the 24-bit significand.
//   Because the key carries the CHUNK-relative index, not a tile-local one, the running pair of a query tile lives across train tiles
// in the key's own form (float bit patterns compared as u32): no per-tile widening and merging (14 VALU instructions per chain in the
// int8 form), the accumulator's start is re-made per tile instead (16 v_add_f32 for QT chains).  Rows past the chunk's end start
// 2^(S+9) higher — they lose against every real key and decode to "none".  Per chain: 4 MFMAs of ~35 cycles against 32 VALU
// instructions (v_med3 + v_min per pair) — the two pipes are level now, where the int8 form left the VALU half idle.
// Operand layout: the usual 32 x 32 one (lane l: row / column l % 32, K half l / 32; D as in the int8 form — the guide: D is
// dtype-independent); WHICH 32 of the 64 K values a lane's 16 bytes are does not matter, both operands use the same map.
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
constexpr int M4_PITCH = 144;                      // bytes per expanded train row in LDS (128 + 16: the 16-byte reads of 16 consecutive lanes cover all 64 banks)
constexpr int M4_TILE_BYTES = 32 * M4_PITCH;
constexpr int M4_LDS_BYTES = 1024 + 4 * M4_TILE_BYTES;     // byte -> 8 nibbles table + ring of four train tiles
constexpr int M4_MAX_IDX_BITS = 15;                // hamming * 2^S + index < 2^24
#ifndef ORBX_M4_QT
#define ORBX_M4_QT 4
#endif
constexpr int M4_QT = ORBX_M4_QT;
#ifndef ORBX_M4_WAVES
#define ORBX_M4_WAVES 3                           // waves per SIMD the FP4 kernels are compiled for (= workgroups per CU): 168 VGPRs; 2 (194 VGPRs): +2...3 % time
#endif
#ifndef ORBX_M4_TWO_A_SETS
#define ORBX_M4_TWO_A_SETS 1
#endif

// (by value: __builtin_bit_cast applied to a vector ELEMENT reads element 0 whatever the index — clang takes the vector's address)
__device__ __forceinline__ uint32_t key_of(float f) { return __float_as_uint(f); }

__device__ __forceinline__ f32x16_t mfma_fp4(const i32x4_t& a, const i32x4_t& b, const f32x16_t& c, int scale_a, int scale_b) {
    const i32x8_t a8 = {a.x, a.y, a.z, a.w, 0, 0, 0, 0}, b8 = {b.x, b.y, b.z, b.w, 0, 0, 0, 0};      // FP4 reads the first four registers only
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, scale_a, 0, scale_b);
}

template <int QT>
__device__ __forceinline__ void mfma4_scan(const uint32_t* __restrict__ Qp, int nq, int qblock0, const uint32_t* __restrict__ Tp, int t0, int t1,
                                           int idx_bits, uint8_t* smem, Top2State& K1, Top2State& K2) {
    static_assert(QT == 2 || QT == 4, "chains alternate accumulator sets by the parity of the query tile");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, kh = lane >> 5;
    uint32_t* lut = reinterpret_cast<uint32_t*>(smem);          // lut[v]: nibble j = bit j of v as +1.0 (0x2) / -1.0 (0xA)
    uint8_t* tiles = smem + 1024;
    const int ntiles = (t1 - t0 + 31) >> 5;
    // every global load of the prologue first, from clamped indices (see mfma_scan): this lane's dword 2c + kh of each chunk of its QT queries
    // and the first four train tiles
    uint32_t qraw[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; qt++) {
        const int q = min(qblock0 + (wave * QT + qt) * 32 + n, nq - 1);
#pragma unroll
        for (int c = 0; c < 4; c++) qraw[qt][c] = Qp[(long long)q * 8 + 2 * c + kh];
    }
    // expansion of one train dword per thread and tile: row m = tid / 8, dword wd = tid % 8 -> 16 bytes of nibbles of the NEGATED bits
    const int m_st = tid >> 3, wd_st = tid & 7;
    auto load_raw = [&](int tile_i) -> uint32_t {               // (rows past t1: any descriptor — they start 2^(S+9) higher and never win)
        return Tp[(long long)min(t0 + tile_i * 32 + m_st, t1 - 1) * 8 + wd_st];
    };
    uint32_t raw0 = 0, raw1 = 0, raw2 = 0, raw_next = 0;
    if (ntiles > 0) { raw0 = load_raw(0); raw1 = load_raw(1); raw2 = load_raw(2); raw_next = load_raw(3); }
    {
        const uint32_t v = (uint32_t)tid;
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) w |= (0x2u | (((v >> j) & 1u) << 3)) << (4 * j);
        lut[tid] = w;
    }
    __syncthreads();
    auto nibbles = [&](uint32_t w) -> i32x4_t {
        return (i32x4_t){(int)lut[w & 255u], (int)lut[(w >> 8) & 255u], (int)lut[(w >> 16) & 255u], (int)lut[w >> 24]};
    };
    // B operands: QT x 4 chunks (K = 64: descriptor dwords 2c and 2c + 1, this lane's half is dword 2c + kh) x 16 bytes per lane
    i32x4_t breg[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; qt++) {
#pragma unroll
        for (int c = 0; c < 4; c++) breg[qt][c] = nibbles(qraw[qt][c]);
    }
    K1.a0 = K1.a1 = K1.a2 = K1.a3 = KEY_NONE;
    K2.a0 = K2.a1 = K2.a2 = K2.a3 = KEY_NONE;
    if (ntiles <= 0) return;
    const int scale_a = (int)((uint32_t)(126 + idx_bits) * 0x01010101u), scale_b = 0x7F7F7F7F;      // E8M0: trains 2^(S-1), queries 1 (every byte: whichever the lane's block reads)
    auto expand = [&](uint32_t raw, int buf) {
        const i32x4_t e = nibbles(~raw);
        *reinterpret_cast<uint4*>(tiles + buf * M4_TILE_BYTES + m_st * M4_PITCH + 16 * wd_st) = make_uint4((uint32_t)e.x, (uint32_t)e.y, (uint32_t)e.z, (uint32_t)e.w);
    };
    auto load_a = [&](const uint8_t* p) -> i32x4_t {
        const uint4 av = *reinterpret_cast<const uint4*>(p);
        return (i32x4_t){(int)av.x, (int)av.y, (int)av.z, (int)av.w};
    };
    // accumulator start of the tile at chunk-relative row base `rel`: 2^(S+7) + rel + row(r, lane); rows at or past `lim` (the
    // padded end of the chunk's last tile) 2^(S+9) higher.  (Sixteen adds of non-zero constants to start0 - 1: with row 0's "+ 0"
    // folded away the compiler pairs the rest into v_pk_add_f32 at odd register offsets and moves every result into the tuple.)
    const float start0 = (float)((1 << (idx_bits + 7)) + 4 * kh - 1), penalty = (float)(1 << (idx_bits + 9));
    auto make_cin = [&](int rel, auto last_c, int lim) -> f32x16_t {
        constexpr bool LAST = decltype(last_c)::value;
        const float s = start0 + (float)rel;
        f32x16_t c;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            c[r] = s + (float)(8 * (r / 4) + (r % 4) + 1);
            if (LAST && rel + 8 * (r / 4) + (r % 4) + 4 * kh >= lim) c[r] += penalty;
        }
        return c;
    };
    expand(raw0, 0);
    expand(raw1, 1);
    expand(raw2, 2);
    __syncthreads();
    f32x16_t accP, accQ, cin;                                   // chain qt writes accP (qt even) or accQ (qt odd)
#if ORBX_M4_TWO_A_SETS
    i32x4_t aregA[4], aregB[4];                                 // A operands of the even / odd tiles (two sets: a single one is copied register by register at the loop head)
#else
    i32x4_t aregA[4];
    i32x4_t (&aregB)[4] = aregA;
#endif
    const uint8_t* lane_tile = tiles + n * M4_PITCH + 16 * kh;
#pragma unroll
    for (int c = 0; c < 4; c++) aregA[c] = load_a(lane_tile + 32 * c);
    // one chain: the 4 MFMAs of (tile, qt) into `acc`; in their shadow the previous chain's 16 keys `prv` enter the running pair
    // (k1, k2) of ITS query tile (HAVE: there is one); REFILL: the other A set is loaded for the next tile under the tile's last chain
    auto chain = [&](auto qc, const i32x4_t (&areg)[4], i32x4_t (&afill)[4], f32x16_t& acc, const f32x16_t& prv, auto have_c, uint32_t& k1, uint32_t& k2,
                     bool refill, const uint8_t* next_tile) {
        constexpr int qt = decltype(qc)::value;
        constexpr bool HAVE = decltype(have_c)::value;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            acc = mfma_fp4(areg[c], breg[qt][c], c == 0 ? cin : acc, scale_a, scale_b);
            __builtin_amdgcn_sched_barrier(0);
            if (HAVE) {
#pragma unroll
                for (int r = 4 * c; r < 4 * c + 4; r++) top2_update(k1, k2, key_of(prv[r]));
            }
            __builtin_amdgcn_sched_barrier(0);
            if (refill) afill[c] = load_a(next_tile + 32 * c);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    using T = std::true_type;
    using F = std::false_type;
    // one tile: its QT chains; the first one takes in the keys of the last chain of the tile before (if any)
    auto tile_pass = [&](int it, auto first_c, auto last_c, const i32x4_t (&areg)[4], i32x4_t (&afill)[4]) {
        constexpr bool FIRST = decltype(first_c)::value, LAST = decltype(last_c)::value;      // no tile before / the chunk's last tile
        const uint8_t* next_tile = lane_tile + ((it + 1) & 3) * M4_TILE_BYTES;
        cin = make_cin(it * 32, last_c, t1 - t0);
        static_for<QT>([&](auto qc) {
            constexpr int qt = decltype(qc)::value;
            constexpr int pq = (qt + QT - 1) % QT;               // the chain before this one belongs to query tile pq
            f32x16_t& acc = (qt & 1) ? accQ : accP;
            const f32x16_t& prv = (qt & 1) ? accP : accQ;
            const bool refill = !LAST && qt == QT - 1;
            if constexpr (qt == 0 && FIRST) chain(qc, areg, afill, acc, prv, F{}, K1.at<pq>(), K2.at<pq>(), refill, next_tile);
            else chain(qc, areg, afill, acc, prv, T{}, K1.at<pq>(), K2.at<pq>(), refill, next_tile);
        });
    };
    auto advance = [&](int it) {                               // tile it + 3 into the ring, tile it + 4 requested
        expand(raw_next, (it + 3) & 3);
        raw_next = load_raw(it + 4);
        __syncthreads();
    };
    if (ntiles == 1) tile_pass(0, T{}, T{}, aregA, aregB);
    else {
        tile_pass(0, T{}, F{}, aregA, aregB);
        advance(0);
        int it = 1;                                            // odd tiles read set B and fill A, even ones the other way round
        for (; it + 2 < ntiles; it += 2) {
            tile_pass(it, F{}, F{}, aregB, aregA);
            advance(it);
            tile_pass(it + 1, F{}, F{}, aregA, aregB);
            advance(it + 1);
        }
        if (it + 1 < ntiles) {
            tile_pass(it, F{}, F{}, aregB, aregA);
            advance(it);
            tile_pass(it + 1, F{}, T{}, aregA, aregB);
        } else tile_pass(it, F{}, T{}, aregB, aregA);
    }
    {   // the last chain of the last tile: nothing left to overlap it with
        const f32x16_t& prv = ((QT - 1) & 1) ? accQ : accP;
#pragma unroll
        for (int r = 0; r < 16; r++) top2_update(K1.at<QT - 1>(), K2.at<QT - 1>(), key_of(prv[r]));
    }
    // float keys -> (hamming << 22) | train index; lanes l and l + 32 hold the two row halves of the same query
    const uint32_t none_from = __builtin_bit_cast(uint32_t, penalty), idx_mask = (1u << idx_bits) - 1u;
    auto widen = [&](uint32_t k) -> uint32_t {
        const uint32_t u = (uint32_t)__builtin_bit_cast(float, k);
        return k >= none_from ? KEY_NONE : ((u >> idx_bits) << KEY_SHIFT) + (u & idx_mask) + (uint32_t)t0;
    };
    static_for<QT>([&](auto qc) {
        constexpr int qt = decltype(qc)::value;
        uint32_t& k1 = K1.at<qt>();
        uint32_t& k2 = K2.at<qt>();
        k1 = widen(k1);
        k2 = widen(k2);
        const uint32_t o1 = (uint32_t)__shfl_xor((int)k1, 32, 64), o2 = (uint32_t)__shfl_xor((int)k2, 32, 64);
        const uint32_t lo = min(k1, o1), hi = max(k1, o1);
        k2 = min(hi, min(k2, o2));
        k1 = lo;
    });
}

template <int QT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ORBX_M4_WAVES, ORBX_M4_WAVES))) void k_match_batch_mfma4(const uint32_t* __restrict__ Q, const int32_t* __restrict__ nqs, const uint32_t* __restrict__ T,
                                                           const int32_t* __restrict__ nts, int cap, int idx_bits, int32_t* __restrict__ idx, int32_t* __restrict__ best,
                                                           int32_t* __restrict__ second) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int prob = blockIdx.y;
    const int nq = min(nqs[prob], cap), nt = min(nts[prob], cap);
    const int qblock0 = blockIdx.x * (128 * QT);
    if (qblock0 >= nq) return;
    Top2State K1, K2;
    mfma4_scan<QT>(Q + (long long)prob * cap * 8, nq, qblock0, T + (long long)prob * cap * 8, 0, nt, idx_bits, smem, K1, K2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 32) {
        static_for<QT>([&](auto qc) {
            constexpr int qt = decltype(qc)::value;
            const int q = qblock0 + (wave * QT + qt) * 32 + lane;
            if (q < nq) {
                const long long o = (long long)prob * cap + q;
                write_result(K1.at<qt>(), K2.at<qt>(), idx + o, best + o, second + o);
            }
        });
    }
}

template <int QT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ORBX_M4_WAVES, ORBX_M4_WAVES))) void k_match_split_mfma4(const uint32_t* __restrict__ Q, int nq, const uint32_t* __restrict__ T, int nt, int chunk, int idx_bits,
                                                           uint32_t* __restrict__ pk1, uint32_t* __restrict__ pk2) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int qblock0 = blockIdx.x * (128 * QT);
    const int t0 = blockIdx.y * chunk, t1 = min(nt, t0 + chunk);
    Top2State K1, K2;
    mfma4_scan<QT>(Q, nq, qblock0, T, t0, t1, idx_bits, smem, K1, K2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 32) {
        static_for<QT>([&](auto qc) {
            constexpr int qt = decltype(qc)::value;
            const int q = qblock0 + (wave * QT + qt) * 32 + lane;
            if (q < nq) {
                pk1[(long long)blockIdx.y * nq + q] = K1.at<qt>();
                pk2[(long long)blockIdx.y * nq + q] = K2.at<qt>();
            }
        });
    }
}

// Candidate-set form (what every ORBmatcher search really scans: the grid window of GetFeaturesInArea or the features of
// one vocabulary node): query q scans the train descriptors cand[seg_off[q] .. seg_off[q+1]) IN LIST ORDER.  One wave per
// query, one candidate per lane and step; key = (distance << 22) | position-in-list keeps the reference's "first candidate
// attaining the best distance" rule; a butterfly of min / med3 steps reduces the 64 lanes' (k1,k2) pairs.
__device__ __forceinline__ void top2_merge(uint32_t& k1, uint32_t& k2, uint32_t o1, uint32_t o2) {
    // two sorted pairs -> the two smallest of the four keys
    const uint32_t lo = min(k1, o1), hi = max(k1, o1);
    k2 = min(hi, min(k2, o2));
    k1 = lo;
}

__global__ __launch_bounds__(256) void k_match_segments(const uint32_t* __restrict__ Q, int nq, const uint32_t* __restrict__ T, int nt,
                                                        const int32_t* __restrict__ seg_off, const int32_t* __restrict__ cand,
                                                        int32_t* __restrict__ idx, int32_t* __restrict__ best, int32_t* __restrict__ second) {
    const int q = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (q >= nq) return;
    const int lane = threadIdx.x & 63;
    const int s0 = seg_off[q], s1 = seg_off[q + 1];
    uint32_t qw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) qw[i] = Q[(long long)q * 8 + i];   // wave-uniform: scalar loads
    uint32_t k1 = KEY_NONE, k2 = KEY_NONE;
    for (int base = s0; base < s1; base += 64) {
        const int p = base + lane;
        if (p < s1) {
            const int t = cand[p];
            uint32_t key = KEY_NONE - 1;   // invalid candidate index: never wins, never reported
            if ((unsigned)t < (unsigned)nt) {
                const dwords4* tp = reinterpret_cast<const dwords4*>(T + (long long)t * 8);
                const dwords4 a = tp[0], c = tp[1];
                uint32_t d = 0;
                d = bcnt_acc(qw[0] ^ a.x, d); d = bcnt_acc(qw[1] ^ a.y, d); d = bcnt_acc(qw[2] ^ a.z, d); d = bcnt_acc(qw[3] ^ a.w, d);
                d = bcnt_acc(qw[4] ^ c.x, d); d = bcnt_acc(qw[5] ^ c.y, d); d = bcnt_acc(qw[6] ^ c.z, d); d = bcnt_acc(qw[7] ^ c.w, d);
                key = (d << KEY_SHIFT) | (uint32_t)(p - s0);
                top2_update(k1, k2, key);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o1 = (uint32_t)__shfl_xor((int)k1, off, 64), o2 = (uint32_t)__shfl_xor((int)k2, off, 64);
        top2_merge(k1, k2, o1, o2);
    }
    if (lane == 0) {
        int32_t bi, bd, sd;
        write_result(k1, k2, &bi, &bd, &sd);
        idx[q] = bi < 0 ? -1 : cand[s0 + bi];   // list position -> train index
        best[q] = bd;
        second[q] = sd;
    }
}

// MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:216-244), one wave per map point.  Lane i owns row i of
// the N x N distance matrix: it never stores the row — the median (element (int)(0.5*(N-1)) of the sorted row) is found by
// bisection on the value range 0..256, each step counting the row's distances <= mid by recomputing them (8 xor + 8 popcount
// per pair; the other descriptors arrive by wave-uniform scalar loads).  The winner is the smallest (median << 16 | i).
__global__ __launch_bounds__(MATCH_BLOCK) void k_distinctive(const uint32_t* __restrict__ desc, const int32_t* __restrict__ seg_off, int npoints,
                                                            int32_t* __restrict__ best_idx, int32_t* __restrict__ best_median) {
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (MATCH_BLOCK / 64) + (threadIdx.x >> 6)));
    if (p >= npoints) return;
    const int s0 = seg_off[p], N = seg_off[p + 1] - s0;
    if (N <= 0) { if (lane == 0) { best_idx[p] = -1; best_median[p] = INT_MAX; } return; }
    const int m = (int)(0.5 * (double)(N - 1));              // `vDists[0.5*(N-1)]`
    const uint32_t* D = desc + (size_t)s0 * 8;
    uint32_t bestkey = 0xFFFFFFFFu;
    for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        uint32_t q[8];
#pragma unroll
        for (int w = 0; w < 8; w++) q[w] = i < N ? D[(size_t)i * 8 + w] : 0u;
        int lo = 0, hi = 256;                                // smallest v with #{j : d(i,j) <= v} >= m + 1
        while (__any(lo < hi)) {
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
            for (int j = 0; j < N; j++) {
                const uint32_t* t = D + (size_t)j * 8;       // wave-uniform address: scalar loads
                uint32_t d = 0;
#pragma unroll
                for (int w = 0; w < 8; w++) d = bcnt_acc(q[w] ^ t[w], d);
                cnt += (int)d <= mid;
            }
            if (lo < hi) { if (cnt >= m + 1) hi = mid; else lo = mid + 1; }
        }
        if (i < N) bestkey = min(bestkey, ((uint32_t)lo << 16) | (uint32_t)i);
    }
    for (int s = 32; s > 0; s >>= 1) bestkey = min(bestkey, (uint32_t)__shfl_xor((int)bestkey, s, 64));
    if (lane == 0) { best_idx[p] = (int32_t)(bestkey & 0xFFFFu); best_median[p] = (int32_t)(bestkey >> 16); }
}

}  // namespace orbx

using namespace orbx;

extern "C" {

int orbm_hamming256(const uint8_t* a, const uint8_t* b) {
    uint32_t wa[8], wb[8];
    memcpy(wa, a, 32);
    memcpy(wb, b, 32);
    return hamming256_words(wa, wb);
}

int orbm_count_accepted(const int32_t* best, const int32_t* second, int nq, int th, float ratio) {
    int n = 0;
    for (int q = 0; q < nq; q++)
        if (best[q] <= th && (float)best[q] < ratio * (float)second[q]) n++;
    return n;
}

// Which kernels the dense top-2 calls use: 0 = xor + popcount (the form north_star names; the A/B baseline), 1 = int8 MFMA, 2 = FP4 MFMA
// (round 5).  Process default: ORBX_MATCH_MFMA = 0 / 8 / 4 in the environment, otherwise ORBX_MATCH_DEFAULT_PATH;
// orbm_debug_set_match_path() overrides it per process at run time (the parity tests run all forms in one process).
#ifndef ORBX_MATCH_DEFAULT_PATH
#define ORBX_MATCH_DEFAULT_PATH 2
#endif
static std::atomic<int> g_match_path{-1};        // -1: environment default
static int match_path() {
    static const int env_default = [] {
        // the WHOLE string: "0" = xor + popcount, "8" / "int8" / "1" (what rounds 2-4 called "on") = int8 MFMA, "4" / "fp4" = FP4 MFMA; anything else
        // is said out loud once and ignored (a first-character parse sent "1", "80", "int8" to the FP4 default without a word)
        const char* e = getenv("ORBX_MATCH_MFMA");
        if (!e || !e[0]) return ORBX_MATCH_DEFAULT_PATH;
        const std::string v(e);
        if (v == "0" || v == "popcount") return 0;
        if (v == "8" || v == "int8" || v == "1") return 1;
        if (v == "4" || v == "fp4") return 2;
        fprintf(stderr, "liborbx: ORBX_MATCH_MFMA=%s not understood (0 | 8 | 4): keeping the default path %d\n", e, ORBX_MATCH_DEFAULT_PATH);
        return ORBX_MATCH_DEFAULT_PATH;
    }();
    const int f = g_match_path.load(std::memory_order_relaxed);
    return f < 0 ? env_default : f;
}

int orbm_debug_set_match_path(int path) {
    if (path < -1 || path > 2) return ORBX_ERR_ARG;
    g_match_path.store(path, std::memory_order_relaxed);
    return ORBX_OK;
}

int orbm_debug_get_match_path(void) { return match_path(); }

// index bits of the FP4 form's keys for chunks of `chunk` train descriptors (whole tiles): the smallest S >= 5 with chunk <= 2^S; 0 = too long
static int m4_idx_bits(int chunk) {
    const int padded = (chunk + 31) / 32 * 32;
    for (int s = 5; s <= orbx::M4_MAX_IDX_BITS; s++) if (padded <= (1 << s)) return s;
    return 0;
}

// compute units of the current device (cached per host thread and device)
static int device_cus() {
    static thread_local int cached_dev = -1, cus = 256;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return cus;
    if (dev != cached_dev) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
        (void)hipGetLastError();
        cached_dev = dev;
    }
    return cus;
}

// workgroups of the FP4 split kernel a CU holds (registers and LDS decide; asked of the runtime once)
static int m4_wgs_per_cu() {
    static const int n = [] {
        int blocks = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, orbx::k_match_split_mfma4<orbx::M4_QT>, 256, orbx::M4_LDS_BYTES) != hipSuccess || blocks < 1) { (void)hipGetLastError(); blocks = 2; }
        return blocks;
    }();
    return n;
}

// Scratch of the split form (partial top-2 per train split): stream-ordered allocation from a PRIVATE memory pool per device (round 4;
// rounds 2-3 raised the release threshold of the device's DEFAULT pool, a process-wide side effect on a pool the host application may
// share, e.g. with torch's hipMallocAsync backend).  The private pool keeps what it has handed out once (release threshold 256 MiB: with
// 0 every synchronise returns the memory to the driver and the next large match pays the allocation again).  Where the runtime cannot
// create a pool the default pool serves, its threshold raised only if it is lower; where it has no memory pools at all the call falls
// back to hipMalloc + a stream synchronise before the free.
static hipMemPool_t match_pool() {
    constexpr int MAX_DEV = 64;
    static std::mutex mu;
    static hipMemPool_t pools[MAX_DEV] = {};
    static int state[MAX_DEV] = {};                 // 0 unknown, 1 pool usable, -1 no pools
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (state[dev] != 0) return state[dev] > 0 ? pools[dev] : nullptr;
    state[dev] = -1;
    int supported = 0;
    if (hipDeviceGetAttribute(&supported, hipDeviceAttributeMemoryPoolsSupported, dev) != hipSuccess || !supported) { (void)hipGetLastError(); return nullptr; }
    uint64_t keep = 256ull << 20;
    hipMemPoolProps props;
    memset(&props, 0, sizeof(props));
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) == hipSuccess && pool) {
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    } else {
        (void)hipGetLastError();
        if (hipDeviceGetDefaultMemPool(&pool, dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        uint64_t cur = 0;
        if (hipMemPoolGetAttribute(pool, hipMemPoolAttrReleaseThreshold, &cur) != hipSuccess || cur < keep)
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    (void)hipGetLastError();
    pools[dev] = pool;
    state[dev] = 1;
    return pool;
}

int orbm_match_top2_device(const uint8_t* dQ, int nq, const uint8_t* dT, int nt, int32_t* d_best_idx, int32_t* d_best,
                           int32_t* d_second, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (nq < 0 || nt < 0 || nt >= (1 << KEY_SHIFT)) return ORBX_ERR_ARG;
    if (nq == 0) return ORBX_OK;
    if (((uintptr_t)dQ & 3) || ((uintptr_t)dT & 3)) return ORBX_ERR_ARG;
    const int path = match_path();
    const bool mfma = path != 0, fp4 = path == 2;
    constexpr int QPL = 2, QT = MF_QT, QT4 = M4_QT;          // popcount form: 2 queries per lane; MFMA forms: QT query tiles per wave
    const int q_per_block = fp4 ? 128 * QT4 : mfma ? 128 * QT : MATCH_BLOCK * QPL;
    const int qblocks = (nq + q_per_block - 1) / q_per_block;
    // enough workgroups to fill 256 CUs several times over, but chunks of >= 256 train descriptors
    const int target_wgs = mfma ? 2048 : 4096;
    int nsplit = std::max(1, std::min((nt + 255) / 256, (target_wgs + qblocks - 1) / qblocks));
    if (mfma) {
        // The MFMA workgroups run two (FP4 form: m4_wgs_per_cu()) per CU and take as long as their chunk is, so the launch proceeds in
        // rounds of that many x CUs workgroups: a split count that leaves the last round nearly empty wastes it (100k x 100k: 196 query
        // blocks x 11 splits = 4.2 rounds took 1.69 ms, x 13 = 4.98 rounds 1.62 ms, x 8 = 3.06 rounds 1.81 ms).  Cost model: rounds x
        // tiles per chunk, in the neighbourhood of the target; the smallest split count among the best wins (less to merge).
        const int slots = (fp4 ? m4_wgs_per_cu() : 2) * device_cus();
        const int floor_ns = fp4 ? (nt + (1 << M4_MAX_IDX_BITS) - 1) >> M4_MAX_IDX_BITS : 1;      // FP4 keys: at most 2^15 train descriptors per chunk
        const int lo = std::max(std::max(1, floor_ns), nsplit / 2), hi = std::max(lo, std::min((nt + 255) / 256, 2 * nsplit));
        long best_cost = LONG_MAX;
        for (int ns = lo; ns <= hi; ++ns) {
            const long rounds = ((long)qblocks * ns + slots - 1) / slots, tiles = ((nt + ns - 1) / ns + 31) / 32;
            const long cost = rounds * tiles * 64 + ns;              // (+ ns: the merge kernel reads 2 keys per split and query)
            if (cost < best_cost) { best_cost = cost; nsplit = ns; }
        }
    }
    int chunk = nt > 0 ? (nt + nsplit - 1) / nsplit : 1;
    if (mfma) chunk = (chunk + 31) / 32 * 32;                // whole train tiles
    nsplit = nt > 0 ? (nt + chunk - 1) / chunk : 1;
    const int idx_bits = fp4 ? m4_idx_bits(chunk) : 0;
    if (fp4 && idx_bits == 0) return ORBX_ERR_DEVICE;        // (cannot happen: floor_ns bounds the chunk)
    // Partial (k1, k2) per (split, query): stream-ordered allocation, so calls on different streams never share a buffer and the
    // call stays asynchronous (the free is queued behind the merge kernel).
    const size_t need = (size_t)2 * nsplit * nq * sizeof(uint32_t);
    uint32_t* pk1 = nullptr;
    hipMemPool_t pool = match_pool();
    const bool pooled = pool != nullptr;
    if ((pooled ? hipMallocFromPoolAsync(reinterpret_cast<void**>(&pk1), need, pool, stream) : hipMalloc(reinterpret_cast<void**>(&pk1), need)) != hipSuccess) {
        (void)hipGetLastError();
        return ORBX_ERR_DEVICE;
    }
    uint32_t* pk2 = pk1 + (size_t)nsplit * nq;
    if (fp4) hipLaunchKernelGGL(k_match_split_mfma4<QT4>, dim3(qblocks, nsplit), dim3(256), M4_LDS_BYTES, stream, (const uint32_t*)dQ, nq, (const uint32_t*)dT, nt,
                                chunk, idx_bits, pk1, pk2);
    else if (mfma) hipLaunchKernelGGL(k_match_split_mfma<QT>, dim3(qblocks, nsplit), dim3(256), MF_LDS_BYTES, stream, (const uint32_t*)dQ, nq, (const uint32_t*)dT, nt,
                                      chunk, pk1, pk2);
    else hipLaunchKernelGGL(k_match_split<QPL>, dim3(qblocks, nsplit), dim3(MATCH_BLOCK), 0, stream, (const uint32_t*)dQ, nq, (const uint32_t*)dT, nt,
                            chunk, pk1, pk2);
    int rc = hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
    if (rc == ORBX_OK) {
        hipLaunchKernelGGL(k_match_merge, dim3((nq + 255) / 256), dim3(256), 0, stream, pk1, pk2, nq, nsplit, d_best_idx, d_best, d_second);
        if (hipGetLastError() != hipSuccess) rc = ORBX_ERR_DEVICE;
    }
    if (pooled) {
        if (hipFreeAsync(pk1, stream) != hipSuccess) rc = ORBX_ERR_DEVICE;
    } else {
        if (hipStreamSynchronize(stream) != hipSuccess) rc = ORBX_ERR_DEVICE;      // no pools on this runtime: the call is synchronous
        if (hipFree(pk1) != hipSuccess) rc = ORBX_ERR_DEVICE;
    }
    return rc;
}

int orbm_match_top2_batch_device(const uint8_t* dQ, const int32_t* d_nq, const uint8_t* dT, const int32_t* d_nt, int nbatch, int cap,
                                 int32_t* d_best_idx, int32_t* d_best, int32_t* d_second, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (nbatch < 0 || cap < 1 || cap >= (1 << KEY_SHIFT)) return ORBX_ERR_ARG;
    if (nbatch == 0) return ORBX_OK;
    if (((uintptr_t)dQ & 3) || ((uintptr_t)dT & 3)) return ORBX_ERR_ARG;
    const int path = match_path();
    if (path == 2 && m4_idx_bits(cap) != 0) {                    // FP4 keys hold 2^15 train indices; larger capacities take the int8 form
        constexpr int QT = M4_QT;
        hipLaunchKernelGGL(k_match_batch_mfma4<QT>, dim3((cap + 128 * QT - 1) / (128 * QT), nbatch), dim3(256), M4_LDS_BYTES, stream, (const uint32_t*)dQ, d_nq,
                           (const uint32_t*)dT, d_nt, cap, m4_idx_bits(cap), d_best_idx, d_best, d_second);
        return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
    }
    if (path != 0) {
        constexpr int QT = MF_QT;                                // 512 queries per workgroup: two workgroups per ~1000-feature frame
        hipLaunchKernelGGL(k_match_batch_mfma<QT>, dim3((cap + 128 * QT - 1) / (128 * QT), nbatch), dim3(256), MF_LDS_BYTES, stream, (const uint32_t*)dQ, d_nq,
                           (const uint32_t*)dT, d_nt, cap, d_best_idx, d_best, d_second);
        return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
    }
    // popcount form, frame-sized problems (~1000 x 1000): 1 query per lane so that a batch of 256 still fills the chip (4 waves per SIMD)
#ifndef ORBX_MATCH_QPL
#define ORBX_MATCH_QPL 1
#endif
    constexpr int BQPL = ORBX_MATCH_QPL;
    hipLaunchKernelGGL(k_match_batch<BQPL>, dim3((cap + MATCH_BLOCK * BQPL - 1) / (MATCH_BLOCK * BQPL), nbatch), dim3(MATCH_BLOCK), 0, stream, (const uint32_t*)dQ,
                       d_nq, (const uint32_t*)dT, d_nt, cap, d_best_idx, d_best, d_second);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbm_match_top2_segments_device(const uint8_t* dQ, int nq, const uint8_t* dT, int nt, const int32_t* d_seg_off, const int32_t* d_cand,
                                    int32_t* d_best_idx, int32_t* d_best, int32_t* d_second, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (nq < 0 || nt < 0 || !d_seg_off || !d_cand) return ORBX_ERR_ARG;
    if (nq == 0) return ORBX_OK;
    if (((uintptr_t)dQ & 3) || ((uintptr_t)dT & 3)) return ORBX_ERR_ARG;
    hipLaunchKernelGGL(k_match_segments, dim3((nq + 3) / 4), dim3(256), 0, stream, (const uint32_t*)dQ, nq, (const uint32_t*)dT, nt, d_seg_off,
                       d_cand, d_best_idx, d_best, d_second);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbm_match_top2_segments(const uint8_t* Q, int nq, const uint8_t* T, int nt, const int32_t* seg_off, const int32_t* cand, int32_t* best_idx,
                             int32_t* best, int32_t* second, int device) {
    if (nq < 0 || nt < 0 || !seg_off || (nq > 0 && seg_off[nq] > 0 && !cand)) return ORBX_ERR_ARG;
    if (nq == 0) return ORBX_OK;
    const int ncand = seg_off[nq];
    if (ncand < 0) return ORBX_ERR_ARG;
    for (int q = 0; q < nq; q++)      // monotone offsets; the key keeps the position inside ONE segment in 22 bits
        if (seg_off[q] > seg_off[q + 1] || seg_off[q] < 0 || seg_off[q + 1] - seg_off[q] >= (1 << KEY_SHIFT)) return ORBX_ERR_ARG;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto q = s.in(Q, (size_t)nq * 32), t = s.in(T, (size_t)nt * 32);
    const auto sg = s.in(seg_off, (size_t)nq + 1), c = s.in(cand, (size_t)ncand);
    const auto bi = s.out<int32_t>(nq), bd = s.out<int32_t>(nq), sd = s.out<int32_t>(nq);
    HIPTRY(s.alloc());
    const int rc = orbm_match_top2_segments_device(s[q], nq, s[t], nt, s[sg], s[c], s[bi], s[bd], s[sd], nullptr);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(best_idx, bi, nq));
    HIPTRY(s.get(best, bd, nq));
    HIPTRY(s.get(second, sd, nq));
    return ORBX_OK;
}

// ---- dense top-2 over a SUBSET of the train descriptors (the optional t_valid mask) ------------------------------------
// The reference's scans skip train features that are already matched — `if(vpMapPointMatches[realIdxF]) continue;`
// (src/ORBmatcher.cc:205-206 and siblings).  Skipping entries of a sequential scan = scanning the ORDER-PRESERVING compaction of the list,
// so: compact the valid descriptors (one workgroup: ordered ballot ranks, the waves' counts through LDS) with their original indices,
// run the batch form of the dense kernels on the compacted set (its train count is read on the device), map the winners' indices back.
__global__ __launch_bounds__(1024) void k_mask_compact(const uint32_t* __restrict__ T, const uint8_t* __restrict__ valid, int nt, int nq,
                                                       uint32_t* __restrict__ Tc, int32_t* __restrict__ map, int32_t* __restrict__ counts) {
    __shared__ int wsum[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0, par = 0;
    for (int i0 = 0; i0 < nt; i0 += 1024, par ^= 1) {
        const int i = i0 + tid;
        const bool ok = i < nt && valid[i] != 0;
        const unsigned long long mk = __ballot(ok);
        if (lane == 0) wsum[par][wave] = __popcll(mk);
        __syncthreads();                                    // (two sets of words: one barrier per round)
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) { const int c = wsum[par][w]; if (w < wave) off += c; tot += c; }
        if (ok) {
            const int pos = off + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
            map[pos] = i;
#pragma unroll
            for (int k = 0; k < 8; k++) Tc[(size_t)pos * 8 + k] = T[(size_t)i * 8 + k];
        }
        base += tot;
    }
    if (tid == 0) { counts[0] = nq; counts[1] = base; }
}
__global__ __launch_bounds__(256) void k_mask_remap(int32_t* __restrict__ best_idx, const int32_t* __restrict__ map, int nq) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < nq) { const int i = best_idx[q]; if (i >= 0) best_idx[q] = map[i]; }
}

int orbm_match_top2_masked_device(const uint8_t* dQ, int nq, const uint8_t* dT, int nt, const uint8_t* d_t_valid, int32_t* d_best_idx,
                                  int32_t* d_best, int32_t* d_second, void* stream_) {
    if (!d_t_valid) return orbm_match_top2_device(dQ, nq, dT, nt, d_best_idx, d_best, d_second, stream_);
    hipStream_t stream = (hipStream_t)stream_;
    if (nq < 0 || nt < 0 || nt >= (1 << KEY_SHIFT) || nq >= (1 << KEY_SHIFT)) return ORBX_ERR_ARG;
    if (nq == 0) return ORBX_OK;
    if (((uintptr_t)dQ & 3) || ((uintptr_t)dT & 3)) return ORBX_ERR_ARG;
    const int cap = std::max(nq, std::max(nt, 1));
    // scratch: compacted train set (padded by two tiles: the kernels load whole tiles), index map, the two counts
    const size_t tc_bytes = ((size_t)cap + 64) * 32, map_bytes = ((size_t)nt + 1) * sizeof(int32_t);
    const size_t need = tc_bytes + map_bytes + 16;
    uint8_t* scratch = nullptr;
    hipMemPool_t pool = match_pool();
    const bool pooled = pool != nullptr;
    if ((pooled ? hipMallocFromPoolAsync(reinterpret_cast<void**>(&scratch), need, pool, stream) : hipMalloc(reinterpret_cast<void**>(&scratch), need)) != hipSuccess) {
        (void)hipGetLastError();
        return ORBX_ERR_DEVICE;
    }
    uint32_t* Tc = reinterpret_cast<uint32_t*>(scratch);
    int32_t* map = reinterpret_cast<int32_t*>(scratch + tc_bytes);
    int32_t* counts = reinterpret_cast<int32_t*>(scratch + tc_bytes + map_bytes);
    int rc = ORBX_OK;
    hipLaunchKernelGGL(k_mask_compact, dim3(1), dim3(1024), 0, stream, (const uint32_t*)dT, d_t_valid, nt, nq, Tc, map, counts);
    if (hipGetLastError() != hipSuccess) rc = ORBX_ERR_DEVICE;
    // Small problems (a frame against a frame: the case the searches have) stay asynchronous: the batch form reads the compacted count on the
    // device.  Large ones (as ONE batch problem a 100k x 100k masked match got no train splits, one workgroup per 512 queries over the
    // whole list, and — beyond the FP4 batch capacity of 32768 — the int8 kernels) fetch the count (4 bytes, one synchronisation) and take the
    // dense split form on the compacted set: grid by nq, FP4 capacity by the compacted nt, train splits by the cost model.
    if (rc == ORBX_OK && cap > 8192) {
        int32_t hc[2] = {0, 0};
        if (hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) rc = ORBX_ERR_DEVICE;
        if (rc == ORBX_OK) rc = orbm_match_top2_device(dQ, nq, reinterpret_cast<const uint8_t*>(Tc), hc[1], d_best_idx, d_best, d_second, stream);
    } else if (rc == ORBX_OK)
        rc = orbm_match_top2_batch_device(dQ, counts, reinterpret_cast<const uint8_t*>(Tc), counts + 1, 1, cap, d_best_idx, d_best, d_second, stream);
    if (rc == ORBX_OK) {
        hipLaunchKernelGGL(k_mask_remap, dim3((nq + 255) / 256), dim3(256), 0, stream, d_best_idx, map, nq);
        if (hipGetLastError() != hipSuccess) rc = ORBX_ERR_DEVICE;
    }
    if (pooled) {
        if (hipFreeAsync(scratch, stream) != hipSuccess) rc = ORBX_ERR_DEVICE;
    } else {
        if (hipStreamSynchronize(stream) != hipSuccess) rc = ORBX_ERR_DEVICE;
        if (hipFree(scratch) != hipSuccess) rc = ORBX_ERR_DEVICE;
    }
    return rc;
}

int orbm_match_top2_masked(const uint8_t* Q, int nq, const uint8_t* T, int nt, const uint8_t* t_valid, int32_t* best_idx, int32_t* best,
                           int32_t* second, int device) {
    if (!t_valid) return orbm_match_top2(Q, nq, T, nt, best_idx, best, second, device);
    if (nq < 0 || nt < 0) return ORBX_ERR_ARG;
    if (nq == 0) return ORBX_OK;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto q = s.in(Q, (size_t)nq * 32), t = s.in(T, (size_t)nt * 32), v = s.in(t_valid, (size_t)nt);
    const auto bi = s.out<int32_t>(nq), bd = s.out<int32_t>(nq), sd = s.out<int32_t>(nq);
    HIPTRY(s.alloc());
    const int rc = orbm_match_top2_masked_device(s[q], nq, s[t], nt, s[v], s[bi], s[bd], s[sd], nullptr);
    if (rc != ORBX_OK) return rc;
    HIPTRY(hipStreamSynchronize(nullptr));
    HIPTRY(s.get(best_idx, bi, nq));
    HIPTRY(s.get(best, bd, nq));
    HIPTRY(s.get(second, sd, nq));
    return ORBX_OK;
}

int orbm_match_top2(const uint8_t* Q, int nq, const uint8_t* T, int nt, int32_t* best_idx, int32_t* best, int32_t* second, int device) {
    if (nq < 0 || nt < 0) return ORBX_ERR_ARG;
    if (nq == 0) return ORBX_OK;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto q = s.in(Q, (size_t)nq * 32), t = s.in(T, (size_t)nt * 32);
    const auto bi = s.out<int32_t>(nq), bd = s.out<int32_t>(nq), sd = s.out<int32_t>(nq);
    HIPTRY(s.alloc());
    const int rc = orbm_match_top2_device(s[q], nq, s[t], nt, s[bi], s[bd], s[sd], nullptr);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(best_idx, bi, nq));
    HIPTRY(s.get(best, bd, nq));
    HIPTRY(s.get(second, sd, nq));
    return ORBX_OK;
}


int orbm_distinctive_device(const uint8_t* d_desc, const int32_t* d_seg_off, int npoints, int32_t* d_best_idx, int32_t* d_best_median, void* stream) {
    if (npoints < 0) return ORBX_ERR_ARG;
    if (npoints == 0) return ORBX_OK;
    if (!d_desc || !d_seg_off || !d_best_idx || !d_best_median) return ORBX_ERR_ARG;
    const int per_block = orbx::MATCH_BLOCK / 64;
    hipLaunchKernelGGL(orbx::k_distinctive, dim3((npoints + per_block - 1) / per_block), dim3(orbx::MATCH_BLOCK), 0, (hipStream_t)stream,
                       (const uint32_t*)d_desc, d_seg_off, npoints, d_best_idx, d_best_median);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_ERR_DEVICE;
}

int orbm_distinctive(const uint8_t* desc, const int32_t* seg_off, int npoints, int32_t* best_idx, int32_t* best_median, int device) {
    if (npoints < 0 || (npoints > 0 && (!seg_off || !best_idx || !best_median))) return ORBX_ERR_ARG;
    if (npoints == 0) return ORBX_OK;
    const int total = seg_off[npoints];
    if (total < 0 || total >= 65536 * 64 || (total > 0 && !desc)) return ORBX_ERR_ARG;
    for (int p = 0; p < npoints; p++) if (seg_off[p + 1] < seg_off[p] || seg_off[p + 1] - seg_off[p] > 65535) return ORBX_ERR_ARG;
    HIPTRY(hipSetDevice(device));
    Staging s;
    const auto d = s.in(desc, (size_t)total * 32);
    const auto sg = s.in(seg_off, (size_t)npoints + 1);
    const auto bi = s.out<int32_t>(npoints), bm = s.out<int32_t>(npoints);
    HIPTRY(s.alloc());
    const int rc = orbm_distinctive_device(s[d], s[sg], npoints, s[bi], s[bm], nullptr);
    if (rc != ORBX_OK) return rc;
    HIPTRY(s.get(best_idx, bi, npoints));
    HIPTRY(s.get(best_median, bm, npoints));
    return ORBX_OK;
}

}  // extern "C"
