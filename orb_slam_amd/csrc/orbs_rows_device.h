// Device code the searches over resident key-frame rows share (orbs_bow_rows.hip, orbs_tri_rows.hip): the second kernel of both, which turns
// the one-record-per-list-position scratch of a pair into its feature-indexed outputs.
#pragma once
#include <hip/hip_runtime.h>

#include "orbs_bow_rows.h"
#include "orbs_device.h"

namespace orbs {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// One workgroup of TPB threads finishes pair p = (query row qr, train row tr): it sets the pair's outputs to -1, walks the records of the query
// row's list, builds the rotation histogram in LDS (integer adds: the result does not depend on their order), takes the three maxima, writes the
// surviving matches to q2t / t2q, best / second of every listed query, and the count.  Without `rot` it only scatters and counts.  A filtered
// match kept its claim during the scan, as in the reference.  rec, O: the pair's records and outputs start at + p * cap.
template <int TPB>
__device__ __forceinline__ void rows_finish(bool rot, const BowStore& S, int qr, int tr, const BowOut& O, const BowRec* rec, int p) {
    __shared__ int hist[32];
    __shared__ int total;
    const int tid = threadIdx.x, cap = S.cap;
    const size_t ob = (size_t)p * cap;
    for (int i = tid; i < cap; i += TPB) {
        if (O.q2t) O.q2t[ob + i] = -1;
        if (O.t2q) O.t2q[ob + i] = -1;
        if (O.best) O.best[ob + i] = -1;
        if (O.second) O.second[ob + i] = -1;
    }
    if (tid < 32) hist[tid] = 0;
    if (tid == 0) total = 0;
    const bool known = (unsigned)qr < (unsigned)S.nrows && (unsigned)tr < (unsigned)S.nrows;
    __syncthreads();                                                     // the -1s are in place before any entry is written again
    if (!known) {
        if (tid == 0) O.nmatches[p] = 0;
        return;
    }
    const int32_t* qo = S.fv_off + (size_t)qr * (cap + 1);
    const uint32_t* qf = S.fv_feat + (size_t)qr * cap;
    const int nfq = clampi(S.nfv[qr], 0, cap);
    const int ntq = clampi(S.nt[qr], 0, cap), ntt = clampi(S.nt[tr], 0, cap);
    const int k0 = nfq > 0 ? clampi(qo[0], 0, cap) : 0, k1 = nfq > 0 ? clampi(qo[nfq], k0, cap) : 0;

    for (int k = k0 + tid; k < k1; k += TPB) {
        const uint32_t idx1 = qf[k];
        if (idx1 >= (uint32_t)ntq) continue;
        const BowRec r = rec[ob + k];
        if (O.best) O.best[ob + idx1] = r.best;
        if (O.second) O.second[ob + idx1] = r.second;
        if (rot && (unsigned)r.idx2 < (unsigned)ntt && (unsigned)r.bin < (unsigned)HISTO_LENGTH) atomicAdd(&hist[r.bin], 1);
    }
    __syncthreads();
    int i1 = -1, i2 = -1, i3 = -1;
    if (rot) three_maxima(hist, HISTO_LENGTH, i1, i2, i3);
    int cnt = 0;
    for (int k = k0 + tid; k < k1; k += TPB) {
        const uint32_t idx1 = qf[k];
        if (idx1 >= (uint32_t)ntq) continue;
        const BowRec r = rec[ob + k];
        if ((unsigned)r.idx2 >= (unsigned)ntt) continue;
        if (rot && (unsigned)r.bin < (unsigned)HISTO_LENGTH && r.bin != i1 && r.bin != i2 && r.bin != i3) continue;      // cleared; its claim held during the scan
        if (O.q2t) O.q2t[ob + idx1] = r.idx2;
        if (O.t2q) O.t2q[ob + r.idx2] = (int)idx1;
        cnt++;
    }
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(&total, cnt);
    __syncthreads();
    if (tid == 0) O.nmatches[p] = total;
}

constexpr int ROWS_FINISH_TPB = 256;

}  // namespace orbs
