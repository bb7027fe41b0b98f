// Probe (k_describe_od, blur column pass in f16): what v_mfma_f32_16x16x32_f16 and v_cvt_pk_u8_f32 do on gfx950 with the operands the
// 7-tap column pass would give them, before the kernel relies on either.
//   (a) layout    A / B / D lane maps of v_mfma_f32_16x16x32_f16, random small integers against the host product
//   (b) exactness D == S / 65536 (S = sum of tap * Mid, the integer column sum) for 16 x 16 tiles in the kernel's K numbering, two chained
//                 MFMAs per tile, in two operand forms:
//                   form 0  Mid = S_row - 32768: HI signed / LO unsigned as f16, accumulator start 128.5
//                   form 1  Mid = S_row: HI unsigned as f16, LO as 1024 + LO (f16 bit pattern 0x6400 | LO: no conversion), start -1024 * 257 / 65536
//                 columns: all 255, all 0, every bright/dark split both ways, alternating, just below 255.5, random
//   (c) conversion v_cvt_pk_u8_f32 on k + 0.5, k + 0.5 -+ 2^-16, negatives, >= 255.5: which rounding, which saturation
//   (d) rate      SIMD cycles per wave instruction of the f16 shape beside the int8 shape and of the VALU instructions of the new split / epilogue
// build: hipcc --offload-arch=gfx950 -O3 mfma_f16_blur_probe.hip -o mfma_f16_blur_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// ---- (a): A[16][32], B[32][16] small integers; hypothesis: lane l holds A[l % 16][8 (l / 16) + j], B[8 (l / 16) + j][l % 16], D[4 (l / 16) + r][l % 16]
__global__ void k_layout(const int* A, const int* B, float* D) {
    const int l = threadIdx.x, n = l & 15, g = l >> 4;
    h8 a, b;
    for (int j = 0; j < 8; j++) { a[j] = (_Float16)A[n * 32 + 8 * g + j]; b[j] = (_Float16)B[(8 * g + j) * 16 + n]; }
    f4 d = {0.f, 0.f, 0.f, 0.f};
    d = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, d, 0, 0, 0);
    for (int r = 0; r < 4; r++) D[(4 * g + r) * 16 + n] = d[r];
}

// ---- (b): one wave per 16 columns x 16 output rows.  mid[tile][column m][row 0 .. 31] (output row ro sums rows ro .. ro + 6; rows >= 22 have zero taps).
// K numbering of the kernel: the row pass leaves lane (m, g) with Mid rows 16 dt + 4 g + i (dt = 0, 1: the two MFMAs; i = 0 .. 3); slot j of the
// lane's eight: i = 2 (j / 4) + j % 2, HI if (j / 2) % 2 else LO (register pairs LO01, HI01, LO23, HI23).
__host__ __device__ inline int tap7(int t) { return t == 0 || t == 6 ? 18 : t == 1 || t == 5 ? 34 : t == 2 || t == 4 ? 49 : t == 3 ? 55 : 0; }
__global__ void k_exact(const uint16_t* mid, float* out, int form) {
    const int l = threadIdx.x, n = l & 15, g = l >> 4;
    const uint16_t* M = mid + ((size_t)blockIdx.x * 16 + n) * 32;
    const float start = form == 0 ? 128.5f : -(1024.f * 257.f) / 65536.f;
    f4 d = {start, start, start, start};
    for (int dt = 0; dt < 2; dt++) {
        h8 a, b;
        for (int j = 0; j < 8; j++) {
            const int i = 2 * (j >> 2) + (j & 1), hi = (j >> 1) & 1;
            const int s = M[16 * dt + 4 * g + i];
            int v;
            if (form == 0) { const int c = s - 32768; v = hi ? (c >> 8) : (c & 255); }
            else v = hi ? (s >> 8) : 1024 + (s & 255);
            a[j] = (_Float16)v;
            const int t = 16 * dt + 4 * g + i - n;             // lane (n = output row, g) of B
            b[j] = (_Float16)((float)tap7(t) * (hi ? 1.f / 256.f : 1.f / 65536.f));
        }
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, d, 0, 0, 0);
    }
    for (int r = 0; r < 4; r++) out[((size_t)blockIdx.x * 16 + 4 * g + r) * 16 + n] = d[r];      // [column][output row]
}

// ---- (c)
__global__ void k_cvt(const float* in, uint32_t* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out[2 * i] = __builtin_amdgcn_cvt_pk_u8_f32(in[i], 0, 0); out[2 * i + 1] = __builtin_amdgcn_cvt_pk_u8_f32(in[i], 2, 0xAAAAAAAAu); }
}

// ---- (d)
template <int KIND>
__global__ __launch_bounds__(256) void k_mfma_rate(float* out, int iters) {
    i4 a = {(int)threadIdx.x & 3, 1, 2, 3}, b = {1, 0, 1, 0};
    if (KIND == 1) { a = (i4){0x3C003C00, 0x3C003C00, 0x40003C00, 0x3C004000}; b = (i4){0x1C001C00, 0x1C001C00, 0x1C001C00, 0x1C001C00}; }
    i4 ci[4] = {{0, 0, 0, 0}, {1, 1, 1, 1}, {2, 2, 2, 2}, {3, 3, 3, 3}};
    f4 cf[4] = {{0, 0, 0, 0}, {1, 1, 1, 1}, {2, 2, 2, 2}, {3, 3, 3, 3}};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 8; u++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (KIND == 0) ci[q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, ci[q], 0, 0, 0);
                else cf[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), cf[q], 0, 0, 0);
            }
    }
    float s = 0;
    for (int q = 0; q < 4; q++) for (int r = 0; r < 4; r++) s += KIND == 0 ? (float)ci[q][r] : cf[q][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
#define REP8(OP)                                                                                                  \
    asm volatile(OP(%0) OP(%1) OP(%2) OP(%3) OP(%4) OP(%5) OP(%6) OP(%7)                                        \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)             \
                 : "v"(b), "v"(c));
#define KERNEL(NAME, OP)                                                                                          \
    __global__ __launch_bounds__(256) void NAME(unsigned* out, int iters) {                                      \
        unsigned a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7; \
        unsigned b = blockIdx.x & 3u, c = 0x64006400u;                                                            \
        for (int i = 0; i < iters; ++i) {                                                                        \
            REP8(OP) REP8(OP) REP8(OP) REP8(OP) REP8(OP) REP8(OP) REP8(OP) REP8(OP)                              \
            REP8(OP) REP8(OP) REP8(OP) REP8(OP) REP8(OP) REP8(OP) REP8(OP) REP8(OP)                              \
        }                                                                                                        \
        out[blockIdx.x * 256 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;                            \
    }
#define OP_CVTPK(x) "v_cvt_pk_u8_f32 " #x ", " #x ", %8, " #x "\n"
#define OP_RNDNE(x) "v_rndne_f32 " #x ", " #x "\n"
#define OP_PERM(x) "v_perm_b32 " #x ", " #x ", %8, %9\n"
#define OP_PKADDH(x) "v_pk_add_f16 " #x ", " #x ", %9\n"
#define OP_CVTH_SDWA(x) "v_cvt_f16_u16_sdwa " #x ", " #x " dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1\n"
#define OP_MINSDWA(x) "v_min_u16_sdwa " #x ", " #x ", %8 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1 src1_sel:DWORD\n"
#define OP_LSHLADD(x) "v_lshl_add_u32 " #x ", " #x ", 8, %8\n"
KERNEL(k_cvtpk, OP_CVTPK) KERNEL(k_rndne, OP_RNDNE) KERNEL(k_perm, OP_PERM) KERNEL(k_pkaddh, OP_PKADDH) KERNEL(k_cvth, OP_CVTH_SDWA)
KERNEL(k_minsdwa, OP_MINSDWA) KERNEL(k_lshladd, OP_LSHLADD)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main() {
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
    printf("%s, %d CUs\n", pr.gcnArchName, pr.multiProcessorCount);
    // ---- (a)
    {
        int *dA, *dB; float* dD;
        CK(hipMalloc(&dA, 512 * 4)); CK(hipMalloc(&dB, 512 * 4)); CK(hipMalloc(&dD, 256 * 4));
        int bad = 0;
        for (int seed = 0; seed < 16; seed++) {
            int A[512], B[512]; float D[256];
            for (int i = 0; i < 512; i++) { A[i] = (int)(rnd() % 31) - 15; B[i] = (int)(rnd() % 31) - 15; }
            if (seed == 0) for (int i = 0; i < 512; i++) { A[i] = 1 + i % 32; B[i] = (i / 16 == 5 * (i % 16) % 32) ? 1 : 0; }      // one-hot B: D[m][n] = A[m][5 n % 32]
            CK(hipMemcpy(dA, A, sizeof(A), hipMemcpyHostToDevice)); CK(hipMemcpy(dB, B, sizeof(B), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, dA, dB, dD);
            CK(hipMemcpy(D, dD, sizeof(D), hipMemcpyDeviceToHost));
            for (int m = 0; m < 16; m++) for (int n = 0; n < 16; n++) {
                int s = 0;
                for (int k = 0; k < 32; k++) s += A[m * 32 + k] * B[k * 16 + n];
                if (D[m * 16 + n] != (float)s) bad++;
            }
        }
        printf("(a) v_mfma_f32_16x16x32_f16: A[row lane %% 16][k = 8 (lane / 16) + j], B[k = 8 (lane / 16) + j][col lane %% 16], D[row 4 (lane / 16) + reg][col lane %% 16]: %s (%d wrong of %d)\n",
               bad ? "NO" : "yes", bad, 16 * 256);
        hipFree(dA); hipFree(dB); hipFree(dD);
    }
    // ---- (b)
    {
        std::vector<uint16_t> cols;      // 32 rows each
        std::vector<int> kind;
        auto push = [&](int k, auto f) { for (int r = 0; r < 32; r++) cols.push_back((uint16_t)f(r)); kind.push_back(k); };
        const char* names[] = {"all 255", "all 0", "bright/dark split", "alternating", "just below 255.5", "random Mid", "random pixels"};
        push(0, [](int) { return 65535; });
        push(1, [](int) { return 0; });
        for (int s = 0; s <= 22; s++) { push(2, [s](int r) { return r < s ? 65535 : 0; }); push(2, [s](int r) { return r < s ? 0 : 65535; }); }
        for (int s = 0; s <= 22; s++) { push(2, [s](int r) { return r < s ? 257 * 254 : 257; }); push(2, [s](int r) { return r < s ? 255 : 65280; }); }
        push(3, [](int r) { return r & 1 ? 65535 : 0; }); push(3, [](int r) { return r & 1 ? 0 : 65535; });
        push(3, [](int r) { return r & 1 ? 0xFF00 : 0x00FF; }); push(3, [](int r) { return r & 1 ? 0x00FF : 0xFF00; });
        for (int q = 0; q < 4096; q++) push(4, [](int) { return 65150 + (int)(rnd() % 8); });            // 257 * 65153.5 = 255.5 * 65536
        for (int q = 0; q < 32768; q++) push(5, [](int) { return (int)(rnd() & 0xFFFF); });
        for (int q = 0; q < 16384; q++) push(6, [](int) { int s = 0; for (int t = 0; t < 7; t++) s += tap7(t) * (int)(rnd() & 255); return s; });
        while (kind.size() % 16) push(1, [](int) { return 0; });
        const int ncol = (int)kind.size(), ntile = ncol / 16;
        uint16_t* dM; float* dO;
        CK(hipMalloc(&dM, cols.size() * 2)); CK(hipMalloc(&dO, (size_t)ncol * 16 * 4));
        CK(hipMemcpy(dM, cols.data(), cols.size() * 2, hipMemcpyHostToDevice));
        std::vector<float> O((size_t)ncol * 16);
        for (int form = 0; form < 2; form++) {
            hipLaunchKernelGGL(k_exact, dim3(ntile), dim3(64), 0, 0, dM, dO, form);
            CK(hipMemcpy(O.data(), dO, O.size() * 4, hipMemcpyDeviceToHost));
            long bad[7] = {0}, cnt[7] = {0}, badsat = 0, nsat = 0;
            double maxv = 0;
            for (int c = 0; c < ncol; c++) for (int ro = 0; ro < 16; ro++) {
                long S = 0;
                for (int t = 0; t < 7; t++) S += (long)tap7(t) * cols[(size_t)c * 32 + ro + t];
                const float got = O[(size_t)c * 16 + ro];
                if (S < (255L << 16) + 0x8000) {          // not saturating: the float must BE S / 65536
                    cnt[kind[c]]++;
                    if (got != (float)S / 65536.f) { if (!bad[kind[c]]++) printf("    first miss (%s, form %d): S = %ld, got %.8f, want %.8f\n", names[kind[c]], form, S, got, (float)S / 65536.f); }
                    if (got > maxv) maxv = got;
                } else { nsat++; if (!(got >= 255.5f)) badsat++; }
            }
            printf("(b) form %d (%s): ", form, form == 0 ? "HI signed, LO unsigned, start 128.5" : "HI unsigned, LO + 1024, start -4.015625");
            for (int k = 0; k < 7; k++) printf("%s %ld/%ld wrong; ", names[k], bad[k], cnt[k]);
            printf("saturating outputs below 255.5: %ld/%ld; largest exact value %.6f\n", badsat, nsat, maxv);
        }
        hipFree(dM); hipFree(dO);
    }
    // ---- (c)
    {
        std::vector<float> in;
        for (int k = 0; k < 256; k++) { in.push_back(k + 0.5f); in.push_back(k + 0.5f - 1.f / 65536.f); in.push_back(k + 0.5f + 1.f / 65536.f); }
        const int n_half = (int)in.size();
        const float extra[] = {-0.f, -0.25f, -0.5f, -0.75f, -1.f, -4.015625f, -1000.f, -1e30f, 255.5f, 255.5f + 1.f / 65536.f, 255.75f, 256.f, 256.5f, 257.f, 1000.f, 1e30f,
                               0.f, 0.25f, 0.49999f, 0.75f, 1.f, 254.99998f, 255.f, 255.25f, 255.49998f};
        for (float v : extra) in.push_back(v);
        const int n = (int)in.size();
        float* dI; uint32_t* dO;
        CK(hipMalloc(&dI, n * 4)); CK(hipMalloc(&dO, 2 * n * 4));
        CK(hipMemcpy(dI, in.data(), n * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_cvt, dim3((n + 63) / 64), dim3(64), 0, 0, dI, dO, n);
        std::vector<uint32_t> o2(2 * n), o(n);
        CK(hipMemcpy(o2.data(), dO, 2 * n * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) o[i] = o2[2 * i];
        int ne = 0, up = 0, dn = 0, other = 0, near_bad = 0, pack_bad = 0;
        for (int i = 0; i < n; i++) if (o2[2 * i] > 255u || o2[2 * i + 1] != (0xAA00AAAAu | o2[2 * i] << 16)) pack_bad++;
        for (int k = 0; k < 256; k++) {
            const int r = o[3 * k] & 255, ev = (k & 1) ? k + 1 : k, hu = k + 1;
            const int evs = ev > 255 ? 255 : ev, hus = hu > 255 ? 255 : hu;
            if (r == evs && evs != hus) ne++; else if (r == hus && evs != hus) up++; else if (r == k && k != evs) dn++; else if (r != evs) other++;
            if ((int)(o[3 * k + 1] & 255) != k) near_bad++;
            if ((int)(o[3 * k + 2] & 255) != (k + 1 > 255 ? 255 : k + 1)) near_bad++;
        }
        printf("(c) v_cvt_pk_u8_f32 on k + 0.5, k = 0 .. 255: of the 128 even k (where the modes differ) to even %d, up %d; of the odd k down %d; other %d -> %s;  k + 0.5 -+ 2^-16 not to nearest: %d;  byte select / other bytes kept wrong: %d\n",
               ne, up, dn, other, (up == 0 && dn == 0 && other == 0) ? "ROUND TO NEAREST EVEN" : (ne == 0 && dn == 0 && other == 0) ? "HALF UP" : (dn > 0 && up == 0) ? "TRUNCATES (or mixed)" : "MIXED", near_bad, pack_bad);
        printf("    others:");
        for (int i = n_half; i < n; i++) printf(" %g->%u", in[i], o[i] & 255u);
        printf("\n");
        hipFree(dI); hipFree(dO);
    }
    // ---- (d)
    {
        const int cus = pr.multiProcessorCount, blocks = cus * 8 * 4;
        float* out;
        CK(hipMalloc(&out, (size_t)blocks * 256 * 4));
        hipEvent_t e0, e1;
        hipEventCreate(&e0); hipEventCreate(&e1);
        const int iters = 1000;
        typedef void (*kf_t)(float*, int);
        typedef void (*ku_t)(unsigned*, int);
        struct { const char* name; kf_t kf; ku_t ku; int per_iter; } K[] = {
            {"v_mfma_i32_16x16x64_i8", k_mfma_rate<0>, nullptr, 32}, {"v_mfma_f32_16x16x32_f16", k_mfma_rate<1>, nullptr, 32},
            {"v_cvt_pk_u8_f32", nullptr, k_cvtpk, 128}, {"v_rndne_f32", nullptr, k_rndne, 128}, {"v_perm_b32", nullptr, k_perm, 128}, {"v_pk_add_f16", nullptr, k_pkaddh, 128},
            {"v_cvt_f16_u16_sdwa BYTE_1 -> WORD_1", nullptr, k_cvth, 128}, {"v_min_u16_sdwa WORD_1 -> BYTE_1", nullptr, k_minsdwa, 128}, {"v_lshl_add_u32", nullptr, k_lshladd, 128}};
        printf("(d) %d blocks x 256 threads (8 waves per SIMD), %d iterations; cycles at 2.4 GHz\n", blocks, iters);
        for (auto& k : K) {
            for (int pass = 0; pass < 2; pass++) {
                const int it = pass ? iters : 20;
                hipEventRecord(e0, 0);
                if (k.kf) hipLaunchKernelGGL(k.kf, dim3(blocks), dim3(256), 0, 0, out, it);
                else hipLaunchKernelGGL(k.ku, dim3(blocks), dim3(256), 0, 0, (unsigned*)out, it);
                hipEventRecord(e1, 0);
                CK(hipEventSynchronize(e1));
            }
            float ms = 0;
            hipEventElapsedTime(&ms, e0, e1);
            const double insts = (double)blocks * 4 * iters * k.per_iter, rate = insts / (ms * 1e-3);
            printf("    %-38s %8.3f ms  %.3e wave-insts/s  = %.2f cycles per wave64 instruction per SIMD\n", k.name, ms, rate, (double)cus * 4 * 2.4e9 / rate);
        }
        hipFree(out);
    }
    return 0;
}
