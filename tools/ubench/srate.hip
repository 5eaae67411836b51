// Scalar ALU issue rate of a gfx950 CU (one scalar unit for its four SIMDs): each wave runs ITER
// iterations of 64 scalar instructions on 8 independent SGPR chains (inline asm, so the compiler
// cannot fold them), from 1, 2, 4 and 8 waves per SIMD on all four SIMDs of every CU — blocks of
// 256 threads, CUs x W of them, each asking for so much LDS that exactly W fit a CU. Each stream
// runs once alone and once with one independent v_add_f32 after every scalar instruction (the
// render kernel's mix is one scalar instruction to two or three VALU). Scalar instructions per
// cycle per CU = waves x ITER x 64 / (time x clock x CUs); the loop's own s_add / s_cmp (2 per 64)
// are not counted. Run: hipcc --offload-arch=gfx950 -O2 srate.hip && ./a.out
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

constexpr int ITER = 2048;

#define S8(ins) \
    ins " %0, %0, %8\n" ins " %1, %1, %8\n" ins " %2, %2, %8\n" ins " %3, %3, %8\n" \
    ins " %4, %4, %8\n" ins " %5, %5, %8\n" ins " %6, %6, %8\n" ins " %7, %7, %8\n"
#define SV8(ins) \
    ins " %0, %0, %16\n v_add_f32 %8, %8, %8\n" ins " %1, %1, %16\n v_add_f32 %9, %9, %9\n" \
    ins " %2, %2, %16\n v_add_f32 %10, %10, %10\n" ins " %3, %3, %16\n v_add_f32 %11, %11, %11\n" \
    ins " %4, %4, %16\n v_add_f32 %12, %12, %12\n" ins " %5, %5, %16\n v_add_f32 %13, %13, %13\n" \
    ins " %6, %6, %16\n v_add_f32 %14, %14, %14\n" ins " %7, %7, %16\n v_add_f32 %15, %15, %15\n"
#define X8(B) B B B B B B B B

// T: uint32_t for 32-bit instructions, uint64_t for the 64-bit lane-mask ones
#define KS(name, T, ins)                                                                         \
    __global__ void name(uint32_t *out, uint32_t seed) {                                         \
        T s0 = seed, s1 = seed + 1, s2 = seed + 2, s3 = seed + 3, s4 = seed + 4, s5 = seed + 5, s6 = seed + 6, s7 = seed + 7; \
        const T k = seed | 1u;                                                                   \
        for (int i = 0; i < ITER; ++i) {                                                         \
            asm volatile(X8(S8(ins))                                                             \
                         : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3), "+s"(s4), "+s"(s5), "+s"(s6), "+s"(s7) \
                         : "s"(k) : "scc");                                                      \
        }                                                                                        \
        out[blockIdx.x * blockDim.x + threadIdx.x] = (uint32_t)(s0 ^ s1 ^ s2 ^ s3 ^ s4 ^ s5 ^ s6 ^ s7); \
    }
#define KSV(name, T, ins)                                                                        \
    __global__ void name(uint32_t *out, uint32_t seed) {                                         \
        T s0 = seed, s1 = seed + 1, s2 = seed + 2, s3 = seed + 3, s4 = seed + 4, s5 = seed + 5, s6 = seed + 6, s7 = seed + 7; \
        const T k = seed | 1u;                                                                   \
        float v0 = (float)threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7; \
        for (int i = 0; i < ITER; ++i) {                                                         \
            asm volatile(X8(SV8(ins))                                                            \
                         : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3), "+s"(s4), "+s"(s5), "+s"(s6), "+s"(s7), \
                           "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7) \
                         : "s"(k) : "scc"); \
        }                                                                                        \
        out[blockIdx.x * blockDim.x + threadIdx.x] = (uint32_t)(s0 ^ s1 ^ s2 ^ s3 ^ s4 ^ s5 ^ s6 ^ s7) ^ __float_as_uint(v0 + v1 + v2 + v3 + v4 + v5 + v6 + v7); \
    }

KS(k_add, uint32_t, "s_add_u32")
KSV(k_add_v, uint32_t, "s_add_u32")
KS(k_and64, uint64_t, "s_and_b64")
KSV(k_and64_v, uint64_t, "s_and_b64")

// the VALU stream alone: the cross-check of the clock (v_add_f32 issue cost, vrate.hip)
__global__ void k_valu(uint32_t *out, uint32_t seed) {
    float v0 = (float)(seed ^ threadIdx.x), v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5, v6 = v0 + 6, v7 = v0 + 7;
    for (int i = 0; i < ITER; ++i) {
        asm volatile(X8("v_add_f32 %0, %0, %0\n v_add_f32 %1, %1, %1\n v_add_f32 %2, %2, %2\n v_add_f32 %3, %3, %3\n"
                        "v_add_f32 %4, %4, %4\n v_add_f32 %5, %5, %5\n v_add_f32 %6, %6, %6\n v_add_f32 %7, %7, %7\n")
                     : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7));
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = __float_as_uint(v0 + v1 + v2 + v3 + v4 + v5 + v6 + v7);
}

typedef void (*K)(uint32_t *, uint32_t);
int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 1;
    int clk_khz = 0;
    (void)hipDeviceGetAttribute(&clk_khz, hipDeviceAttributeClockRate, 0);
    const int cus = p.multiProcessorCount, threads = 256;
    uint32_t *out;
    if (hipMalloc(&out, (size_t)cus * 8 * threads * 4) != hipSuccess) return 1;
    struct { const char *n; K k; } ks[] = {{"s_add_u32", k_add}, {"s_add_u32 + v_add_f32", k_add_v}, {"s_and_b64", k_and64},
                                          {"s_and_b64 + v_add_f32", k_and64_v}, {"v_add_f32 alone", k_valu}};
    // LDS per block that lets exactly W blocks share a CU's 160 KB
    const struct { int w; size_t lds; } ws[] = {{1, 96u << 10}, {2, 64u << 10}, {4, 36u << 10}, {8, 18u << 10}};
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    printf("CUs %d clock %d MHz\n", cus, clk_khz / 1000);
    for (auto &k : ks) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k.k), hipFuncAttributeMaxDynamicSharedMemorySize, 96 << 10) != hipSuccess) return 1;
        for (auto &w : ws) {
            const int blocks = cus * w.w, reps = 5;
            hipLaunchKernelGGL(k.k, dim3(blocks), dim3(threads), w.lds, 0, out, 1u);
            (void)hipEventRecord(a);
            for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k.k, dim3(blocks), dim3(threads), w.lds, 0, out, 1u);
            (void)hipEventRecord(b);
            if (hipEventSynchronize(b) != hipSuccess) return 1;
            float ms = 0;
            (void)hipEventElapsedTime(&ms, a, b);
            const double insts = (double)reps * blocks * (threads / 64) * ITER * 64.0;  // per class
            const double cu_cycles = ms * 1e-3 * clk_khz * 1e3 * cus;
            printf("%-24s %d waves/SIMD %8.3f ms  %.3f instructions per cycle per CU (%.2f cycles each)\n", k.n, w.w, ms / reps,
                   insts / cu_cycles, cu_cycles / insts);
        }
    }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
