// Exhaustive device check of short square roots against the correctly rounded one
// (-fhip-fp32-correctly-rounded-divide-sqrt). Every candidate starts from a hardware estimate; the
// domain that counts is the kernel's sqrt_rn_big: x = +0 or x >= 2^-96, +inf and positive NaNs
// included. Per candidate: mismatches by range of x, and the lowest and highest failing input of
// the domain.
//   0  neighbours  s = v_sqrt_f32(x), the one-ulp neighbours chosen by the sign of the fma remainders
//                  with two compares and two selects (the compiler's own correction, without its
//                  small-input scaling and class fix-up): 8 instructions after v_sqrt_f32
//   1  med3        the same neighbours and remainders, the choice as integers: s - 1 + [rm > 0] +
//                  [rp > 0], each bracket one v_med3_i32 of the remainder's bits into [0, 1] and the sum
//                  one v_add3_u32: 7 instructions, no compare, no mask
//   2  residual    r = fma(-s, s, x), s' = fma(r, h, s) with h = 0.5 * v_rsq_f32(x); x = 0 and inf keep
//                  s by one v_cmp_class and a select: 6 instructions, two of them transcendental
//   3  rsq only    y = v_rsq_f32(x), s = x * y, h = 0.5 * y, r = fma(-s, s, x), s' = fma(r, h, s), the
//                  same class fix-up (selecting x itself): 7 instructions, one transcendental
//   4  residual, NaN dropped  candidate 2 without the compare: fmaxf(r, bound) turns the NaN residual of
//                  x = inf into a finite value, whose product with h = 0 leaves s = inf; x = 0 (h = inf) is
//                  not covered: 6 instructions, two of them transcendental, x dead after the residual.
//                  With bound = -2^100: 1964 mismatches above 0, up to bits 0x7f4cdadb (residuals of x near
//                  2^127 reach 2^103)
//   5  the same with bound = -FLT_MAX
//   6  rsq only, div_fixup  candidate 3 without the compare: v_div_fixup_f32(s', y, 1.0) returns +inf for a
//                  zero y (x = inf), +-0 for an infinite y (x = +-0) and s' otherwise: 6 instructions, one
//                  transcendental, x dead after the residual (the kernel's sqrt_rn_res)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

__device__ __forceinline__ float sqrt_neighbours(float x) {
    float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = __builtin_fmaf(-sm, s, x), rp = __builtin_fmaf(-sp, s, x);
    s = rm <= 0.0f ? sm : s;
    s = rp > 0.0f ? sp : s;
    return s;
}
__device__ __forceinline__ int med3_i32(int a, int b, int c) {
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float sqrt_med3(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const uint32_t um = __float_as_uint(s) - 1u;
    const float sm = __uint_as_float(um), sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = __builtin_fmaf(-sm, s, x), rp = __builtin_fmaf(-sp, s, x);
    const int a = med3_i32((int)__float_as_uint(rm), 0, 1), b = med3_i32((int)__float_as_uint(rp), 0, 1);
    return __uint_as_float(um + (uint32_t)a + (uint32_t)b);
}
__device__ __forceinline__ float sqrt_residual(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const bool keep = __builtin_isfpclass(x, 0x260);  // +-0, +inf
    const float h = 0.5f * __builtin_amdgcn_rsqf(x);
    const float r = __builtin_fmaf(-s, s, x);
    const float t = __builtin_fmaf(r, h, s);
    return keep ? s : t;
}
__device__ __forceinline__ float sqrt_rsq_only(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    const bool keep = __builtin_isfpclass(x, 0x260);
    const float s = x * y, h = 0.5f * y;
    const float r = __builtin_fmaf(-s, s, x);
    const float t = __builtin_fmaf(r, h, s);
    return keep ? x : t;
}
__device__ __forceinline__ float sqrt_residual_max(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float h = 0.5f * __builtin_amdgcn_rsqf(x);
    const float r = __builtin_fmaxf(__builtin_fmaf(-s, s, x), -0x1.0p100f);
    return __builtin_fmaf(r, h, s);
}
__device__ __forceinline__ float sqrt_residual_max_flt(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float h = 0.5f * __builtin_amdgcn_rsqf(x);
    const float r = __builtin_fmaxf(__builtin_fmaf(-s, s, x), -0x1.fffffep127f);
    return __builtin_fmaf(r, h, s);
}
__device__ __forceinline__ float sqrt_rsq_fixup(float x) {
    const float y = __builtin_amdgcn_rsqf(x);
    const float s = x * y, h = 0.5f * y;
    const float r = __builtin_fmaf(-s, s, x);
    const float t = __builtin_fmaf(r, h, s);
    return __builtin_amdgcn_div_fixupf(t, y, 1.0f);
}
__device__ __forceinline__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

constexpr int kCandidates = 7;
struct Result {
    unsigned long long bad[3];  // x < 2^-96 non-negative (0 excluded) | the domain | x < 0 (-0 included)
    uint32_t lo, hi;
};

__global__ void check(Result *res) {
    for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < (1ull << 32); k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t u = (uint32_t)k;
        const float x = __uint_as_float(u);
        const float want = __builtin_sqrtf(x);
        const float got[kCandidates] = {sqrt_neighbours(x), sqrt_med3(x), sqrt_residual(x), sqrt_rsq_only(x), sqrt_residual_max(x), sqrt_residual_max_flt(x), sqrt_rsq_fixup(x)};
        const int c = (u >> 31) ? 2 : ((u != 0u && u < 0x0f800000u) ? 0 : 1);
        for (int j = 0; j < kCandidates; ++j) {
            if (same(got[j], want)) continue;
            atomicAdd(&res[j].bad[c], 1ull);
            if (c == 1) {
                atomicMin(&res[j].lo, u);
                atomicMax(&res[j].hi, u);
            }
        }
    }
}

int main() {
    Result *d, h[kCandidates];
    for (int j = 0; j < kCandidates; ++j) h[j] = Result{{0, 0, 0}, 0xffffffffu, 0u};
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 2;
    if (hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) return 2;
    hipLaunchKernelGGL(check, dim3(16384), dim3(256), 0, 0, d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 3;
    const char *names[kCandidates] = {"neighbours", "med3", "residual", "rsq only", "residual, NaN dropped", "the same, -FLT_MAX", "rsq only, div_fixup"};
    for (int j = 0; j < kCandidates; ++j) {
        printf("%-22s  x = +0 or x >= 2^-96: %llu mismatches", names[j], h[j].bad[1]);
        if (h[j].bad[1]) printf(" (bits 0x%08x..0x%08x)", h[j].lo, h[j].hi);
        printf("; 0 < x < 2^-96: %llu; x < 0 or -0: %llu\n", h[j].bad[0], h[j].bad[2]);
    }
    return 0;
}
