// pow_zero_probe.hip -- below which x is this device's powf(x, 500.0f) bitwise +0?  
//
// highlight_of (mr_phong.h) may write e = +0 without calling powf when every lane's clamped e is below kHighlightZeroBelow.
// That is right if powf(x, 500.0f) is +0 for EVERY float x of [0, kHighlightZeroBelow): this probe runs the call highlight_of
// makes -- highlight_pow of mr_phong.h, compiled with the Makefile's HIPFLAGS -- on every float bit pattern of [0, 1]
// (0x00000000 .. 0x3F800000: 1 065 353 217 values) and prints
//   X, the largest float such that the result is bitwise +0 for every float of [0, X];
//   how many floats above X give +0 all the same (if any: the results are not monotone there, and X is the safe bound);
//   the first few floats above X with their results; the results at 0, at the smallest denormal and at 1;
//   whether kHighlightZeroBelow <= X (exit status 1 if not).
// In the reals x^500 < 2^-150 (half the smallest denormal) for x < 2^-0.3 = 0.81225.
//   make -C cse168-raytracer_amd tools && cse168-raytracer_amd/build/pow_zero_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "mr_phong.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } } while (0)

constexpr uint32_t kOne = 0x3F800000u;      // 1.0f: the last pattern probed

// out[0]: the smallest bit pattern whose result is not bitwise +0; out[1]: how many patterns give bitwise +0 (in all)
__global__ void scan(unsigned long long *out) {
    unsigned long long first = ~0ull, zeros = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i <= kOne; i += (unsigned long long)gridDim.x * blockDim.x) {
        const float y = mr::highlight_pow(__uint_as_float((uint32_t)i));
        if (__float_as_uint(y) == 0u) zeros++;
        else if (i < first) first = i;
    }
    if (first != ~0ull) atomicMin(&out[0], first);
    atomicAdd(&out[1], zeros);
}
__global__ void eval(const uint32_t *x, uint32_t *y, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __float_as_uint(mr::highlight_pow(__uint_as_float(x[i])));
}

static float as_float(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }
static uint32_t as_bits(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }

int main() {
    unsigned long long *d_out, out[2] = {~0ull, 0ull};
    CHECK(hipMalloc(&d_out, sizeof(out)));
    CHECK(hipMemcpy(d_out, out, sizeof(out), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(scan, dim3(256 * 32), dim3(256), 0, 0, d_out);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out, d_out, sizeof(out), hipMemcpyDeviceToHost));
    if (out[0] == ~0ull || out[0] == 0ull) { printf("no float of [0, 1] or the first one gives a result other than +0: %llu\n", out[0]); return 1; }
    const uint32_t first = (uint32_t)out[0], X = first - 1u;
    printf("powf(x, 500.0f) as highlight_of calls it, every float bit pattern of [0, 1]: %llu values\n", (unsigned long long)kOne + 1ull);
    printf("X = %.9g (%a, 0x%08X): bitwise +0 for every float of [0, X]\n", as_float(X), as_float(X), X);
    printf("floats above X with a result of +0: %llu\n", out[1] - (unsigned long long)first);

    constexpr int kN = 12;
    uint32_t xs[kN], ys[kN];
    const char *what[kN] = {"X", "X + 1 ulp", "X + 2 ulp", "X + 3 ulp", "X + 4 ulp", "X + 5 ulp", "X + 6 ulp", "0", "smallest denormal", "1",
                            "kHighlightZeroBelow", "kHighlightZeroBelow - 1 ulp"};
    for (int k = 0; k < 7; k++) xs[k] = X + (uint32_t)k;
    xs[7] = 0u; xs[8] = 1u; xs[9] = kOne; xs[10] = as_bits(mr::kHighlightZeroBelow); xs[11] = xs[10] - 1u;
    uint32_t *d_x, *d_y;
    CHECK(hipMalloc(&d_x, sizeof(xs))); CHECK(hipMalloc(&d_y, sizeof(ys)));
    CHECK(hipMemcpy(d_x, xs, sizeof(xs), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval, dim3(1), dim3(64), 0, 0, d_x, d_y, kN);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(ys, d_y, sizeof(ys), hipMemcpyDeviceToHost));
    for (int k = 0; k < kN; k++) printf("  %-28s x = %-14.9g 0x%08X   powf(x, 500) = %-14.9g 0x%08X\n", what[k], as_float(xs[k]), xs[k], as_float(ys[k]), ys[k]);
    const bool ok = as_bits(mr::kHighlightZeroBelow) <= X;       // (positive floats order as their bit patterns)
    printf("%s: kHighlightZeroBelow = %.9g %s X\n", ok ? "OK" : "FORBIDDEN", mr::kHighlightZeroBelow, ok ? "<=" : ">");
    return ok ? 0 : 1;
}
