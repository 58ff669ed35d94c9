// mr_finish_image.hip -- the last step of a frame as the reference takes it (mr_finish_image, include/miro_hip_passes.h):
// Scene.cpp:150-163, 184-197 and Image.cpp:47-52 -- the image's maximum and minimum over all channel values, every NaN channel
// replaced by that maximum, then the tone map (tonemap_byte, mr_tonemap.h: the expression mr_tonemap's kernel calls).  Two kernels
// on the caller's stream, no memset node and no read-back; tests/golden/kernel_budget_finish_image.json holds both.
#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_tonemap.h"

namespace mr {
namespace {

// An order-preserving integer image of a float: a < b as floats <=> key(a) < key(b) as unsigned words (no NaN comes here)
__device__ __forceinline__ uint32_t finish_key_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float finish_value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// first kernel: `>` and `<` from -inf and +inf, so a NaN never wins (Scene.cpp:150-163); a workgroup reduction and one atomic per
// workgroup and bound on state[0] (maximum) / state[1] (minimum), which hold the images of -inf / +inf when the kernel starts
__global__ __launch_bounds__(kBlock) void finish_minmax_kernel(const float *rgb, unsigned long long n_values, uint32_t *state) {
    __shared__ float s_max[kBlock / 64], s_min[kBlock / 64];
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    float hi = -INFINITY, lo = INFINITY;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < n_values; i += stride) {
        const float v = rgb[i];
        if (v > hi) hi = v;
        if (v < lo) lo = v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float h2 = __shfl_xor(hi, off, 64), l2 = __shfl_xor(lo, off, 64);
        if (h2 > hi) hi = h2;
        if (l2 < lo) lo = l2;
    }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = hi; s_min[threadIdx.x >> 6] = lo; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; w++) {
            if (s_max[w] > hi) hi = s_max[w];
            if (s_min[w] < lo) lo = s_min[w];
        }
        atomicMax(&state[0], finish_key_of(hi));
        atomicMin(&state[1], finish_key_of(lo));
    }
}

// second kernel: every lane reads the maximum from the same word, replaces its NaN channels by it (Scene.cpp:184-197) and maps.
// A workgroup takes a ticket (state[2]) once all its lanes have read; the one that draws the last ticket knows every read of the
// state is over: it writes (max, min) for the caller and puts the identities back, so the next call starts from them
__global__ __launch_bounds__(kBlock) void finish_map_kernel(const float *rgb, unsigned long long n_values, uint8_t *out, float *minmax,
                                                            uint32_t *state) {
    const float hi = finish_value_of(state[0]);                     // every lane, one address: wave-uniform
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < n_values; i += stride) {
        float v = rgb[i];
        if (v != v) v = hi;
        out[i] = tonemap_byte(v);
    }
    __threadfence();                                                // the read of the state before the ticket
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(&state[2], 1u) == gridDim.x - 1) {
        if (minmax) { minmax[0] = hi; minmax[1] = finish_value_of(state[1]); }
        state[0] = kFinishMaxIdentity; state[1] = kFinishMinIdentity; state[2] = 0u;
    }
}

}  // namespace

mr_status launch_finish_image(const float *d_rgb, unsigned long long n_values, uint8_t *d_out, float *d_minmax, uint32_t *d_state,
                              hipStream_t stream) {
    if (n_values == 0) return MR_OK;
    hipLaunchKernelGGL(finish_minmax_kernel, dim3(grid_for(n_values)), dim3(kBlock), 0, stream, d_rgb, n_values, d_state);
    MR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(finish_map_kernel, dim3(grid_for(n_values)), dim3(kBlock), 0, stream, d_rgb, n_values, d_out, d_minmax, d_state);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
