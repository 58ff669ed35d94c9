// mr_level_lights_queued.hip -- the level kernels of mr_level_lights.hip and mr_level_lights_path.hip for a queue whose LENGTH is
// a word on the device (mr_render_recursion, mr_api.cpp): level_lights_body<VAR, CHILDREN, PATH, QUEUED = true>
// (mr_level_lights_body.h), the per-ray body of those two units as it stands, with its `n` read by the kernel instead of taken from
// the argument block.
//
// Why.  A level's queue is what the level before it emitted, and how many rays that is only its d_out_count says.  The two
// units above take n from the host (a.tp.n, and trace_grid(n) workgroups), so a recursive frame reads that word back after
// every level: a synchronisation per level, and nothing that a graph can hold.  Here
//
//   n = min(*d_n, n_cap)      d_n: the word the previous level counted its children into, stored or not (the capacity rule of
//                             rec::write_children[_col]: a child beyond capacity is counted, not stored), n_cap: that queue's
//                             capacity -- so n is the number of rays the queue really holds
//
// is read by every lane from the same address before anything else: a wave-uniform load from a kernel argument's pointer, which
// comes out as a scalar load, and n lives in two SGPRs as a.tp.n does in the other units.  The body adds this n to counts[0].
//
// The grid cannot depend on n either.  The host sizes it from an upper bound (launch_level_lights_queued's n_bound: fan^level x
// the frame's samples, or the capacity if that is less), and a workgroup whose first ray index is at or beyond n leaves at once
// -- before the noise tables are staged, before any LDS is touched, before any barrier.  The test is on xcd_block_id() and n
// alone, both the same in every lane of the workgroup: whole workgroups leave, and the ones that stay run every iteration
// whole, as the body's traversals, accumulate_runs and write_children[_col] need.  xcd_block_id() permutes on gridDim.x, so
// first indices still cover 0, 256, ... (gridDim.x - 1) * 256 once each, and blockIdx.x == 0, which adds n to counts[0], has
// first index 0: it stays unless the queue is empty, where there is nothing to add.  An empty queue costs its grid of exits.
//
// d_out_count is NOT zeroed here: mr_render_recursion zeroes every level's counters in one kernel before level 0.
//
// 24 level kernels: the six traversal variants of with_trace_variant x CHILDREN 0 / 1 x the two builds, and the kernel that zeroes
// the counters.  Four waves per SIMD, as the two units above, and their figures give or take n's two SGPRs (hipcc, gfx950, the
// Makefile's flags): 103 to 128 VGPRs, 0 to 68 bytes of scratch per lane, spilled VGPRs 0 except <1818,1> 4 (path 2), <43,1> 2,
// <826,1> 8 (path 5); tests/golden/kernel_budget_level_lights_queued.json holds every kernel.  Times against the per-level
// driver: DESIGN section 5c, profiles/recursion_device_ab.log.
#include <hip/hip_runtime.h>

#include "mr_level_lights_body.h"

namespace mr {
namespace {

#ifndef MIRO_LEVEL_LIGHTS_QUEUED_WAVES
#define MIRO_LEVEL_LIGHTS_QUEUED_WAVES 4
#endif

// VAR, CHILDREN: as in level_lights_kernel / level_lights_path_kernel.  The arguments are taken BY VALUE (mr_lights_body.h says why).
// queued_length (mr_level_lights_body.h): the queue's length, and whether this workgroup has a ray of it.
template <int VAR, int CHILDREN>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_LEVEL_LIGHTS_QUEUED_WAVES, 8))) void level_lights_queued_kernel(
    const LevelLightsArgs a, const unsigned long long *d_n, const unsigned long long n_cap) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    unsigned long long n;
    if (!queued_length(d_n, n_cap, n)) return;        // workgroup-uniform
    level_lights_body<VAR, CHILDREN, false, true>(a, s_stack, s_tab, n);
}

template <int VAR, int CHILDREN>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_LEVEL_LIGHTS_QUEUED_WAVES, 8))) void level_lights_path_queued_kernel(
    const LevelLightsPathArgs a, const unsigned long long *d_n, const unsigned long long n_cap) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    unsigned long long n;
    if (!queued_length(d_n, n_cap, n)) return;        // workgroup-uniform
    level_lights_body<VAR, CHILDREN, true, true>(a, s_stack, s_tab, n);
}

// words[0 .. n) = 0 on the launch's stream, as a kernel (mr_level_lights.hip says what a memset node did on replay)
__global__ void zero_words_kernel(unsigned long long *words, unsigned long long n) {
    const unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) words[k] = 0ull;
}

}  // namespace

unsigned level_lights_queued_grid(unsigned long long n_cap, unsigned long long n_bound) {
    return trace_grid(n_cap < n_bound ? n_cap : n_bound);
}

mr_status launch_zero_words(unsigned long long *d_words, unsigned long long n, hipStream_t stream) {
    if (n == 0) return MR_OK;
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_words, n);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

// LevelLightsArgs or LevelLightsPathArgs for level `lv` between the two queues, and the kernel of that build
mr_status launch_level_lights_queued(const LightScene &ls, const QueuedLevel &lv, const RayQueue &in, const RayQueue &out,
                                     const unsigned long long *d_n, unsigned long long n_cap, unsigned long long n_bound, float *d_rgb,
                                     mr_hit *d_hits, float *d_normal, unsigned long long *row, hipStream_t stream) {
    const DeviceScene &ds = *ls.ds;
    const unsigned grid = level_lights_queued_grid(n_cap, n_bound);
    if (ls.bumped_specular && !lv.path && !lv.last)   // the children bounce about the bumped normal: mr_level_lights_queued_bump.hip
        return launch_level_lights_queued_bumped(ls, lv, in, out, d_n, n_cap, n_bound, d_rgb, d_hits, d_normal, row, stream);
    auto fill = [&](auto &a) {
        fill_level_lights_args(a, ls, lv.spp, lv.environment, in, 0ull, d_rgb, d_hits, nullptr, nullptr, d_normal, out, row + 5, lv.capacity,
                               nullptr, row);
    };
    // the traversal variants of launch_level_lights: the same hit records from each of them
    if (!lv.path) {
        LevelLightsArgs a;
        fill(a);
        return with_trace_variant(ds.n_planes || ds.n_spheres, lv.flags & MR_MATH_PRODUCT, lv.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
            constexpr int VAR = decltype(var)::value;
            const auto kern = lv.last ? &level_lights_queued_kernel<VAR, 0> : &level_lights_queued_kernel<VAR, 1>;
            return launch_traversal(kern, grid, a.tp.stack_depth, stream, a, d_n, n_cap);
        });
    }
    LevelLightsPathArgs a;
    fill(a);
    fill_level_lights_path_args(a, in.ids, in.low, lv.flags, lv.seed, lv.bounce, lv.path_kinds, lv.last ? nullptr : out.low);
    return with_trace_variant(ds.n_planes || ds.n_spheres, lv.flags & MR_MATH_PRODUCT, lv.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        const auto kern = lv.last ? &level_lights_path_queued_kernel<VAR, 0> : &level_lights_path_queued_kernel<VAR, 1>;
        return launch_traversal(kern, grid, a.tp.stack_depth, stream, a, d_n, n_cap);
    });
}

}  // namespace mr
