// mr_level_lights_queued_bump.hip -- the specular level WITH children of mr_render_recursion[_lens|_photons|_passes] on a scene
// where a STONE material reflects (mr_scene_set_textures: bumped_specular): level_lights_body<VAR, 1, false, QUEUED = true,
// BUMPED = true> (mr_level_lights_body.h), the kernel of mr_level_lights_queued.hip whose children take their N from the surface
// step -- the normal Scene::trace hands on, bumped on STONE -- as mr_level_lights_bump.hip's do for a queue whose length the host
// knows.  The queue's length, the grid, the early exit of workgroups beyond the length and the counters are
// mr_level_lights_queued.hip's, which says why each is as it is; launch_level_lights_queued hands such a level on to this unit
// and launches its own kernels for every other level and scene.  Level 0 of those frames (mr_frame_level_lights.hip,
// mr_frame_lens.hip, mr_frame_passes.hip) and the PATH levels take the surface step's N already and need no other kernel.
//
// A unit of its own because the 24 level kernels of mr_level_lights_queued.hip are held, by name and by number, to
// tests/golden/kernel_budget_level_lights_queued.json; this unit's record is kernel_budget_level_lights_queued_bump.json.  Six
// kernels, one per traversal variant, four waves per SIMD.
#include <hip/hip_runtime.h>

#include "mr_level_lights_body.h"

namespace mr {
namespace {

#ifndef MIRO_LEVEL_LIGHTS_QUEUED_WAVES
#define MIRO_LEVEL_LIGHTS_QUEUED_WAVES 4
#endif

// VAR: as in level_lights_queued_kernel.  The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_LEVEL_LIGHTS_QUEUED_WAVES, 8))) void level_lights_queued_bumped_kernel(
    const LevelLightsArgs a, const unsigned long long *d_n, const unsigned long long n_cap) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    unsigned long long n;
    if (!queued_length(d_n, n_cap, n)) return;        // workgroup-uniform
    level_lights_body<VAR, 1, false, true, true>(a, s_stack, s_tab, n);
}

}  // namespace

mr_status launch_level_lights_queued_bumped(const LightScene &ls, const QueuedLevel &lv, const RayQueue &in, const RayQueue &out,
                                            const unsigned long long *d_n, unsigned long long n_cap, unsigned long long n_bound, float *d_rgb,
                                            mr_hit *d_hits, float *d_normal, unsigned long long *row, hipStream_t stream) {
    const DeviceScene &ds = *ls.ds;
    const unsigned grid = level_lights_queued_grid(n_cap, n_bound);
    LevelLightsArgs a;
    fill_level_lights_args(a, ls, lv.spp, lv.environment, in, 0ull, d_rgb, d_hits, nullptr, nullptr, d_normal, out, row + 5, lv.capacity,
                           nullptr, row);
    return with_trace_variant(ds.n_planes || ds.n_spheres, lv.flags & MR_MATH_PRODUCT, lv.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        return launch_traversal(&level_lights_queued_bumped_kernel<VAR>, grid, a.tp.stack_depth, stream, a, d_n, n_cap);
    });
}

}  // namespace mr
