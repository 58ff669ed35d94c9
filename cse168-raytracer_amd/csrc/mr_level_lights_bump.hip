// mr_level_lights_bump.hip -- mr_trace_level_lights' level with specular children on a scene where a STONE material reflects
// (mr_scene_set_textures: bumped_specular): level_lights_body<VAR, 1, false, false, BUMPED = true> (mr_level_lights_body.h), the
// kernel of mr_level_lights.hip with ONE step changed -- the children's N is the surface step's, the normal Scene::trace hands on
// (Scene.cpp:234-263: bumped on STONE, then normalised), about which Ray::reflect bounces (Ray.h:156), not the object's own rebuilt
// from the hit record.  Everything else, and every other scene, is mr_level_lights.hip's: launch_level_lights hands a level WITH
// children on a bumped_specular scene on to this unit and launches its own kernels otherwise (a last level has no children and
// needs no other kernel).  The batched chain such a level equals:
//   mr_trace -> mr_shade_environment -> mr_hit_surface -> mr_shade_lights_surface -> mr_gen_secondary_rays_surface;
// tests/test_bump_specular.py compares level by level on the same queues.
//
// A unit of its own because the twelve kernels of mr_level_lights.hip are held, by name and by number, to
// tests/golden/kernel_budget_level_lights.json; this unit's record is kernel_budget_level_lights_bump.json.  Six kernels, one per
// traversal variant of with_trace_variant, CHILDREN == 1 only.  Four waves per SIMD, the family's setting.  N is live through the
// light loop in both forms, and this form drops the normalize3 of the rebuilt normal: the figures are those of
// level_lights_kernel<VAR, 1> or below them (DESIGN section 5c has the table).
#include <hip/hip_runtime.h>

#include "mr_level_lights_body.h"

namespace mr {
namespace {

#ifndef MIRO_LEVEL_LIGHTS_WAVES
#define MIRO_LEVEL_LIGHTS_WAVES 4
#endif

// VAR: the traversal variant of trace_ray (mr_traverse.h) for the ray and its shadow rays.  The arguments are taken BY VALUE
// (mr_lights_body.h says why).
template <int VAR>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_LEVEL_LIGHTS_WAVES, 8))) void level_lights_bumped_kernel(
    const LevelLightsArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    level_lights_body<VAR, 1, false, false, true>(a, s_stack, s_tab);
}

}  // namespace

mr_status launch_level_lights_bumped(const LightScene &ls, const mr_level_lights_desc &ld, const mr_ray *d_rays, const float *d_weights,
                                     const uint32_t *d_pixels, unsigned long long n, float *d_rgb, mr_hit *d_hits, float *d_ray_rgb,
                                     float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                                     unsigned long long *d_out_count, unsigned long long *d_counts, hipStream_t stream) {
    const mr_status zs = launch_zero_count(d_out_count, stream);
    if (zs != MR_OK) return zs;
    if (n == 0) return MR_OK;
    LevelLightsArgs a;
    const RayQueue in = {const_cast<mr_ray *>(d_rays), const_cast<float *>(d_weights), const_cast<uint32_t *>(d_pixels), nullptr, nullptr};   // only read
    const RayQueue out = {d_out_rays, d_out_weights, d_out_pixels, nullptr, nullptr};
    fill_level_lights_args(a, ls, ld.spp, ld.environment, in, n, d_rgb, d_hits, d_ray_rgb, d_color, d_normal, out, d_out_count,
                           out_capacity_of(ld), ld.d_out_octants, d_counts);

    // the traversal variants of launch_level_lights: the same hit records from each of them
    const DeviceScene &ds = *ls.ds;
    return with_trace_variant(ds.n_planes || ds.n_spheres, ld.flags & MR_MATH_PRODUCT, ld.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        return launch_traversal(&level_lights_bumped_kernel<VAR>, trace_grid(n), a.tp.stack_depth, stream, a);
    });
}

}  // namespace mr
