// mr_level_lights.hip -- ONE level of Scene::traceScene's recursion (Scene.cpp:270-346) for a queue of rays in ONE launch on ANY
// scene (mr_trace_level_lights).  The kernel is level_lights_body<VAR, CHILDREN, false> (mr_level_lights_body.h, where the per-ray
// sequence, what it saves and what it does not buy are described), the body mr_level_lights_path.hip instantiates with PATH =
// true: a miss reads the full environment image (env_lookup_full), and the children are those of Ray::reflect /
// getReflectionCoefficient / refract (Scene.cpp:302-336).
//
// It joins two kernels: mr_level.hip's level (queue in, accumulate_runs, ChildGen<false>, write_children), which shades by one
// point light with the plain material table, and the per-sample body of the fused light-list frames
// (mr_frame_lights_surface_body.h: hit_color_normal, shade_light_list, env_lookup_full), which stops at the eye ray's hit.  The
// batched route runs such a level as five launches,
//   mr_trace -> mr_shade_environment -> mr_hit_surface -> mr_shade_lights_surface -> mr_gen_secondary_rays;
// tests/test_level_lights.py compares level by level on the same queues.
//
// The children bounce about the normal and material mr_gen_secondary_rays uses -- the object's own normal, normalised.  That is
// the normal Scene::trace hands on wherever a child exists, unless a STONE material reflects (mr_scene_set_textures:
// bumped_specular; a STONE material never transmits): a level with children on such a scene is handed on to
// mr_level_lights_bump.hip, whose kernels are this body with BUMPED set and take the children's N from the surface step, as
// mr_gen_secondary_rays_surface reads it from mr_hit_surface's buffer.  A unit of its own so that this unit's twelve kernels and
// their record stay what they are.  A specular child is never isDiffuse: the low-res image is not read.  Times against the
// batched route: DESIGN section 5c, profiles/level_lights_ab.log.
//
// Live state, besides what the body lists: the children's own normal is computed again from the hit record.  Four waves per SIMD,
// as every frame_lights_env_kernel: at six the specular level_kernel of mr_level.hip already spills 30 VGPRs without a light loop
// or a lookup.
#include <hip/hip_runtime.h>

#include "mr_level_lights_body.h"

namespace mr {
namespace {

#ifndef MIRO_LEVEL_LIGHTS_WAVES
#define MIRO_LEVEL_LIGHTS_WAVES 4
#endif

// VAR: the traversal variant of trace_ray (mr_traverse.h) for the ray and its shadow rays; CHILDREN: 0 none, 1 specular.
// The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, int CHILDREN>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_LEVEL_LIGHTS_WAVES, 8))) void level_lights_kernel(
    const LevelLightsArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    level_lights_body<VAR, CHILDREN, false>(a, s_stack, s_tab);
}

// d_out_count = 0 on the launch's stream, as a kernel.  mr_trace_level and the generators use hipMemsetAsync for this word; captured
// into a graph, that 8-byte memset node has been seen to fill the word with a wrong byte on replay (each byte 0x04 or 0x10
// instead of 0, depending on where the word lies in its allocation; the direct call is always right).  A store from a kernel node
// replays as written.
__global__ void zero_count_kernel(unsigned long long *count) {
    if (threadIdx.x == 0) *count = 0ull;
}

}  // namespace

mr_status launch_zero_count(unsigned long long *d_count, hipStream_t stream) {
    hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(64), 0, stream, d_count);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_level_lights(const LightScene &ls, const mr_level_lights_desc &ld, const mr_ray *d_rays, const float *d_weights,
                              const uint32_t *d_pixels, unsigned long long n, float *d_rgb, mr_hit *d_hits, float *d_ray_rgb,
                              float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                              unsigned long long *d_out_count, unsigned long long *d_counts, hipStream_t stream) {
    if (ls.bumped_specular && ld.children != MR_LEVEL_LAST)
        return launch_level_lights_bumped(ls, ld, d_rays, d_weights, d_pixels, n, d_rgb, d_hits, d_ray_rgb, d_color, d_normal, d_out_rays,
                                          d_out_weights, d_out_pixels, d_out_count, d_counts, stream);
    if (ld.children != MR_LEVEL_LAST) {
        const mr_status zs = launch_zero_count(d_out_count, stream);
        if (zs != MR_OK) return zs;
    }
    if (n == 0) return MR_OK;
    LevelLightsArgs a;
    const RayQueue in = {const_cast<mr_ray *>(d_rays), const_cast<float *>(d_weights), const_cast<uint32_t *>(d_pixels), nullptr, nullptr};   // only read
    const RayQueue out = {d_out_rays, d_out_weights, d_out_pixels, nullptr, nullptr};
    fill_level_lights_args(a, ls, ld.spp, ld.environment, in, n, d_rgb, d_hits, d_ray_rgb, d_color, d_normal, out, d_out_count,
                           out_capacity_of(ld), ld.d_out_octants, d_counts);

    // the traversal variants of launch_level / launch_frame_lights_env: the same hit records from each of them
    const DeviceScene &ds = *ls.ds;
    return with_trace_variant(ds.n_planes || ds.n_spheres, ld.flags & MR_MATH_PRODUCT, ld.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        const auto kern = ld.children == MR_LEVEL_LAST ? &level_lights_kernel<VAR, 0> : &level_lights_kernel<VAR, 1>;
        return launch_traversal(kern, trace_grid(n), a.tp.stack_depth, stream, a);
    });
}

}  // namespace mr
