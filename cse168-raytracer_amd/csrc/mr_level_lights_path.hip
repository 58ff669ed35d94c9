// mr_level_lights_path.hip -- ONE level of Scene::traceScene's recursion (Scene.cpp:270-346) of a PATH_TRACING build for a queue of
// rays in ONE launch on ANY scene (mr_trace_level_lights_path).  The kernel is level_lights_body<VAR, CHILDREN, true>
// (mr_level_lights_body.h), mr_level_lights.hip's per-ray sequence with two steps of its own:
//
//   a ray that leaves the scene reads getEnvironmentMap(ray) from the FULL image or, for a ray made by Ray::random (ray.isDiffuse,
//   Scene.cpp:678-681), from its 24-texel-wide low-res copy (env_lookup, mr_children_col.h)
//
//   the children are those of mr_gen_path_rays_surface in place of those of mr_gen_secondary_rays: the PATH_TRACING build of
//   Ray::reflect / getReflectionCoefficient / refract (Ray.h:149-158, 235-239) plus Ray::random's diffuse bounce (Ray.h:124-140),
//   every one of them about the normal Scene::trace hands on -- the BUMPED one on stone -- and the diffuse child with weight x
//   diffuseColor, the looked-up colour (write_children_col, mr_children_col.h: the frame that emits level 1 ends in the same step)
//
// The batched route runs such a level as five launches,
//   mr_trace -> mr_shade_environment -> mr_hit_surface -> mr_shade_lights_surface -> mr_gen_path_rays_surface;
// the children are the same set with the same ids (tests/test_level_lights_path.py compares level by level on the same queues).
//
// The queue carries what the path tracer's queues carry: stable ray ids (d_ids, NULL: the ray's index), from which a child's
// random numbers and its own id derive (rec::ChildGen<true>, rec::child_id), and one byte per ray that says whether Ray::random
// made it (d_lowres, or MR_ENV_LOWRES for the whole queue).  The kernel that generates the children knows each child's kind, so
// it writes that byte for the next level (d_out_lowres: 1 for kind 3): a diffuse bounce next to a refraction under an
// environment image, which the batched driver has to refuse, works here.
//
// The low-res copy (at most 24 x 96 texels) is read from global memory, not staged in LDS as shade_environment_kernel does: a
// miss of a diffuse ray fetches four 16-byte records of an image that stays in the L2, and the workgroup's LDS remains the
// traversal stack's.  The texels, and so the values, are the same either way (env_texels / env_blend on env.low with lw x lh).
// The two masks are wave-uniform runtime branches, as the environment and the texture table are.
//
// Diffuse bounce queues in open scenes hit rarely, which is where the body's remark on what a fused level does NOT buy weighs
// most.  Times against the batched route: DESIGN section 5c, profiles/level_lights_path_ab.log.
//
// Live state, besides what the body lists: unlike the specular form, which recomputes the object's own normal for its children,
// this form keeps the bumped normal and the colour across the light loop: six values.  Four waves per SIMD, as level_lights_kernel.
// d_out_count is zeroed by mr_level_lights.hip's one-word kernel (launch_zero_count), not a memset node.
#include <hip/hip_runtime.h>

#include "mr_level_lights_body.h"

namespace mr {
namespace {

#ifndef MIRO_LEVEL_LIGHTS_PATH_WAVES
#define MIRO_LEVEL_LIGHTS_PATH_WAVES 4
#endif

// VAR: the traversal variant of trace_ray (mr_traverse.h) for the ray and its shadow rays; CHILDREN: 0 none, 1 path tracing.
// The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, int CHILDREN>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_LEVEL_LIGHTS_PATH_WAVES, 8))) void level_lights_path_kernel(
    const LevelLightsPathArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    level_lights_body<VAR, CHILDREN, true>(a, s_stack, s_tab);
}

}  // namespace

mr_status launch_level_lights_path(const LightScene &ls, const mr_level_lights_path_desc &ld, const mr_ray *d_rays, const float *d_weights,
                                   const uint32_t *d_pixels, const uint32_t *d_ids, unsigned long long n, float *d_rgb, mr_hit *d_hits,
                                   float *d_ray_rgb, float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights,
                                   uint32_t *d_out_pixels, uint32_t *d_out_ids, unsigned long long *d_out_count,
                                   unsigned long long *d_counts, hipStream_t stream) {
    if (ld.children != MR_LEVEL_LAST) {
        const mr_status zs = launch_zero_count(d_out_count, stream);
        if (zs != MR_OK) return zs;
    }
    if (n == 0) return MR_OK;
    LevelLightsPathArgs a;
    const RayQueue in = {const_cast<mr_ray *>(d_rays), const_cast<float *>(d_weights), const_cast<uint32_t *>(d_pixels), nullptr, nullptr};   // only read
    const RayQueue out = {d_out_rays, d_out_weights, d_out_pixels, d_out_ids, nullptr};
    fill_level_lights_args(a, ls, ld.spp, ld.environment, in, n, d_rgb, d_hits, d_ray_rgb, d_color, d_normal, out, d_out_count,
                           out_capacity_of(ld), ld.d_out_octants, d_counts);
    fill_level_lights_path_args(a, d_ids, ld.d_lowres, ld.flags, ld.seed, ld.bounce, ld.path_kinds, ld.d_out_lowres);

    // the traversal variants of launch_level_lights: the same hit records from each of them
    const DeviceScene &ds = *ls.ds;
    return with_trace_variant(ds.n_planes || ds.n_spheres, ld.flags & MR_MATH_PRODUCT, ld.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        const auto kern = ld.children == MR_LEVEL_LAST ? &level_lights_path_kernel<VAR, 0> : &level_lights_path_kernel<VAR, 1>;
        return launch_traversal(kern, trace_grid(n), a.tp.stack_depth, stream, a);
    });
}

}  // namespace mr
