// mr_square_surface.hip -- Phong::shade over SquareLights on a scene with a texture table: mr_shade_square_lights_surface.
//
//   shade_square_lights_surf_kernel   shade_square_lights_kernel (mr_distribution.hip, where the loop is described) reading the
//                                     hit's diffuseColor and N from the surface pass's two per-ray buffers (mr_hit_surface,
//                                     mr_procedural.hip) instead of computing them: shade_square_lights_body<.., kColorSurface>
//                                     (mr_square_body.h).  The kernel looks no texture up, so it runs on any scene, with a table
//                                     or without; on a scene without one the buffers hold the material's colour and the object's
//                                     normal and the light is the plain kernel's.
//
// The shadow side is untouched: light_scale_of reads the occluder's own normal for a refractive occluder alone
// (Phong.cpp:102-109), a STONE material must have kt = 0 (ks is free) and so is never one, and nothing bumps a UVW material.
//
// A unit of its own because the kernel lists of mr_distribution.hip and mr_procedural.hip are held to their records
// (tests/golden/kernel_budget_distribution.json, kernel_budget_procedural.json); this unit's record is
// kernel_budget_square_surface.json.  Compiled with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_square_body.h"

namespace mr {
namespace {

template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void shade_square_lights_surf_kernel(SquareArgs a, const float *color,
                                                                                                                         const float *normal) {
    shade_square_lights_body<VAR, ANY, kColorSurface>(a, color, normal);
}

}  // namespace

mr_status launch_shade_square_lights_surface(const DeviceScene &ds, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t side,
                                             uint32_t seed, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                             const float *d_normal, const float *d_weights, const uint32_t *d_pixels, const float *d_uv_in,
                                             unsigned long long n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb,
                                             unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    const SquareArgs a = square_args_of(ds, lights, n_lights, side, seed, d_rays, d_hits, d_weights, d_pixels, d_uv_in, n, spp, d_rgb, d_ray_rgb, d_counts);
    return launch_square_variant(ds, flags, a, stream, [](auto var, auto any) {
        return &shade_square_lights_surf_kernel<decltype(var)::value, decltype(any)::value>;
    }, d_color, d_normal);
}

}  // namespace mr
