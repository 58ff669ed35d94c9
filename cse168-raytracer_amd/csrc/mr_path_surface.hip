// mr_path_surface.hip -- the PATH_TRACING generators on a scene with a texture table: mr_gen_path_rays_surface.
//
//   children_surf_kernel   children_kernel<true> (mr_bounce.hip) reading every hit's N and the diffuse child's colour from the
//                          surface pass's two per-ray buffers (mr_hit_surface, mr_procedural.hip) instead of computing the one
//                          and taking m_diffuse for the other: children_body<true, kColorSurface> (mr_children_body.h).  The
//                          kernel looks no texture up, so it runs on any scene, with a table or without; on a scene without one
//                          the buffers hold the object's normal and the material's colour, and the children are the plain
//                          kernel's bit for bit.
//
// The surface form of the non-path generators is mr_bump_surface.hip (mr_gen_secondary_rays_surface): they emit no diffuse child
// and read the normal buffer alone, for the mirror child of a STONE material with ks != 0 (a STONE material has kt = 0, and
// nothing bumps another material's normal).
//
// A unit of its own because the kernels of mr_bounce.hip are held to tests/golden/kernel_budget.json; this unit's record is
// kernel_budget_path_surface.json.  Compiled with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_children_body.h"
#include "mr_launch.h"

namespace mr {
namespace {

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(MIRO_CHILDREN_WAVES, 8))) void children_surf_kernel(BounceArgs a, const float *color,
                                                                                                                           const float *normal) {
    children_body<true, kColorSurface>(a, color, normal);
}

}  // namespace

mr_status launch_path_rays_surface(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                   const float *d_normal, const float *d_weights, const uint32_t *d_pixels, const uint32_t *d_ids,
                                   unsigned long long n, uint32_t spp, uint32_t seed, uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays,
                                   float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids, unsigned long long *d_count,
                                   unsigned long long out_capacity, uint8_t *d_out_octants, hipStream_t stream) {
    MR_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream));
    if (n == 0) return MR_OK;
    const BounceArgs a = path_args_of(ds, d_rays, d_hits, d_weights, d_pixels, d_ids, n, spp, seed, bounce, kinds, d_out_rays, d_out_weights,
                                      d_out_pixels, d_out_ids, d_count, out_capacity, d_out_octants);
    hipLaunchKernelGGL(children_surf_kernel, dim3(grid_for((n + kGenIter - 1) / kGenIter)), dim3(kBlock), 0, stream, a, d_color, d_normal);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
