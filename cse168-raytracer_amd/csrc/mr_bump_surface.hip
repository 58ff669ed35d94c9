// mr_bump_surface.hip -- the reflect / Fresnel / refract generators about the normal Scene::trace hands on:
// mr_gen_secondary_rays_surface (include/miro_hip_bump.h).
//
//   children_bump_kernel   children_kernel<false> (mr_bounce.hip) reading every listed hit's N from the surface pass's normal buffer
//                          (mr_hit_surface, mr_procedural.hip) instead of computing the object's own:
//                          children_body<false, kColorSurface> (mr_children_body.h).  Scene::trace bumps the normal of a hit on a
//                          STONE material (Scene.cpp:234-263) and Ray::reflect bounces about what it left (Ray.h:156), so the
//                          mirror child of a reflective stone floor needs this buffer.  Both passes of the body take N through
//                          child_normal, so the Fresnel decision of a refractive hit is the same bits in both.  No diffuse child
//                          exists without PATH, so the colour buffer is not an argument: the body's `color` is NULL and never read.
//                          The kernel looks no texture up and runs on any scene; where no STONE material reflects, the buffer
//                          holds the object's normal on every hit that has a child, and the children are mr_gen_secondary_rays'
//                          bit for bit.
//
// A unit of its own, beside mr_path_surface.hip, because the kernels of mr_bounce.hip are held to
// tests/golden/kernel_budget.json; this unit's record is kernel_budget_bump_surface.json.  The waves-per-SIMD request is
// children_kernel<false>'s.  Compiled with -ffp-contract=off like the rest of the library.
#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_children_body.h"
#include "mr_launch.h"

namespace mr {
namespace {

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 8))) void children_bump_kernel(BounceArgs a, const float *normal) {
    children_body<false, kColorSurface>(a, nullptr, normal);
}

}  // namespace

mr_status launch_secondary_rays_surface(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                                        const float *d_weights, const uint32_t *d_pixels, unsigned long long n, uint32_t spp,
                                        mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels, unsigned long long *d_count,
                                        unsigned long long out_capacity, uint8_t *d_out_octants, hipStream_t stream) {
    MR_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream));
    if (n == 0) return MR_OK;
    BounceArgs a;
    a.m = rec::mesh_of(ds); a.rays = d_rays; a.hits = d_hits; a.weights = d_weights; a.pixels = d_pixels; a.ids = nullptr;
    a.spp = spp; a.hbase = 0; a.bounce = 0; a.kinds = 0; a.n = n;
    a.out.rays = d_out_rays; a.out.weights = d_out_weights; a.out.pixels = d_out_pixels; a.out.ids = nullptr; a.out.count = d_count; a.out.capacity = out_capacity; a.out.octants = d_out_octants;
    hipLaunchKernelGGL(children_bump_kernel, dim3(grid_for((n + kGenIter - 1) / kGenIter)), dim3(kBlock), 0, stream, a, d_normal);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
