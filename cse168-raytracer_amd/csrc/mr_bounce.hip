// mr_bounce.hip -- specular secondary rays ("next" row f4 of SURVEY.md section 8): the recursion of
// Scene::traceScene (Scene.cpp:270-346) unrolled into wavefront bounces.
//   light_scale_kernel      what Phong::shade does with the shadow hit (Phong.cpp:97-113): opaque occluder -> 0,
//                           refractive occluder -> dot(N, l) (0 if negative or < epsilon), no occluder -> 1
//   shade_accumulate_kernel Phong::shade per ray with per-triangle materials, times the ray's path weight, added to
//                           its pixel (float atomics: the order of additions is not reproducible for multi-bounce
//                           frames; the single-bounce path of mr_shade_direct stays deterministic)
//   children_kernel         Ray::reflect / getReflectionCoefficient / refract (Ray.h:143-243) for every hit on a
//                           reflective or refractive material: up to three children per ray, each with
//                           weight * (specular | transmission*Rs | transmission*(1-Rs)) (Scene.cpp:302-336), written
//                           compacted by wave64 ballots + prefix sums (the body is mr_children_body.h)
#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_accumulate_body.h"
#include "mr_children_body.h"
#include "mr_launch.h"
#include "mr_phong.h"
#include "mr_recursion.h"

namespace mr {
namespace {

using namespace rec;

__global__ __launch_bounds__(kBlock) void light_scale_kernel(MeshMat m, const mr_ray *shadow_rays, const mr_hit *shadow_hits,
                                                             const uint32_t *src, const unsigned long long *count,
                                                             unsigned long long max_n, float *light_scale) {
    unsigned long long n = *count;
    if (n > max_n) n = max_n;
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        const float4 h = reinterpret_cast<const float4 *>(shadow_hits)[k];
        float scale = 1.0f;
        if (__float_as_uint(h.y) != MR_MISS)
            scale = light_scale_of(m, reinterpret_cast<const float4 *>(shadow_rays)[2 * k],
                                   reinterpret_cast<const float4 *>(shadow_rays)[2 * k + 1], h);
        light_scale[src[k]] = scale;
    }
}

// the body is shade_accumulate_body (mr_accumulate_body.h), which the textured form in mr_textures.hip and the surface-pass
// form in mr_procedural.hip share
__global__ __launch_bounds__(kBlock) void shade_accumulate_kernel(AccumArgs a) {
    shade_accumulate_body<kColorMaterial>(a, TexParams(), nullptr, nullptr);
}

// the body is children_body (mr_children_body.h, where the chunks, the list and the two passes are described), which the
// surface-pass form in mr_path_surface.hip shares
template <bool PATH>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(PATH ? MIRO_CHILDREN_WAVES : 1, 8))) void children_kernel(BounceArgs a) {
    children_body<PATH, kColorMaterial>(a, nullptr, nullptr);
}

}  // namespace

mr_status launch_light_scale(const DeviceScene &ds, const mr_ray *d_shadow_rays, const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src,
                             const unsigned long long *d_shadow_count, unsigned long long n, float *d_light_scale, hipStream_t stream) {
    if (n == 0) return MR_OK;
    hipLaunchKernelGGL(light_scale_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, mesh_of(ds), d_shadow_rays, d_shadow_hits,
                       d_shadow_src, d_shadow_count, n, d_light_scale);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_shade_accumulate(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                  const uint32_t *d_pixels, unsigned long long n, const mr_ray *d_shadow_rays,
                                  const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src,
                                  const unsigned long long *d_shadow_count, float *d_light_scale, const mr_light &light,
                                  uint32_t spp, float *d_rgb, const TexParams *tex, hipStream_t stream) {
    if (n == 0) return MR_OK;
    const mr_status st = launch_light_scale(ds, d_shadow_rays, d_shadow_hits, d_shadow_src, d_shadow_count, n, d_light_scale, stream);
    if (st != MR_OK) return st;
    if (tex) return launch_shade_accumulate_tex(ds, *tex, d_rays, d_hits, d_weights, d_pixels, n, d_light_scale, light, spp, d_rgb, stream);
    const AccumArgs a = accum_args_of(ds, d_rays, d_hits, d_weights, d_pixels, n, d_light_scale, light, spp, d_rgb);
    hipLaunchKernelGGL(shade_accumulate_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_secondary_rays(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                const uint32_t *d_pixels, unsigned long long n, uint32_t spp, mr_ray *d_out_rays,
                                float *d_out_weights, uint32_t *d_out_pixels, unsigned long long *d_count,
                                unsigned long long out_capacity, uint8_t *d_out_octants, hipStream_t stream) {
    MR_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream));
    if (n == 0) return MR_OK;
    BounceArgs a;
    a.m = mesh_of(ds); a.rays = d_rays; a.hits = d_hits; a.weights = d_weights; a.pixels = d_pixels; a.ids = nullptr;
    a.spp = spp; a.hbase = 0; a.bounce = 0; a.kinds = 0; a.n = n;
    a.out.rays = d_out_rays; a.out.weights = d_out_weights; a.out.pixels = d_out_pixels; a.out.ids = nullptr; a.out.count = d_count; a.out.capacity = out_capacity; a.out.octants = d_out_octants;
    hipLaunchKernelGGL(children_kernel<false>, dim3(grid_for((n + kGenIter - 1) / kGenIter)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_path_rays(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                           const uint32_t *d_pixels, const uint32_t *d_ids, unsigned long long n, uint32_t spp, uint32_t seed,
                           uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                           uint32_t *d_out_ids, unsigned long long *d_count, unsigned long long out_capacity, uint8_t *d_out_octants, hipStream_t stream) {
    MR_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream));
    if (n == 0) return MR_OK;
    const BounceArgs a = path_args_of(ds, d_rays, d_hits, d_weights, d_pixels, d_ids, n, spp, seed, bounce, kinds, d_out_rays, d_out_weights,
                                      d_out_pixels, d_out_ids, d_count, out_capacity, d_out_octants);
    hipLaunchKernelGGL(children_kernel<true>, dim3(grid_for((n + kGenIter - 1) / kGenIter)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
