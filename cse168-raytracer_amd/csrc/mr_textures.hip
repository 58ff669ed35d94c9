// mr_textures.hip -- TexturedPhong materials (Texture.cpp:509-527): the diffuse colour of a hit looked up in a 2-D texture
// at the object's UV coordinates (Phong.cpp:51-56 -> Texture::lookup2D -> Object::toUVCoordinates(hit.P)).
//
//   hit_uv_kernel                 toUVCoordinates(hit.P) of every ray of a traced batch (mr_hit_uv; mr_uv.h)
//   texture_lookup_kernel         Texture::lookup2D of one texture for a batch of coordinates (mr_texture_lookup; mr_texture.h)
//   shade_lights_tex_kernel       shade_lights_kernel (mr_lights.hip) with the lookup: shade_lights_body<.., kColorTexture>
//   shade_accumulate_tex_kernel   shade_accumulate_kernel (mr_bounce.hip) with the lookup: shade_accumulate_body<kColorTexture>
//
// The two shading kernels are chosen by the host when the scene has a texture table (mr_scene_set_textures); a scene without
// one runs the untextured kernels under their own names.  A lane finds its material's texture id in the table's per-material
// array, computes (u, v) from the hit point it has rebuilt anyway, and fetches: one 48-byte table record (three dwordx4), and
// for an image four 16-byte texels at unrelated addresses -- vector loads throughout, because neighbouring lanes hit different
// materials and different texels; nothing is staged in LDS (an image does not fit, and a lane reads four texels of it once).
// The light-list kernel does this once per hit, before the light loop, and carries the colour (three registers) across its
// shadow traversals rather than (u, v) and a second lookup per light.
#include <hip/hip_runtime.h>

#include "mr_accumulate_body.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_lights_body.h"
#include "mr_texture.h"
#include "mr_uv.h"

namespace mr {
namespace {

__global__ __launch_bounds__(kBlock) void hit_uv_kernel(UvPtrs m, const mr_ray *rays, const mr_hit *hits, unsigned long long n, float *uv) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        const float4 h = reinterpret_cast<const float4 *>(hits)[k];
        const uint32_t prim = __float_as_uint(h.y);
        float u = 0.f, v = 0.f;
        if (prim != MR_MISS) {
            float P[3], N[3];
            surface<false>(m.s, rays, k, h.x, prim, h.z, h.w, P, N);
            uv_of(m, prim, P, u, v);
        }
        uv[2 * k] = u; uv[2 * k + 1] = v;
    }
}

__global__ __launch_bounds__(kBlock) void texture_lookup_kernel(TexParams t, uint32_t id, const float *uv, unsigned long long n,
                                                                float *rgb, unsigned long long *counts) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_undefined = 0;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        float c[3];
        if (!texture_color(t, id, uv[2 * k], uv[2 * k + 1], c)) my_undefined++;
        rgb[3 * k] = c[0]; rgb[3 * k + 1] = c[1]; rgb[3 * k + 2] = c[2];
    }
    if (counts) workgroup_add<kBlock>(my_undefined, &counts[0]);
}

template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void shade_lights_tex_kernel(LightsArgs a, TexParams t) {
    shade_lights_body<VAR, ANY, kColorTexture>(a, t, nullptr, nullptr);
}

__global__ __launch_bounds__(kBlock) void shade_accumulate_tex_kernel(AccumArgs a, TexParams t) {
    shade_accumulate_body<kColorTexture>(a, t, nullptr, nullptr);
}

}  // namespace

mr_status launch_shade_lights_tex(const DeviceScene &ds, const TexParams &tex, const ShadeLight *lights, uint32_t n_lights,
                                  const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels,
                                  unsigned long long n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb,
                                  unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    const LightsArgs a = lights_args_of(ds, lights, n_lights, d_rays, d_hits, d_weights, d_pixels, n, spp, d_rgb, d_ray_rgb, d_counts);
    const bool any = flags & MR_TRACE_ANY;
    return with_trace_variant(ds.n_planes || ds.n_spheres, flags & MR_MATH_PRODUCT, flags & MR_TRACE_INCOHERENT, [&](auto var) {
        constexpr int VAR = decltype(var)::value;
        return launch_traversal(any ? &shade_lights_tex_kernel<VAR, true> : &shade_lights_tex_kernel<VAR, false>, trace_grid(n), a.s.tp.stack_depth, stream, a, tex);
    });
}

mr_status launch_shade_accumulate_tex(const DeviceScene &ds, const TexParams &tex, const mr_ray *d_rays, const mr_hit *d_hits,
                                      const float *d_weights, const uint32_t *d_pixels, unsigned long long n,
                                      const float *d_light_scale, const mr_light &light, uint32_t spp, float *d_rgb,
                                      hipStream_t stream) {
    if (n == 0) return MR_OK;
    const AccumArgs a = accum_args_of(ds, d_rays, d_hits, d_weights, d_pixels, n, d_light_scale, light, spp, d_rgb);
    hipLaunchKernelGGL(shade_accumulate_tex_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, a, tex);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_hit_uv(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, unsigned long long n, float *d_uv,
                        hipStream_t stream) {
    if (n == 0) return MR_OK;
    if ((ds.spheres || ds.planes) && !d_rays)
        return fail(MR_ERR_INVALID, "the scene holds spheres / planes: their hit point is o + t*d, d_rays is required");
    hipLaunchKernelGGL(hit_uv_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, uv_ptrs(ds), d_rays, d_hits, n, d_uv);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_texture_lookup(const TexParams &tex, uint32_t texture, const float *d_uv, unsigned long long n, float *d_rgb,
                                unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    hipLaunchKernelGGL(texture_lookup_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, tex, texture, d_uv, n, d_rgb, d_counts);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
