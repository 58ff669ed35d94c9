// mr_procedural.hip -- the reference's procedural textures and the bump mapping of Scene::trace: StemTexture::lookup2D
// (Texture.h:192-212), StoneTexture::lookup2D and ::bumpHeight2D (Texture.cpp:358-440) over the noise of mr_noise.h, and the
// normal as Scene.cpp:234-263 leaves it.
//
//   hit_surface_kernel             per hit of a traced batch: diffuseColor (Phong.cpp:51-56) and the bumped, normalised normal,
//                                  into two per-ray buffers of three floats each (mr_hit_surface).  The one surface pass: every
//                                  scene, all seven texture kinds in any mixture or no table at all; the per-hit step is
//                                  hit_color_normal (mr_hit_surface_body.h), which the photon walk on textured scenes calls too
//   shade_lights_surf_kernel       shade_lights_kernel (mr_lights.hip) reading that colour and normal instead of computing
//                                  them: shade_lights_body<.., kColorSurface>
//   shade_accumulate_surf_kernel   shade_accumulate_kernel (mr_bounce.hip), the same way: shade_accumulate_body<kColorSurface>
//   texture_lookup_proc_kernel     lookup2D of a STONE / STEM texture for a batch of coordinates (mr_texture_lookup)
//   texture_lookup3_kernel         lookup3D of one UVW texture (PETAL, LEAF, FLOWER_CENTER) for a batch of points
//                                  (mr_texture_lookup3): the UVW inspection kernel lives here with the pass that serves its kinds
//   bump_height_kernel             bumpHeight2D of one texture for a batch of coordinates (mr_texture_bump_height)
//   noise_probe_kernel             PerlinNoise::noise / WorleyNoise::noise2D of order 3 themselves (mr_noise_probe)
//
// The lookups and the bump themselves are the device functions of mr_procedural_body.h, the UVW arms those of mr_solid_body.h.
//
// Why a pass of its own: a stone hit costs five three-point Worley searches and up to 5 + 4 * 7 Perlin evaluations.  The
// textured light-list kernel already spills in its worst variant; the surface pass has no traversal, so it
// keeps everything in registers, and the shading kernels that follow it are the light-list and accumulate kernels with two
// loads in place of the normal and the colour: the shared bodies of mr_lights_body.h / mr_accumulate_body.h with the
// kColorSurface source.
//
// powf and exp are the double series of miro_math.h rounded once (mm_powf, mm_exp); the reference calls libm's, which a
// host restatement can call too -- tests/test_procedural.py measures the distance.  pow(f1f0, 2) (Texture.cpp:424) is
// std::pow(float, int) of the C++03 library the reference was written for, which returns float (only then does the std::min
// next to it compile): the float product f1f0 * f1f0.
#include <hip/hip_runtime.h>

#include "mr_accumulate_body.h"
#include "mr_hit_surface_body.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_lights_body.h"
#include "mr_noise.h"
#include "mr_procedural_body.h"
#include "mr_solid_body.h"
#include "mr_texture.h"

namespace mr {
namespace {

struct SurfaceArgs {
    rec::MeshMat m;
    TexParams t;                 // recs / mat_tex nullptr: the scene has no texture table
    const mr_ray *rays;
    const mr_hit *hits;
    unsigned long long n;
    float *color, *normal;       // three floats per ray each; a ray that missed keeps what the buffers held
    unsigned long long *counts;  // optional: [0] += lookups the reference leaves undefined
};

__global__ __launch_bounds__(kBlock) void hit_surface_kernel(SurfaceArgs a) {
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_undefined = 0;
    // hit_color_normal's test of mat_tex, taken out of the loop: a scene without a texture table runs a call that is compiled
    // knowing it, the plain arm alone (measured: DESIGN section 4)
    const bool table = a.t.mat_tex != nullptr;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < a.n; k += stride) {
        const float4 h = reinterpret_cast<const float4 *>(a.hits)[k];
        const uint32_t prim = __float_as_uint(h.y);
        if (prim == MR_MISS) continue;
        float P[3], N[3], col[3];
        surface<true>(a.m.s, a.rays, k, h.x, prim, h.z, h.w, P, N);
        bool ok = true;
        if (table) {
            hit_color_normal(a.m, a.t, nt, prim, P, N, col, ok);
        } else {
            TexParams t0 = a.t;
            t0.mat_tex = nullptr;
            hit_color_normal(a.m, t0, nt, prim, P, N, col, ok);
        }
        if (!ok) my_undefined++;
        a.color[3 * k] = col[0]; a.color[3 * k + 1] = col[1]; a.color[3 * k + 2] = col[2];
        a.normal[3 * k] = N[0]; a.normal[3 * k + 1] = N[1]; a.normal[3 * k + 2] = N[2];
    }
    if (a.counts) workgroup_add<kBlock>(my_undefined, &a.counts[0]);
}

__global__ __launch_bounds__(kBlock) void texture_lookup_proc_kernel(TexParams t, uint32_t id, const float *uv, unsigned long long n,
                                                                     float *rgb, unsigned long long *counts) {
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const bool stem = __float_as_uint(t.recs[3 * (size_t)id].x) == kTexStem;
    const float scale = t.recs[3 * (size_t)id + 1].w;
    unsigned my_undefined = 0;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        float c[3];
        bool ok = true;
        if (stem) stem_color(nt, scale, uv[2 * k], uv[2 * k + 1], c, ok);
        else stone_color(nt, scale, uv[2 * k], uv[2 * k + 1], c, ok);
        if (!ok) my_undefined++;
        rgb[3 * k] = c[0]; rgb[3 * k + 1] = c[1]; rgb[3 * k + 2] = c[2];
    }
    if (counts) workgroup_add<kBlock>(my_undefined, &counts[0]);
}

// coords: optional, written for a PETAL alone
__global__ __launch_bounds__(kBlock) void texture_lookup3_kernel(TexParams t, uint32_t id, const float *p, unsigned long long n, float *rgb,
                                                                 float *coords, unsigned long long *counts) {
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const uint32_t kind = __float_as_uint(t.recs[3 * (size_t)id].x);
    const float4 q1 = t.recs[3 * (size_t)id + 1], q2 = t.recs[3 * (size_t)id + 2];
    unsigned my_undefined = 0;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        const float P[3] = {p[3 * k], p[3 * k + 1], p[3 * k + 2]};
        float c[3], crd[3];
        bool ok = true;
        solid_color(nt, kind, q1, q2, P, c, crd, ok);
        if (!ok) my_undefined++;
        rgb[3 * k] = c[0]; rgb[3 * k + 1] = c[1]; rgb[3 * k + 2] = c[2];
        if (coords && kind == kTexPetal) { coords[3 * k] = crd[0]; coords[3 * k + 1] = crd[1]; coords[3 * k + 2] = crd[2]; }
    }
    if (counts) workgroup_add<kBlock>(my_undefined, &counts[0]);
}

// stone: the texture is a StoneTexture; every other kind's bumpHeight2D is 0 (Texture.h:63,191)
__global__ __launch_bounds__(kBlock) void bump_height_kernel(bool stone, float scale, const float *uv, unsigned long long n, float *height) {
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        bool ok = true;
        height[k] = stone ? stone_height(nt, scale, uv[2 * k], uv[2 * k + 1], ok) : 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void noise_probe_kernel(uint32_t which, const float *in, unsigned long long n, float *out) {
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        bool ok = true;
        if (which == MR_NOISE_PERLIN) {
            out[k] = perlin_noise(nt, in[3 * k], in[3 * k + 1], in[3 * k + 2], ok);
        } else {
            const Worley3 w = worley2(nt, in[2 * k], in[2 * k + 1], ok);
            float *o = out + 6 * k;
            o[0] = w.F0; o[1] = w.F1; o[2] = w.F2;
            o[3] = __uint_as_float(w.I0); o[4] = __uint_as_float(w.I1); o[5] = __uint_as_float(w.I2);
        }
    }
}

// shade_lights_body (mr_lights_body.h) and shade_accumulate_body (mr_accumulate_body.h) with the hit's diffuseColor and N read
// from the surface pass's buffers
template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void shade_lights_surf_kernel(LightsArgs a, const float *color,
                                                                                                                  const float *normal) {
    shade_lights_body<VAR, ANY, kColorSurface>(a, TexParams(), color, normal);
}

__global__ __launch_bounds__(kBlock) void shade_accumulate_surf_kernel(AccumArgs a, const float *color, const float *normal) {
    shade_accumulate_body<kColorSurface>(a, TexParams(), color, normal);
}

}  // namespace

mr_status launch_hit_surface(const DeviceScene &ds, const TexParams &tex, const mr_ray *d_rays, const mr_hit *d_hits, unsigned long long n,
                             float *d_color, float *d_normal, unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    if ((ds.spheres || ds.planes) && !d_rays)
        return fail(MR_ERR_INVALID, "the scene holds spheres / planes: their hit point is o + t*d, d_rays is required");
    SurfaceArgs a;
    a.m = rec::mesh_of(ds); a.t = tex; a.rays = d_rays; a.hits = d_hits; a.n = n; a.color = d_color; a.normal = d_normal; a.counts = d_counts;
    hipLaunchKernelGGL(hit_surface_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_shade_lights_surf(const DeviceScene &ds, const ShadeLight *lights, uint32_t n_lights, const mr_ray *d_rays,
                                   const mr_hit *d_hits, const float *d_color, const float *d_normal, const float *d_weights,
                                   const uint32_t *d_pixels, unsigned long long n, uint32_t spp, uint32_t flags, float *d_rgb,
                                   float *d_ray_rgb, unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    const LightsArgs a = lights_args_of(ds, lights, n_lights, d_rays, d_hits, d_weights, d_pixels, n, spp, d_rgb, d_ray_rgb, d_counts);
    const bool any = flags & MR_TRACE_ANY;
    return with_trace_variant(ds.n_planes || ds.n_spheres, flags & MR_MATH_PRODUCT, flags & MR_TRACE_INCOHERENT, [&](auto var) {
        constexpr int VAR = decltype(var)::value;
        return launch_traversal(any ? &shade_lights_surf_kernel<VAR, true> : &shade_lights_surf_kernel<VAR, false>, trace_grid(n), a.s.tp.stack_depth, stream, a,
                                d_color, d_normal);
    });
}

mr_status launch_shade_accumulate_surf(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                       const float *d_normal, const float *d_weights, const uint32_t *d_pixels, unsigned long long n,
                                       const float *d_light_scale, const mr_light &light, uint32_t spp, float *d_rgb, hipStream_t stream) {
    if (n == 0) return MR_OK;
    const AccumArgs a = accum_args_of(ds, d_rays, d_hits, d_weights, d_pixels, n, d_light_scale, light, spp, d_rgb);
    hipLaunchKernelGGL(shade_accumulate_surf_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, a, d_color, d_normal);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_texture_lookup_proc(const TexParams &tex, uint32_t texture, const float *d_uv, unsigned long long n, float *d_rgb,
                                     unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    hipLaunchKernelGGL(texture_lookup_proc_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, tex, texture, d_uv, n, d_rgb, d_counts);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_texture_lookup3(const TexParams &tex, uint32_t texture, const float *d_p, unsigned long long n, float *d_rgb,
                                 float *d_coords, unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    hipLaunchKernelGGL(texture_lookup3_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, tex, texture, d_p, n, d_rgb, d_coords, d_counts);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_bump_height(bool stone, float scale, const float *d_uv, unsigned long long n, float *d_height, hipStream_t stream) {
    if (n == 0) return MR_OK;
    hipLaunchKernelGGL(bump_height_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, stone, scale, d_uv, n, d_height);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_noise_probe(uint32_t which, const float *d_in, unsigned long long n, float *d_out, hipStream_t stream) {
    if (n == 0) return MR_OK;
    hipLaunchKernelGGL(noise_probe_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, which, d_in, n, d_out);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
