// mr_lights_body.h -- the body of shade_lights_kernel (mr_lights.hip, where the kernel is described) as a __device__
// template, so that its textured form (mr_textures.hip) and its surface-pass form (mr_procedural.hip) are the same code with
// one more step.  SRC (ColorSource, mr_texture.h) says where the hit's diffuseColor comes from:
//   kColorMaterial  the material's own m_diffuse, read where it is used
//   kColorTexture   looked up once per hit, before the light loop, as Phong.cpp:51-56 does (diffuse_color_of)
//   kColorSurface   loaded from the surface pass's colour buffer, and the hit's N from its normal buffer (Scene.cpp:234-263)
// The last two keep the colour (three registers) across the shadow traversals.  The arguments are taken BY VALUE: through a
// reference to the kernel's argument block the same body compiles to other register and scratch figures.  Measured when
// kColorSurface joined the other two (hipcc, gfx950, the Makefile's flags): a source leaves the code of the other sources'
// kernels alone -- the device assembly of mr_lights.hip, mr_textures.hip and mr_bounce.hip did not change by an instruction.
// The three forms fill their arguments with lights_args_of below and launch with launch_traversal (mr_launch.h).  Included by the .hip units that instantiate it (everything
// here is local to its unit).
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_phong.h"
#include "mr_recursion.h"
#include "mr_texture.h"
#include "mr_traverse.h"
#include "mr_uv.h"

namespace mr {
namespace {

// what every light-list kernel takes besides its lights: the scene, the batch of traced rays and where the light goes
struct ShadeArgs {
    TraceParams tp;              // scene arrays, root box; tp.rays = the batch, tp.n its length
    rec::MeshMat m;
    const mr_hit *hits;
    const float *weights;        // rgb per ray or NULL (= 1)
    const uint32_t *pixels;      // pixel per ray or NULL (= ray index / spp)
    uint32_t spp, n_lights;
    float inv_spp;
    float *rgb;                  // may be NULL (then ray_rgb is not)
    float *ray_rgb;              // may be NULL: the un-weighted L of every ray
    unsigned long long *counts;  // optional: [0] += shadow rays traced
};
// fills these fields of a kernel's argument block: a ShadeArgs, or a block that carries the same fields itself (SquareArgs)
template <typename A>
inline void fill_shade_args(A &a, const DeviceScene &ds, uint32_t n_lights, const mr_ray *d_rays, const mr_hit *d_hits,
                            const float *d_weights, const uint32_t *d_pixels, unsigned long long n, uint32_t spp, float *d_rgb,
                            float *d_ray_rgb, unsigned long long *d_counts) {
    a.tp = scene_trace_params(ds);
    a.tp.rays = d_rays; a.tp.n = n;
    a.m = rec::mesh_of(ds);
    a.hits = d_hits; a.weights = d_weights; a.pixels = d_pixels;
    a.spp = spp; a.n_lights = n_lights; a.inv_spp = 1.0f / (float)spp;
    a.rgb = d_rgb; a.ray_rgb = d_ray_rgb; a.counts = d_counts;
}

// The parts of a light-list kernel around its loop over the lights.  The loop of the fused kernels is shade_light_list
// (mr_light_loop.h); shade_lights_body below keeps the same statements written out, on a measurement: through that function
// the kernels of mr_lights.hip were slower than before by more than the run-to-run spread on the sponza stand-in (up to 0.5 %,
// profiles/light_loop_ab.log).  A change to one copy goes into the other; tests/test_lights_fuzz.py and the
// parity tests hold the two to the same bits.  A: ShadeArgs, or a block with the same fields.
// ray k's hit record: a miss for a lane past the end of the batch
template <typename A>
__device__ __forceinline__ float4 hit_record_of(const A &a, unsigned long long k, bool live) {
    float4 h = make_float4(0.f, __uint_as_float(MR_MISS), 0.f, 0.f);
    if (live) h = reinterpret_cast<const float4 *>(a.hits)[k];
    return h;
}
// for a hit: the point P, the normal N, the direction d of the ray that produced it and its material record
template <typename A>
__device__ __forceinline__ void shade_point_of(const A &a, unsigned long long k, const float4 h, float P[3], float N[3], float d[3],
                                               const float *&mt) {
    rec::surface_point(a.m, a.tp.rays, k, h, P, N);
    const float4 rb = reinterpret_cast<const float4 *>(a.tp.rays)[2 * k + 1];
    d[0] = rb.x; d[1] = rb.y; d[2] = rb.z;
    mt = rec::material_of(a.m, __float_as_uint(h.y));
}
// the ray's L to d_ray_rgb, and weight * L / spp to its pixel.  Called by all lanes of the wave (accumulate_runs).
// One product per ray, hit or miss, as the level kernels form it (mr_level_lights_body.h): Scene::traceScene answers true for a
// ray that leaves the scene (Scene.cpp:338-342), so the parent adds weight * m_bgColor = weight * 0 (Scene.cpp:309, 325, 334),
// which is NaN for a weight that is not finite -- the weight of a child made at a hit whose normal is NaN.  For a finite weight
// the product is a zero, which accumulate_runs does not add.  L is 0 for a ray that missed.
template <typename A>
__device__ __forceinline__ void store_shaded(const A &a, unsigned long long k, bool live, const float L[3]) {
    if (a.ray_rgb && live) { a.ray_rgb[3 * k] = L[0]; a.ray_rgb[3 * k + 1] = L[1]; a.ray_rgb[3 * k + 2] = L[2]; }
    if (a.rgb) {                                                       // wave-uniform
        uint32_t pix = 0xFFFFFFFFu;
        float v[3] = {0.f, 0.f, 0.f};
        if (live) {
            pix = rec::pixel_of(a.pixels, k, a.spp);
            float w[3];
            rec::weight_of(a.weights, k, w);
            for (int c = 0; c < 3; c++) v[c] = L[c] * w[c] * a.inv_spp;
        }
        rec::accumulate_runs(a.rgb, pix, v[0], v[1], v[2]);
    }
}

struct LightsArgs {
    ShadeArgs s;
    ShadeLight lights[MR_MAX_LIGHTS];
};

// t: read by kColorTexture only; color, normal: three floats per ray each, read by kColorSurface only
template <int VAR, bool ANY, int SRC>
__device__ __forceinline__ void shade_lights_body(const LightsArgs a, const TexParams t, const float *color, const float *normal) {
    using namespace rec;
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    const int tid = threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTraceBlock;
    const unsigned long long n = a.s.tp.n;
    const unsigned long long n_round = whole_workgroups(n);
    Stats st = {0ull, 0ull};
    unsigned my_shadow_rays = 0;

    for (unsigned long long k = (unsigned long long)xcd_block_id() * kTraceBlock + tid; k < n_round; k += stride) {
        const bool live = k < n;
        const float4 h = hit_record_of(a.s, k, live);
        const bool hit = __float_as_uint(h.y) != MR_MISS;              // a miss keeps L = 0 (m_bgColor); store_shaded forms weight * 0
        float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 1.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
        const float *mt = a.s.m.mats;
        float col[3] = {0.f, 0.f, 0.f};                                // diffuseColor, unless the material's own
        if (hit) {
            shade_point_of(a.s, k, h, P, N, d, mt);
            if (SRC == kColorTexture) diffuse_color_of(a.s.m, t, material_id(a.s.m.s, a.s.m.prim_mat, __float_as_uint(h.y)), __float_as_uint(h.y), P, col);
            if (SRC == kColorSurface)
                for (int c = 0; c < 3; c++) { col[c] = color[3 * k + c]; N[c] = normal[3 * k + c]; }
            my_shadow_rays += a.s.n_lights;
        }
        const float *dc = SRC == kColorMaterial ? mt : col;

        float L[3] = {0.f, 0.f, 0.f};
        for (uint32_t li = 0; li < a.s.n_lights; li++) {               // Phong.cpp:63, wave-uniform
            const ShadeLight &lt = a.lights[li];
            float4 sh;
            {
                float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(1.f, 1.f, 1.f, -1.f);
                if (hit) shadow_ray_for(lt, P, sa, sb);
                const mr_hit hs = trace_hit<true, ANY, false, VAR>(a.s.tp, sa, sb, sb.w, hit, s_stack, tid, st);
                sh = *reinterpret_cast<const float4 *>(&hs);
            }
            if (hit) {
                float4 sa, sb;
                shadow_ray_for(lt, P, sa, sb);                         // rebuilt rather than kept across the traversal
                const float scale = light_scale_of(a.s.m, sa, sb, sh);
                float diffuse[3] = {0.f, 0.f, 0.f}, highlight = 0.0f, out[3] = {0.f, 0.f, 0.f};
                bool lit = scale != 0.0f;                              // Phong.cpp:100-111: the light is skipped
                if (lit) {
                    if (lt.kind == MR_LIGHT_DISC) {
                        const float l[3] = {sb.x, sb.y, sb.z};
                        lit = disc_terms(lt, mt, dc, P, N, l, d[0], d[1], d[2], diffuse, highlight);
                    } else {
                        phong_terms(lt.position, lt.color, lt.wattage, mt, dc, P, N, d[0], d[1], d[2], diffuse, highlight);
                    }
                }
                if (lit) phong_combine(diffuse, highlight, scale, out);
                L[0] += out[0]; L[1] += out[1]; L[2] += out[2];
            }
        }
        store_shaded(a.s, k, live, L);
    }

    if (a.s.counts) workgroup_add<kTraceBlock>(my_shadow_rays, &a.s.counts[0]);
}

// what launch_shade_lights and its textured and surface-pass forms fill in the same way
inline LightsArgs lights_args_of(const DeviceScene &ds, const ShadeLight *lights, uint32_t n_lights, const mr_ray *d_rays,
                                 const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels, unsigned long long n,
                                 uint32_t spp, float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts) {
    LightsArgs a;
    fill_shade_args(a.s, ds, n_lights, d_rays, d_hits, d_weights, d_pixels, n, spp, d_rgb, d_ray_rgb, d_counts);
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) a.lights[i] = lights[i < n_lights ? i : 0];
    return a;
}

}  // namespace
}  // namespace mr
