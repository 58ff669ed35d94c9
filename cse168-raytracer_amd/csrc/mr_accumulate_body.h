// mr_accumulate_body.h -- the body of shade_accumulate_kernel (mr_bounce.hip, where the kernel is described) as a
// __device__ template: its textured form (mr_textures.hip) is the same code with the hit's diffuseColor looked up first
// (Phong.cpp:51-56; diffuse_color_of), its surface-pass form (mr_procedural.hip) the same code with the colour and the normal
// loaded from the pass's two buffers.  SRC is the ColorSource of mr_texture.h, and the arguments are taken by value, as in
// mr_lights_body.h.  Every source calls surface_point: the surface-pass form needs P alone, but P is the same fp32 operations
// in the same order whether surface_od is asked for N or not (no contraction in these units), and the N it would compute is
// overwritten from the buffer before anything reads it, so no code is generated for it.  Included by the .hip units that
// instantiate it (everything here is local to its unit).
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_phong.h"
#include "mr_recursion.h"
#include "mr_texture.h"
#include "mr_uv.h"

namespace mr {
namespace {

struct AccumArgs {
    rec::MeshMat m;
    const mr_ray *rays;
    const mr_hit *hits;
    const float *weights;         // rgb per ray or NULL (= 1)
    const uint32_t *pixels;       // pixel per ray or NULL (= ray index / spp)
    const float *light_scale;     // per ray
    LightArgs lt;
    float inv_spp;
    uint32_t spp;
    unsigned long long n;
    float *rgb;
};

// what launch_shade_accumulate and its textured and surface-pass forms fill in the same way
inline AccumArgs accum_args_of(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                               const uint32_t *d_pixels, unsigned long long n, const float *d_light_scale, const mr_light &light,
                               uint32_t spp, float *d_rgb) {
    AccumArgs a;
    a.m = rec::mesh_of(ds); a.rays = d_rays; a.hits = d_hits; a.weights = d_weights; a.pixels = d_pixels; a.light_scale = d_light_scale;
    a.lt = light_args_of(light); a.spp = spp; a.inv_spp = 1.0f / (float)spp; a.n = n; a.rgb = d_rgb;
    return a;
}

// t: read by kColorTexture only; color, normal: three floats per ray each, read by kColorSurface only
template <int SRC>
__device__ __forceinline__ void shade_accumulate_body(const AccumArgs a, const TexParams t, const float *color, const float *normal) {
    using namespace rec;
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const unsigned long long n_round = (a.n + 63ull) & ~63ull;                            // whole waves: accumulate_runs shuffles
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n_round; k += stride) {
        float v[3] = {0.f, 0.f, 0.f};
        uint32_t pix = 0xFFFFFFFFu;
        if (k < a.n) {
            pix = pixel_of(a.pixels, k, a.spp);
            const float4 h = reinterpret_cast<const float4 *>(a.hits)[k];
            const uint32_t prim = __float_as_uint(h.y);
            const float scale = prim != MR_MISS ? a.light_scale[k] : 0.0f;                // a miss: m_bgColor = 0 contributes nothing
            if (scale != 0.0f) {
                float P[3], N[3], diffuse[3], highlight, out[3];
                surface_point(a.m, a.rays, k, h, P, N);
                const float4 rb = reinterpret_cast<const float4 *>(a.rays)[2 * k + 1];
                const float *mt = material_of(a.m, prim);
                float col[3] = {0.f, 0.f, 0.f};
                if (SRC == kColorTexture) diffuse_color_of(a.m, t, material_id(a.m.s, a.m.prim_mat, prim), prim, P, col);
                if (SRC == kColorSurface)
                    for (int c = 0; c < 3; c++) { col[c] = color[3 * k + c]; N[c] = normal[3 * k + c]; }
                phong_terms(a.lt, mt, SRC == kColorMaterial ? mt : col, P, N, rb.x, rb.y, rb.z, diffuse, highlight);
                phong_combine(diffuse, highlight, scale, out);
                float w[3];
                weight_of(a.weights, k, w);
                for (int c = 0; c < 3; c++) v[c] = out[c] * w[c] * a.inv_spp;
            }
        }
        accumulate_runs(a.rgb, pix, v[0], v[1], v[2]);
    }
}

}  // namespace
}  // namespace mr
