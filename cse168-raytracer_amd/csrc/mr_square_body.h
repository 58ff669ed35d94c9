// mr_square_body.h -- the body of shade_square_lights_kernel (mr_distribution.hip, where the kernel is described) as a
// __device__ template, so that its surface-pass form (mr_square_surface.hip) is the same loop with two loads per hit, the way
// mr_lights_body.h serves the light-list kernels.  SRC (ColorSource, mr_texture.h) says where the hit's diffuseColor and N come
// from:
//   kColorMaterial  the material's own m_diffuse and the object's normal, computed here (mr_shade_square_lights)
//   kColorSurface   both loaded from the surface pass's per-ray buffers (mr_hit_surface): the colour of Phong.cpp:51-56 and the
//                   normal that Scene::trace hands on (Scene.cpp:234-263), bumped on a STONE material.  The colour is the
//                   separate `dc` of phong_terms (mr_phong.h); `mt` stays the hit's material record, whose m_diffuse is the
//                   second factor of Phong.cpp:146 and whose shininess gates the highlight.  The buffered N feeds the diffuse
//                   term and the highlight, as Phong.cpp:139,151 read hit.N.  P is still rebuilt from ray and hit.  Both
//                   buffers are read for rays with a hit only: mr_hit_surface leaves the six floats of a miss untouched.
// The occluder's side keeps the object's own normal in both forms: light_scale_of reads the shadow hit's normal
// (Phong.cpp:102-109) only for a refractive occluder, a STONE material must have kt = 0 (ks is free) and so never is one, and nothing
// bumps a UVW material -- the bumped normal and the object's are the same wherever that arm looks.
// kColorSurface keeps the colour (three registers) across up to 64 shadow traversals per light.  The arguments are taken BY
// VALUE, for the reason mr_lights_body.h gives; the two buffers are kernel arguments of their own rather than fields of
// SquareArgs, so that the plain kernel's argument block is what it was.  The host work of the two launchers -- the argument
// block with tangents, cell sizes and hseed, and the launch by traversal variant -- is square_args_of / launch_square_variant below.
// Included by the .hip units that instantiate it (everything here is local to its unit).
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_lights_body.h"

namespace mr {
namespace {

constexpr uint32_t kSquareDomain = 0x73717561u;       // "squa": the seed domain of the sample pairs

// a SquareLight as the kernel takes it: tangents (getTangents, Utility.h:25-31) and cell sizes (SquareLight.h:27-29) from the host
struct SquareLightRec {
    float position[3], t1[3], t2[3], color[3], wattage;
    float du, dv, half_u, half_v;    // m_dimensions / sideLength, m_dimensions / 2.0f
};

// ShadeArgs' fields (mr_lights_body.h: fill_shade_args and the shared pieces take either) with the kernel's own among them.  With
// a ShadeArgs as member or base every variant reserves 32 B more scratch per lane, touched by nothing, and leaves the budget.
struct SquareArgs {
    TraceParams tp;
    rec::MeshMat m;
    const mr_hit *hits;
    const float *weights;
    const uint32_t *pixels;
    const float *uv_in;              // NULL: the counter generator; else 2 * n * n_lights * samples floats
    uint32_t spp, n_lights, side, samples, hseed;
    float inv_spp, fsamples;
    float *rgb, *ray_rgb;
    unsigned long long *counts;
    SquareLightRec lights[MR_MAX_LIGHTS];
};

// samplePhotonOrigin(i, samples) for sample cell (sx, sy) of light li and ray k (SquareLight.h:23-39), and the shadow ray to it
__device__ __forceinline__ void square_shadow_ray(const SquareArgs &a, const SquareLightRec &lt, unsigned long long k, uint32_t li,
                                                  uint32_t sx, uint32_t sy, const float P[3], float origin[3], float4 &sa, float4 &sb) {
    const uint32_t i = sy * a.side + sx;
    float r0, r1;
    if (a.uv_in) {
        const float2 r = reinterpret_cast<const float2 *>(a.uv_in)[(k * a.n_lights + li) * a.samples + i];
        r0 = r.x; r1 = r.y;
    } else {
        const uint32_t h = pcg32(pcg32(a.hseed ^ (uint32_t)k) + (li * 64u + i));
        r0 = unit01(pcg32(h)); r1 = unit01(pcg32(h ^ 0x68bc21ebu));
    }
    const float u = ((lt.du * r0) + (float)sx * lt.du) - lt.half_u;                        // SquareLight.h:35-36
    const float v = ((lt.dv * r1) + (float)sy * lt.dv) - lt.half_v;
    for (int c = 0; c < 3; c++) origin[c] = (lt.position[c] + u * lt.t1[c]) + v * lt.t2[c];   // :38
    shadow_ray_of(P, origin[0], origin[1], origin[2], sa, sb);
}

// color, normal: three floats per ray each, read by kColorSurface only
template <int VAR, bool ANY, int SRC>
__device__ __forceinline__ void shade_square_lights_body(const SquareArgs a, const float *color, const float *normal) {
    using namespace rec;
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    const int tid = threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTraceBlock;
    const unsigned long long n = a.tp.n;
    const unsigned long long n_round = whole_workgroups(n);
    Stats st = {0ull, 0ull};
    unsigned my_shadow_rays = 0;

    for (unsigned long long k = (unsigned long long)xcd_block_id() * kTraceBlock + tid; k < n_round; k += stride) {
        const bool live = k < n;
        const float4 h = hit_record_of(a, k, live);
        const bool hit = __float_as_uint(h.y) != MR_MISS;              // a miss keeps L = 0; store_shaded forms weight * 0
        float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 1.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
        const float *mt = a.m.mats;
        float col[3] = {0.f, 0.f, 0.f};                                // diffuseColor, unless the material's own
        if (hit) {
            shade_point_of(a, k, h, P, N, d, mt);
            if (SRC == kColorSurface)
                for (int c = 0; c < 3; c++) { col[c] = color[3 * k + c]; N[c] = normal[3 * k + c]; }
            my_shadow_rays += a.n_lights * a.samples;
        }
        const float *dc = SRC == kColorMaterial ? mt : col;

        float L[3] = {0.f, 0.f, 0.f};
        for (uint32_t li = 0; li < a.n_lights; li++) {               // Phong.cpp:63, wave-uniform
            const SquareLightRec &lt = a.lights[li];
            for (uint32_t sy = 0; sy < a.side; sy++)                   // :78, sample i = sy * side + sx (SquareLight.h:32-33)
                for (uint32_t sx = 0; sx < a.side; sx++) {
                    float4 sh;
                    {
                        float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(1.f, 1.f, 1.f, -1.f);
                        float origin[3];
                        if (hit) square_shadow_ray(a, lt, k, li, sx, sy, P, origin, sa, sb);                     // :80-92
                        const mr_hit hs = trace_hit<true, ANY, false, VAR>(a.tp, sa, sb, sb.w, hit, s_stack, tid, st);   // :97
                        sh = *reinterpret_cast<const float4 *>(&hs);
                    }
                    if (hit) {
                        float origin[3]; float4 sa, sb;
                        square_shadow_ray(a, lt, k, li, sx, sy, P, origin, sa, sb);   // rebuilt rather than kept across the traversal
                        const float scale = light_scale_of(a.m, sa, sb, sh);        // :97-113
                        if (scale != 0.0f) {                                          // otherwise `continue`: the sample is skipped
                            float diffuse[3], highlight;
                            phong_terms(origin, lt.color, lt.wattage, mt, dc, P, N, d[0], d[1], d[2], diffuse, highlight, a.fsamples);
                            for (int c = 0; c < 3; c++) L[c] += diffuse[c] * scale;                    // :146
                            for (int c = 0; c < 3; c++) L[c] += highlight;                             // :155, one term after the other
                        }
                    }
                }
        }
        store_shaded(a, k, live, L);
    }

    if (a.counts) workgroup_add<kTraceBlock>(my_shadow_rays, &a.counts[0]);
}

// what launch_shade_square_lights and its surface-pass form fill in the same way.  side: the sample cells along an edge
inline SquareArgs square_args_of(const DeviceScene &ds, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t side,
                                 uint32_t seed, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                 const uint32_t *d_pixels, const float *d_uv_in, unsigned long long n, uint32_t spp, float *d_rgb,
                                 float *d_ray_rgb, unsigned long long *d_counts) {
    SquareArgs a;
    fill_shade_args(a, ds, n_lights, d_rays, d_hits, d_weights, d_pixels, n, spp, d_rgb, d_ray_rgb, d_counts);
    a.uv_in = d_uv_in;
    a.side = side; a.samples = side * side; a.fsamples = (float)a.samples;
    a.hseed = pcg32(seed ^ kSquareDomain);
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) {
        const mr_square_light_desc &in = lights[i < n_lights ? i : 0];
        SquareLightRec &o = a.lights[i];
        for (int c = 0; c < 3; c++) { o.position[c] = in.position[c]; o.color[c] = in.color[c]; }
        o.wattage = in.wattage;
        tangents_of(in.normal, o.t1, o.t2);                                      // SquareLight::preCalc
        const float side_length = sqrtf(a.fsamples);                             // SquareLight.h:27-29
        o.du = in.dimensions[0] / side_length; o.dv = in.dimensions[1] / side_length;
        o.half_u = in.dimensions[0] / 2.0f; o.half_v = in.dimensions[1] / 2.0f;
    }
    return a;
}

// ... and launch the same way, the variant by scene and flags.  pick(var, any): the unit's kernel<VAR, ANY> for two
// std::integral_constants (a kernel template cannot be handed over itself); `rest`: its arguments after the SquareArgs
template <typename Pick, typename... Rest>
mr_status launch_square_variant(const DeviceScene &ds, uint32_t flags, const SquareArgs &a, hipStream_t stream, Pick pick, Rest... rest) {
    return with_trace_variant(ds.n_planes || ds.n_spheres, flags & MR_MATH_PRODUCT, flags & MR_TRACE_INCOHERENT, [&](auto var) {
        const auto kern = (flags & MR_TRACE_ANY) ? pick(var, std::true_type()) : pick(var, std::false_type());
        return launch_traversal(kern, trace_grid(a.tp.n), a.tp.stack_depth, stream, a, rest...);
    });
}

}  // namespace
}  // namespace mr
