// mr_lights.hip -- Phong::shade (Phong.cpp:44-160) for a batch of traced rays over the scene's LIGHT LIST in ONE launch
// (mr_shade_lights):
//
//   for every ray with a hit:  L = 0;  for every light of Scene::lights() in list order (Phong.cpp:59-63): the shadow ray
//   (:80-92), Scene::trace (:97), the occluder's light scale (:97-113), the light's diffuse term times the scale plus its
//   highlight (:116-156) added to L;  then weight * L / spp added to the ray's pixel.
//
// One lane owns one ray for the whole call.  It loads the ray and its hit record, rebuilds P / N once, and walks the light
// list: the list (at most MR_MAX_LIGHTS records) sits in the kernel arguments and the loop index is wave-uniform, so the trip
// count and a light's fields are scalar loads.  Each iteration builds the shadow ray in registers and traces it with
// trace_ray (mr_traverse.h) on the scene's ordinary tables -- the traversal the level kernel runs for its shadow ray -- so
// the shadow hit, and with it the light scale, is the record of mr_gen_shadow_rays -> mr_trace_indirect.  No shadow-ray,
// shadow-hit, source-index or light-scale buffer exists.  Across a traversal a lane keeps P, N, the ray direction, the
// running L and the material pointer; the shadow ray is rebuilt from P afterwards (a handful of operations), the weight and
// the pixel are loaded after the loop.
//
// Lanes whose ray missed idle through the loop: a launch works at the hit rate of its queue (the finding of
// profiles/r02_level_probe.log for the level kernel) -- dense first levels are what it is for.
//
// Two kinds of light:
//   MR_LIGHT_POINT  PointLight (PointLight.h:8-59): shadow_ray_of / phong_terms / phong_combine / light_scale_of (mr_phong.h),
//                   the code of the batched chain, so that one point light gives the chain's bits.
//   MR_LIGHT_DISC   DirectionalAreaLight (DirectionalAreaLight.h:7-38) as Phong::shade treats it, quirks included:
//                   getLightDirection ignores the sampled origin (no random number); l = -normal, the shadow ray runs from
//                   P + l * epsilon along l / |l| with tMax = |normal| (:81-97: sqrt(falloff) of the UN-normalised l -- with a
//                   unit normal occluders are looked for one unit towards the light only); after the shadow test
//                   nDotL = dot(N, -normal) with the normal as given, the hit must lie inside the disc's cylinder
//                   (:132-133), falloff = 1 / PI (:135): shadow_ray_for / disc_terms of mr_phong.h.
#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_phong.h"
#include "mr_recursion.h"
#include "mr_traverse.h"

namespace mr {
namespace {

using namespace rec;

struct LightsArgs {
    TraceParams tp;              // scene arrays, root box; tp.rays = the batch, tp.n its length
    MeshMat m;
    const mr_hit *hits;
    const float *weights;        // rgb per ray or NULL (= 1)
    const uint32_t *pixels;      // pixel per ray or NULL (= ray index / spp)
    uint32_t spp, n_lights;
    float inv_spp;
    float *rgb;                  // may be NULL (then ray_rgb is not)
    float *ray_rgb;              // may be NULL: the un-weighted L of every ray
    unsigned long long *counts;  // optional: [0] += shadow rays traced
    ShadeLight lights[MR_MAX_LIGHTS];
};

// VAR: the traversal variant of trace_ray (mr_traverse.h); ANY: the shadow rays stop at their first accepted hit (scenes
// without a refractive material only: every occluder then scales the light to 0, whichever it is)
template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void shade_lights_kernel(LightsArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    const int tid = threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTraceBlock;
    const unsigned long long n = a.tp.n;
    const unsigned long long n_round = whole_workgroups(n);
    Stats st = {0ull, 0ull};
    unsigned my_shadow_rays = 0;

    for (unsigned long long k = (unsigned long long)xcd_block_id() * kTraceBlock + tid; k < n_round; k += stride) {
        const bool live = k < n;
        float4 h = make_float4(0.f, __uint_as_float(MR_MISS), 0.f, 0.f);
        if (live) h = reinterpret_cast<const float4 *>(a.hits)[k];
        const bool hit = __float_as_uint(h.y) != MR_MISS;              // a miss contributes nothing (m_bgColor = 0)
        float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 1.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
        const float *mt = a.m.mats;
        if (hit) {
            surface_point(a.m, a.tp.rays, k, h, P, N);
            const float4 rb = reinterpret_cast<const float4 *>(a.tp.rays)[2 * k + 1];
            d[0] = rb.x; d[1] = rb.y; d[2] = rb.z;
            mt = material_of(a.m, __float_as_uint(h.y));
            my_shadow_rays += a.n_lights;
        }

        float L[3] = {0.f, 0.f, 0.f};
        for (uint32_t li = 0; li < a.n_lights; li++) {                 // Phong.cpp:63, wave-uniform
            const ShadeLight &lt = a.lights[li];
            float4 sh;
            {
                float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(1.f, 1.f, 1.f, -1.f);
                if (hit) shadow_ray_for(lt, P, sa, sb);
                const mr_hit hs = trace_hit<true, ANY, false, VAR>(a.tp, sa, sb, sb.w, hit, s_stack, tid, st);
                sh = *reinterpret_cast<const float4 *>(&hs);
            }
            if (hit) {
                float4 sa, sb;
                shadow_ray_for(lt, P, sa, sb);                         // rebuilt rather than kept across the traversal
                const float scale = light_scale_of(a.m, sa, sb, sh);
                float diffuse[3] = {0.f, 0.f, 0.f}, highlight = 0.0f, out[3] = {0.f, 0.f, 0.f};
                bool lit = scale != 0.0f;                              // Phong.cpp:100-111: the light is skipped
                if (lit) {
                    if (lt.kind == MR_LIGHT_DISC) {
                        const float l[3] = {sb.x, sb.y, sb.z};
                        lit = disc_terms(lt, mt, P, N, l, d[0], d[1], d[2], diffuse, highlight);
                    } else {
                        phong_terms(lt.position, lt.color, lt.wattage, mt, P, N, d[0], d[1], d[2], diffuse, highlight);
                    }
                }
                if (lit) phong_combine(diffuse, highlight, scale, out);
                L[0] += out[0]; L[1] += out[1]; L[2] += out[2];
            }
        }

        if (a.ray_rgb && live) { a.ray_rgb[3 * k] = L[0]; a.ray_rgb[3 * k + 1] = L[1]; a.ray_rgb[3 * k + 2] = L[2]; }
        if (a.rgb) {                                                   // wave-uniform
            uint32_t pix = 0xFFFFFFFFu;
            float v[3] = {0.f, 0.f, 0.f};
            if (live) pix = pixel_of(a.pixels, k, a.spp);
            if (hit) {
                float w[3];
                weight_of(a.weights, k, w);
                for (int c = 0; c < 3; c++) v[c] = L[c] * w[c] * a.inv_spp;
            }
            accumulate_runs(a.rgb, pix, v[0], v[1], v[2]);
        }
    }

    if (a.counts) workgroup_add<kTraceBlock>(my_shadow_rays, &a.counts[0]);
}

template <int VAR, bool ANY>
mr_status launch_lights_t(const LightsArgs &a, hipStream_t stream) {
    size_t lds = 0;
    const mr_status st = stack_lds(&shade_lights_kernel<VAR, ANY>, a.tp.stack_depth, kStackLdsShared, lds);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL((shade_lights_kernel<VAR, ANY>), dim3(trace_grid(a.tp.n)), dim3(kTraceBlock), lds, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

template <int VAR>
mr_status launch_lights_a(const LightsArgs &a, bool any, hipStream_t stream) {
    return any ? launch_lights_t<VAR, true>(a, stream) : launch_lights_t<VAR, false>(a, stream);
}

}  // namespace

mr_status launch_shade_lights(const DeviceScene &ds, const ShadeLight *lights, uint32_t n_lights, const mr_ray *d_rays,
                              const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels, unsigned long long n,
                              uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts,
                              hipStream_t stream) {
    if (n == 0) return MR_OK;
    LightsArgs a;
    a.tp = scene_trace_params(ds);
    a.tp.rays = d_rays; a.tp.n = n;
    a.m = mesh_of(ds);
    a.hits = d_hits; a.weights = d_weights; a.pixels = d_pixels;
    a.spp = spp; a.n_lights = n_lights; a.inv_spp = 1.0f / (float)spp;
    a.rgb = d_rgb; a.ray_rgb = d_ray_rgb; a.counts = d_counts;
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) a.lights[i] = lights[i < n_lights ? i : 0];

    // the traversal variants of launch_level / launch_trace: the same hit records from each of them
    const bool any = flags & MR_TRACE_ANY;
    return with_trace_variant(ds.n_planes || ds.n_spheres, flags & MR_MATH_PRODUCT, flags & MR_TRACE_INCOHERENT,
                              [&](auto var) { return launch_lights_a<decltype(var)::value>(a, any, stream); });
}

}  // namespace mr
