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
#include "mr_lights_body.h"

namespace mr {
namespace {

using namespace rec;

// VAR: the traversal variant of trace_ray (mr_traverse.h); ANY: the shadow rays stop at their first accepted hit (scenes
// without a refractive material only: every occluder then scales the light to 0, whichever it is).  The body is
// shade_lights_body (mr_lights_body.h), which the textured form in mr_textures.hip and the surface-pass form in
// mr_procedural.hip share.
template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void shade_lights_kernel(LightsArgs a) {
    shade_lights_body<VAR, ANY, kColorMaterial>(a, TexParams(), nullptr, nullptr);
}

}  // namespace

mr_status launch_shade_lights(const DeviceScene &ds, const ShadeLight *lights, uint32_t n_lights, const mr_ray *d_rays,
                              const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels, unsigned long long n,
                              uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts,
                              hipStream_t stream) {
    if (n == 0) return MR_OK;
    const LightsArgs a = lights_args_of(ds, lights, n_lights, d_rays, d_hits, d_weights, d_pixels, n, spp, d_rgb, d_ray_rgb, d_counts);

    // the traversal variants of launch_level / launch_trace: the same hit records from each of them
    const bool any = flags & MR_TRACE_ANY;
    return with_trace_variant(ds.n_planes || ds.n_spheres, flags & MR_MATH_PRODUCT, flags & MR_TRACE_INCOHERENT, [&](auto var) {
        constexpr int VAR = decltype(var)::value;
        return launch_traversal(any ? &shade_lights_kernel<VAR, true> : &shade_lights_kernel<VAR, false>, trace_grid(n), a.s.tp.stack_depth, stream, a);
    });
}

}  // namespace mr
