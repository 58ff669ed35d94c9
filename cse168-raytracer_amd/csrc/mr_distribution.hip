// mr_distribution.hip -- the two per-sample effects of the reference that draw random numbers: the thin-lens camera and the
// square area light.  Kernels and launchers of both live in this unit; the C entry points are in mr_api.cpp.
//
//   eye_rays_lens_kernel          Camera::eyeRay under -DDOF (Camera.cpp:135-160, Miro.h:18-19, sampleDisc Utility.h:82-95):
//                                 mr_gen_eye_rays_lens.  One lane per sample, a store-bound kernel like eye_rays_kernel.
//   shade_square_lights_kernel    Phong::shade (Phong.cpp:66-157) over a list of SquareLights (SquareLight.h:6-58), `samples`
//                                 shadow rays per hit and light: mr_shade_square_lights.  Its body is the template of
//                                 mr_square_body.h, which mr_square_surface.hip instantiates for mr_shade_square_lights_surface.
//
// The square-light kernel is shade_lights_kernel (mr_lights.hip) with one more loop, written from the same pieces
// (mr_lights_body.h): a SquareLight is a PointLight whose origin is sampled (SquareLight.h:6-58), so a sample is
// shadow_ray_of and phong_terms (mr_phong.h) at the sampled origin, with the wattage divided by the sample count.  One lane
// owns one ray for the whole call: it loads the ray and its hit record, rebuilds P / N once and walks lights x sample cells;
// the list (at most MR_MAX_LIGHTS records) sits in the kernel arguments and light, cell row and cell column are
// wave-uniform, so a light's fields and the cell offsets are scalar.  Every iteration draws its pair (r0, r1), builds the
// sampled origin and the shadow ray in registers and traces it with trace_hit (mr_traverse.h) on the scene's ordinary
// tables: no shadow-ray, shadow-hit or sample buffer exists, and at samples = 49 a hit costs 49 traversals per light inside
// one launch rather than 49 host rounds of mr_gen_shadow_rays -> mr_trace_indirect -> mr_shade_accumulate.  The origin and
// the shadow ray are rebuilt from the pair after the traversal rather than kept across it.  Lanes whose ray missed idle
// through the loops, as in shade_lights_kernel.
//
// Compiled with -ffp-contract=off like the rest of the library: every fp32 operation is one rounding, in the reference's order.
#include <hip/hip_runtime.h>

#include "mr_eye.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_lights_body.h"
#include "mr_square_body.h"

namespace mr {
namespace {

using namespace rec;

// ---------------------------------------------------------------------------------------------------------------------------
// the thin lens
// ---------------------------------------------------------------------------------------------------------------------------
// The per-sample arithmetic is mr_eye.h's (eye_lens_draw, eye_lens_ray), which the fused lens frame (mr_frame_lens.hip) calls too.
struct LensArgs {
    LensParams p;                    // the focus point and the aperture
    const float *in;                 // optional: dx, dy, lx, ly per ray
    float *out;                      // optional: the values used
    unsigned long long *counts;      // optional: [0] += rays written, [1] += samples that exhausted kLensRounds
};

__global__ __launch_bounds__(kBlock) void eye_rays_lens_kernel(EyeFrame f, LensArgs ln, mr_ray *rays) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned mine[2] = {0u, 0u};
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < f.n; k += stride) {
        uint32_t x, row, y, sm;
        eye_sample_of(f, k, x, row, y, sm);
        float dx = 0.5f, dy = 0.5f, lx = 0.0f, ly = 0.0f;
        if (ln.in) {
            const float4 s = reinterpret_cast<const float4 *>(ln.in)[k];
            dx = s.x; dy = s.y; lx = s.z; ly = s.w;
        } else if (!eye_lens_draw(f, ln.p.aperture, x, y, sm, dx, dy, lx, ly)) {
            mine[1]++;
        }
        float4 ra, rb;
        eye_lens_ray(f, ln.p, x, y, dx, dy, lx, ly, ra, rb);
        reinterpret_cast<float4 *>(rays)[2 * k] = ra;
        reinterpret_cast<float4 *>(rays)[2 * k + 1] = rb;
        if (ln.out) reinterpret_cast<float4 *>(ln.out)[k] = make_float4(dx, dy, lx, ly);
        mine[0]++;
    }
    if (ln.counts) workgroup_add<kBlock, 2>(mine, ln.counts);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the square light
// ---------------------------------------------------------------------------------------------------------------------------
// The loop is shade_square_lights_body (mr_square_body.h, with SquareArgs, SquareLightRec and square_shadow_ray), which the
// surface-pass form (mr_square_surface.hip) instantiates with kColorSurface; here the hit's N is computed and diffuseColor is
// the material's own.
template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void shade_square_lights_kernel(SquareArgs a) {
    shade_square_lights_body<VAR, ANY, kColorMaterial>(a, nullptr, nullptr);
}

}  // namespace

mr_status launch_eye_rays_lens(const mr_camera &cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t spp, uint32_t jitter,
                               uint32_t seed, const mr_lens_desc &lens, const float *d_samples_in, float *d_samples_out,
                               unsigned long long *d_counts, mr_ray *d_rays, hipStream_t stream) {
    float view[3];
    const EyeFrame f = make_eye_frame(cam, W, H, y0, y1, spp, jitter, seed, false, view);
    if (f.n == 0) return MR_OK;
    LensArgs ln;
    ln.p = lens_params_of(cam, view, lens);
    ln.in = d_samples_in; ln.out = d_samples_out; ln.counts = d_counts;
    hipLaunchKernelGGL(eye_rays_lens_kernel, dim3(grid_for(f.n)), dim3(kBlock), 0, stream, f, ln, d_rays);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_shade_square_lights(const DeviceScene &ds, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t side,
                                     uint32_t seed, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                     const uint32_t *d_pixels, const float *d_uv_in, unsigned long long n, uint32_t spp, uint32_t flags,
                                     float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    const SquareArgs a = square_args_of(ds, lights, n_lights, side, seed, d_rays, d_hits, d_weights, d_pixels, d_uv_in, n, spp, d_rgb, d_ray_rgb, d_counts);
    return launch_square_variant(ds, flags, a, stream, [](auto var, auto any) {
        return &shade_square_lights_kernel<decltype(var)::value, decltype(any)::value>;
    });
}

}  // namespace mr
