// mr_distribution.hip -- the two per-sample effects of the reference that draw random numbers: the thin-lens camera and the
// square area light.  Kernels and launchers of both live in this unit; the C entry points are in mr_api.cpp.
//
//   eye_rays_lens_kernel          Camera::eyeRay under -DDOF (Camera.cpp:135-160, Miro.h:18-19, sampleDisc Utility.h:82-95):
//                                 mr_gen_eye_rays_lens.  One lane per sample, a store-bound kernel like eye_rays_kernel.
//   shade_square_lights_kernel    Phong::shade (Phong.cpp:66-157) over a list of SquareLights (SquareLight.h:6-58), `samples`
//                                 shadow rays per hit and light: mr_shade_square_lights.
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

namespace mr {
namespace {

using namespace rec;

// ---------------------------------------------------------------------------------------------------------------------------
// the thin lens
// ---------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kLensRounds = 32;                  // rounds of sampleDisc's rejection loop before the sample is (0, 0)
constexpr uint32_t kLensDomain = 0x4c454e53u;         // "LENS": the lens draws' keys, see mr_gen_eye_rays_lens (miro_hip.h)

struct LensArgs {
    float focus[3];                  // m_eye + m_viewDir * DOF_FOCUS_PLANE (Camera.cpp:142), computed on the host
    float aperture;
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
        } else {
            const uint32_t h = eye_sample_key(f, x, y, sm);
            if (f.jitter) eye_jitter_of(h, dx, dy);
            bool found = false;
            for (uint32_t r = 0; r < kLensRounds && !found; r++) {                      // sampleDisc (Utility.h:86-89)
                const float fx = unit01(pcg32(h ^ (kLensDomain + 2u * r))), fy = unit01(pcg32(h ^ (kLensDomain + 2u * r + 1u)));
                const float xr = (2 * fx - 1) * ln.aperture, yr = (2 * fy - 1) * ln.aperture;
                if (!(xr * xr + yr * yr > ln.aperture * ln.aperture)) { lx = xr; ly = yr; found = true; }
            }
            if (!found) mine[1]++;
        }
        float up, vp, e[3], lw[3];
        eye_film_of(f, x, y, dx, dy, up, vp);
        for (int c = 0; c < 3; c++) {
            e[c] = f.eye[c] + (lx * f.u[c] + ly * f.v[c]);                                 // Camera.cpp:140
            lw[c] = -(ln.focus[c] - e[c]);                                                 // :142, :145
        }
        normalize3(lw);
        reinterpret_cast<float4 *>(rays)[2 * k] = make_float4(e[0], e[1], e[2], 0.0f);
        reinterpret_cast<float4 *>(rays)[2 * k + 1] = eye_direction_of(f, up, vp, lw);     // :160, uDir / vDir of the unmoved eye
        if (ln.out) reinterpret_cast<float4 *>(ln.out)[k] = make_float4(dx, dy, lx, ly);
        mine[0]++;
    }
    if (ln.counts) workgroup_add<kBlock, 2>(mine, ln.counts);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the square light
// ---------------------------------------------------------------------------------------------------------------------------
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
    MeshMat m;
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

template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(6, 8))) void shade_square_lights_kernel(SquareArgs a) {
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
        const bool hit = __float_as_uint(h.y) != MR_MISS;              // a miss contributes nothing
        float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 1.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
        const float *mt = a.m.mats;
        if (hit) {
            shade_point_of(a, k, h, P, N, d, mt);
            my_shadow_rays += a.n_lights * a.samples;
        }

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
                            phong_terms(origin, lt.color, lt.wattage, mt, P, N, d[0], d[1], d[2], diffuse, highlight, a.fsamples);
                            for (int c = 0; c < 3; c++) L[c] += diffuse[c] * scale;                    // :146
                            for (int c = 0; c < 3; c++) L[c] += highlight;                             // :155, one term after the other
                        }
                    }
                }
        }
        store_shaded(a, k, live, hit, L);
    }

    if (a.counts) workgroup_add<kTraceBlock>(my_shadow_rays, &a.counts[0]);
}

template <int VAR, bool ANY>
mr_status launch_square_t(const SquareArgs &a, hipStream_t stream) {
    size_t lds = 0;
    const mr_status st = stack_lds(&shade_square_lights_kernel<VAR, ANY>, a.tp.stack_depth, kStackLdsShared, lds);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL((shade_square_lights_kernel<VAR, ANY>), dim3(trace_grid(a.tp.n)), dim3(kTraceBlock), lds, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace

mr_status launch_eye_rays_lens(const mr_camera &cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t spp, uint32_t jitter,
                               uint32_t seed, const mr_lens_desc &lens, const float *d_samples_in, float *d_samples_out,
                               unsigned long long *d_counts, mr_ray *d_rays, hipStream_t stream) {
    float view[3];
    const EyeFrame f = make_eye_frame(cam, W, H, y0, y1, spp, jitter, seed, false, view);
    if (f.n == 0) return MR_OK;
    LensArgs ln;
    for (int c = 0; c < 3; c++) ln.focus[c] = cam.eye[c] + view[c] * lens.focus_plane;    // Camera.cpp:142's first two terms
    ln.aperture = lens.aperture; ln.in = d_samples_in; ln.out = d_samples_out; ln.counts = d_counts;
    hipLaunchKernelGGL(eye_rays_lens_kernel, dim3(grid_for(f.n)), dim3(kBlock), 0, stream, f, ln, d_rays);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_shade_square_lights(const DeviceScene &ds, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t side,
                                     uint32_t seed, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                     const uint32_t *d_pixels, const float *d_uv_in, unsigned long long n, uint32_t spp, uint32_t flags,
                                     float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
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
    return with_trace_variant(ds.n_planes || ds.n_spheres, flags & MR_MATH_PRODUCT, flags & MR_TRACE_INCOHERENT, [&](auto var) {
        constexpr int V = decltype(var)::value;
        return (flags & MR_TRACE_ANY) ? launch_square_t<V, true>(a, stream) : launch_square_t<V, false>(a, stream);
    });
}

}  // namespace mr
