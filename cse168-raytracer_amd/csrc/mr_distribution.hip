// mr_distribution.hip -- the two per-sample effects of the reference that draw random numbers: the thin-lens camera and the
// square area light.  Kernels, launchers and the C entry points of both live in this unit.
//
//   eye_rays_lens_kernel          Camera::eyeRay under -DDOF (Camera.cpp:135-160, Miro.h:18-19, sampleDisc Utility.h:82-95):
//                                 mr_gen_eye_rays_lens.  One lane per sample, a store-bound kernel like eye_rays_kernel.
//   shade_square_lights_kernel    Phong::shade (Phong.cpp:66-157) over a list of SquareLights (SquareLight.h:6-58), `samples`
//                                 shadow rays per hit and light: mr_shade_square_lights.
//
// The square-light kernel is shade_lights_kernel (mr_lights.hip) with one more loop.  One lane owns one ray for the whole call:
// it loads the ray and its hit record, rebuilds P / N once and walks lights x sample cells; the list (at most MR_MAX_LIGHTS
// records) sits in the kernel arguments and light, cell row and cell column are wave-uniform, so a light's fields and the
// cell offsets are scalar.  Every iteration draws its pair (r0, r1), builds the sampled origin and the shadow ray in registers
// and traces it with trace_hit (mr_traverse.h) on the scene's ordinary tables: no shadow-ray, shadow-hit or sample buffer
// exists, and at samples = 49 a hit costs 49 traversals per light inside one launch rather than 49 host rounds of
// mr_gen_shadow_rays -> mr_trace_indirect -> mr_shade_accumulate.  Across a traversal a lane keeps P, N, the ray direction,
// the running L and the material pointer; the origin and the shadow ray are rebuilt from the pair afterwards (the pair is
// drawn again from its key, or read again: a handful of operations against a traversal).  Lanes whose ray missed idle through
// the loops, as in shade_lights_kernel.
//
// Compiled with -ffp-contract=off like the rest of the library: every fp32 operation is one rounding, in the reference's order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mr_eye.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_phong.h"
#include "mr_recursion.h"
#include "mr_surface.h"
#include "mr_traverse.h"

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
            const uint32_t h = eye_pcg(eye_pcg(f.hbase ^ (y * f.W + x)) + sm);          // eye_ray_of's per-sample hash
            if (f.jitter) {
                dx = (float)(eye_pcg(h) >> 8) * (1.0f / 16777216.0f);
                dy = (float)(eye_pcg(h ^ 0x68bc21ebu) >> 8) * (1.0f / 16777216.0f);
            }
            bool found = false;
            for (uint32_t r = 0; r < kLensRounds && !found; r++) {                      // sampleDisc (Utility.h:86-89)
                const float fx = (float)(eye_pcg(h ^ (kLensDomain + 2u * r)) >> 8) * (1.0f / 16777216.0f);
                const float fy = (float)(eye_pcg(h ^ (kLensDomain + 2u * r + 1u)) >> 8) * (1.0f / 16777216.0f);
                const float xr = (2 * fx - 1) * ln.aperture, yr = (2 * fy - 1) * ln.aperture;
                if (!(xr * xr + yr * yr > ln.aperture * ln.aperture)) { lx = xr; ly = yr; found = true; }
            }
            if (!found) mine[1]++;
        }
        const float up = f.left + (f.right - f.left) * (((float)x + dx) / (float)f.W);     // Camera.cpp:157-158
        const float vp = f.bottom + (f.top - f.bottom) * (((float)y + dy) / (float)f.H);
        float e[3], lw[3], d[3];
        for (int c = 0; c < 3; c++) {
            e[c] = f.eye[c] + (lx * f.u[c] + ly * f.v[c]);                                 // :140
            lw[c] = -(ln.focus[c] - e[c]);                                                 // :142, :145
        }
        {
            const float len = sqrtf((lw[0] * lw[0] + lw[1] * lw[1]) + lw[2] * lw[2]);
            const float inv = 1.0f / len;
            lw[0] *= inv; lw[1] *= inv; lw[2] *= inv;
        }
        for (int c = 0; c < 3; c++) d[c] = (up * f.u[c] + vp * f.v[c]) - lw[c];            // :160, uDir / vDir of the unmoved eye
        const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        const float inv = 1.0f / len;
        reinterpret_cast<float4 *>(rays)[2 * k] = make_float4(e[0], e[1], e[2], 0.0f);
        reinterpret_cast<float4 *>(rays)[2 * k + 1] = make_float4(d[0] * inv, d[1] * inv, d[2] * inv, 1e12f);   // MIRO_TMAX
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

struct SquareArgs {
    TraceParams tp;                  // scene arrays, root box; tp.rays = the batch, tp.n its length
    MeshMat m;
    const mr_hit *hits;
    const float *weights;            // rgb per ray or NULL (= 1)
    const uint32_t *pixels;          // pixel per ray or NULL (= ray index / spp)
    const float *uv_in;              // NULL: the counter generator; else 2 * n * n_lights * samples floats
    uint32_t spp, n_lights, side, samples, hseed;
    float inv_spp, fsamples;
    float *rgb, *ray_rgb;            // either may be NULL, not both
    unsigned long long *counts;      // optional: [0] += shadow rays traced
    SquareLightRec lights[MR_MAX_LIGHTS];
};

// getLightDirection(samplePhotonOrigin(i, samples), P) for sample cell (sx, sy) of light li and ray k: l = origin - P, not
// normalised (SquareLight.h:23-39, PointLight.h:40-43)
__device__ __forceinline__ void square_light_direction(const SquareArgs &a, const SquareLightRec &lt, unsigned long long k, uint32_t li,
                                                       uint32_t sx, uint32_t sy, const float P[3], float l[3]) {
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
    for (int c = 0; c < 3; c++) l[c] = ((lt.position[c] + u * lt.t1[c]) + v * lt.t2[c]) - P[c];   // :38, PointLight.h:42
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
        float4 h = make_float4(0.f, __uint_as_float(MR_MISS), 0.f, 0.f);
        if (live) h = reinterpret_cast<const float4 *>(a.hits)[k];
        const bool hit = __float_as_uint(h.y) != MR_MISS;              // a miss contributes nothing
        float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 1.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
        const float *mt = a.m.mats;
        if (hit) {
            surface_point(a.m, a.tp.rays, k, h, P, N);
            const float4 rb = reinterpret_cast<const float4 *>(a.tp.rays)[2 * k + 1];
            d[0] = rb.x; d[1] = rb.y; d[2] = rb.z;
            mt = material_of(a.m, __float_as_uint(h.y));
            my_shadow_rays += a.n_lights * a.samples;
        }

        float L[3] = {0.f, 0.f, 0.f};
        for (uint32_t li = 0; li < a.n_lights; li++) {                 // Phong.cpp:63, wave-uniform
            const SquareLightRec &lt = a.lights[li];
            for (uint32_t sy = 0; sy < a.side; sy++)                   // :78, sample i = sy * side + sx (SquareLight.h:32-33)
                for (uint32_t sx = 0; sx < a.side; sx++) {
                    float4 sh;
                    {
                        float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(1.f, 1.f, 1.f, -1.f);
                        if (hit) {
                            float l[3];
                            square_light_direction(a, lt, k, li, sx, sy, P, l);
                            shadow_ray_along(P, l[0], l[1], l[2], sa, sb);         // :85-92
                        }
                        const mr_hit hs = trace_hit<true, ANY, false, VAR>(a.tp, sa, sb, sb.w, hit, s_stack, tid, st);   // :97
                        sh = *reinterpret_cast<const float4 *>(&hs);
                    }
                    if (hit) {
                        float l[3];
                        float4 sa, sb;
                        square_light_direction(a, lt, k, li, sx, sy, P, l);        // rebuilt rather than kept across the traversal
                        shadow_ray_along(P, l[0], l[1], l[2], sa, sb);
                        const float scale = light_scale_of(a.m, sa, sb, sh);       // :97-113
                        if (scale != 0.0f) {                                       // otherwise `continue`: the sample is skipped
                            const float falloff = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2];          // :85
                            const float ln[3] = {sb.x, sb.y, sb.z};                                    // :88
                            const float nDotL = (N[0] * ln[0] + N[1] * ln[1]) + N[2] * ln[2];          // :139
                            const float f2 = 1.0f / (falloff * 4.0f * kPhongPI * kPhongPI);            // :140
                            const float diff = fmaxf(0.0f, nDotL * f2 * lt.wattage / a.fsamples);      // :146
                            for (int c = 0; c < 3; c++) L[c] += lt.color[c] * (diff * mt[c] * mt[c]) * scale;
                            if (mt[9] < __builtin_huge_valf()) {                                       // :149-155
                                const float two = 2 * ((ln[0] * N[0] + ln[1] * N[1]) + ln[2] * N[2]);
                                const float rx = -ln[0] + two * N[0], ry = -ln[1] + two * N[1], rz = -ln[2] + two * N[2];
                                float e = (-d[0] * rx + -d[1] * ry) + -d[2] * rz;
                                e = powf(fmaxf(0.0f, fminf(1.0f, e)), 500.0f);
                                const float high = fmaxf(0.0f, e * f2 * lt.wattage / a.fsamples);
                                L[0] += high; L[1] += high; L[2] += high;
                            }
                        }
                    }
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
mr_status launch_square_t(const SquareArgs &a, hipStream_t stream) {
    size_t lds = 0;
    const mr_status st = stack_lds(&shade_square_lights_kernel<VAR, ANY>, a.tp.stack_depth, kStackLdsShared, lds);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL((shade_square_lights_kernel<VAR, ANY>), dim3(trace_grid(a.tp.n)), dim3(kTraceBlock), lds, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

template <int VAR>
mr_status launch_square_a(const SquareArgs &a, bool any, hipStream_t stream) {
    return any ? launch_square_t<VAR, true>(a, stream) : launch_square_t<VAR, false>(a, stream);
}

void cross3(const float *a, const float *b, float *o) {                // Vector3.h cross()
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// getTangents (Utility.h:25-31), as SquareLight::preCalc calls it
void tangents_of(const float normal[3], float t1[3], float t2[3]) {
    const float ez[3] = {0.f, 0.f, 1.f}, ey[3] = {0.f, 1.f, 0.f};
    cross3(ez, normal, t1);
    if ((double)((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]) < 1e-6) cross3(ey, normal, t1);
    cross3(t1, normal, t2);
}

bool finite3(const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace
}  // namespace mr

using namespace mr;

extern "C" {

mr_status mr_gen_eye_rays_lens(mr_scene *s, const mr_camera *cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t spp,
                               uint32_t jitter, uint32_t seed, mr_ray *d_rays, void *stream, const mr_lens_desc *lens,
                               const float *d_samples_in, float *d_samples_out, uint64_t *d_counts) {
    if (!s || !cam || !d_rays) return fail(MR_ERR_INVALID, "NULL argument");
    if (!lens) return fail(MR_ERR_INVALID, "mr_gen_eye_rays_lens: NULL lens");
    for (int k = 0; k < 6; k++)
        if (lens->reserved[k] != 0) return fail(MR_ERR_INVALID, "mr_gen_eye_rays_lens: mr_lens_desc.reserved must be 0");
    if (!std::isfinite(lens->aperture) || lens->aperture < 0.0f) return fail(MR_ERR_INVALID, "mr_gen_eye_rays_lens: aperture must be finite and >= 0");
    if (!std::isfinite(lens->focus_plane) || !(lens->focus_plane > 0.0f)) return fail(MR_ERR_INVALID, "mr_gen_eye_rays_lens: focus_plane must be finite and > 0");
    if (W == 0 || H == 0 || spp == 0 || y1 < y0 || y1 > H) return fail(MR_ERR_INVALID, "bad image window");
    if ((reinterpret_cast<uintptr_t>(d_rays) & 15) || (reinterpret_cast<uintptr_t>(d_samples_in) & 15) ||
        (reinterpret_cast<uintptr_t>(d_samples_out) & 15) || (reinterpret_cast<uintptr_t>(d_counts) & 7))
        return fail(MR_ERR_INVALID, "d_rays and the sample buffers must be 16-byte aligned, counters 8-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    const EyeFrame f = make_eye_frame(*cam, W, H, y0, y1, spp, jitter, seed, false);
    if (f.n == 0) return MR_OK;
    LensArgs ln;
    {   // m_viewDir as make_eye_frame computes it (Camera.h:79-110), then Camera.cpp:142's first two terms
        float view[3] = {cam->lookat[0] - cam->eye[0], cam->lookat[1] - cam->eye[1], cam->lookat[2] - cam->eye[2]};
        const float len = sqrtf((view[0] * view[0] + view[1] * view[1]) + view[2] * view[2]);
        const float inv = 1.0f / len;
        for (int c = 0; c < 3; c++) {
            view[c] *= inv;
            ln.focus[c] = cam->eye[c] + view[c] * lens->focus_plane;
        }
    }
    ln.aperture = lens->aperture;
    ln.in = d_samples_in; ln.out = d_samples_out; ln.counts = reinterpret_cast<unsigned long long *>(d_counts);
    hipLaunchKernelGGL(eye_rays_lens_kernel, dim3(grid_for(f.n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), f, ln, d_rays);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status mr_square_light_tangents(const float normal[3], float t1[3], float t2[3]) {
    if (!normal || !t1 || !t2) return fail(MR_ERR_INVALID, "mr_square_light_tangents: NULL argument");
    tangents_of(normal, t1, t2);
    return MR_OK;
}

mr_status mr_shade_square_lights(mr_scene *s, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t samples, uint32_t seed,
                                 const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels,
                                 const float *d_uv_in, uint64_t n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb,
                                 uint64_t *d_counts, void *stream) {
    const char *who = "mr_shade_square_lights";
    if (!s) return fail(MR_ERR_INVALID, "%s: NULL scene", who);
    if (n_lights == 0 || n_lights > MR_MAX_LIGHTS) return fail(MR_ERR_INVALID, "%s: %u lights, at least 1 and at most %u", who, n_lights, (unsigned)MR_MAX_LIGHTS);
    if (!lights) return fail(MR_ERR_INVALID, "%s: NULL list of %u lights", who, n_lights);
    uint32_t side = 0;
    while (side < 8 && side * side < samples) side++;
    if (samples == 0 || side * side != samples)
        return fail(MR_ERR_INVALID, "%s: samples = %u is not a perfect square in 1 ... 64 (SquareLight.h:27-33 subdivides the rectangle "
                                    "into int(sqrt(samples))^2 cells)", who, samples);
    SquareArgs a;
    for (uint32_t i = 0; i < n_lights; i++) {
        const mr_square_light_desc &in = lights[i];
        for (int k = 0; k < 4; k++)
            if (in.reserved[k] != 0) return fail(MR_ERR_INVALID, "%s: light %u: mr_square_light_desc.reserved must be 0", who, i);
        if (!finite3(in.position) || !finite3(in.color)) return fail(MR_ERR_INVALID, "%s: light %u: position and color must be finite", who, i);
        if (!std::isfinite(in.wattage)) return fail(MR_ERR_INVALID, "%s: light %u: wattage must be finite", who, i);
        if (!finite3(in.normal)) return fail(MR_ERR_INVALID, "%s: light %u: the normal must be finite", who, i);
        if (in.normal[0] == 0.0f && in.normal[1] == 0.0f && in.normal[2] == 0.0f) return fail(MR_ERR_INVALID, "%s: light %u: the normal is zero", who, i);
        for (int k = 0; k < 2; k++)
            if (!std::isfinite(in.dimensions[k]) || in.dimensions[k] < 0.0f)
                return fail(MR_ERR_INVALID, "%s: light %u: dimensions must be finite and >= 0", who, i);
        SquareLightRec &o = a.lights[i];
        for (int c = 0; c < 3; c++) { o.position[c] = in.position[c]; o.color[c] = in.color[c]; }
        o.wattage = in.wattage;
        tangents_of(in.normal, o.t1, o.t2);                                      // SquareLight::preCalc
        const float side_length = sqrtf((float)samples);                         // SquareLight.h:27-29
        o.du = in.dimensions[0] / side_length; o.dv = in.dimensions[1] / side_length;
        o.half_u = in.dimensions[0] / 2.0f; o.half_v = in.dimensions[1] / 2.0f;
    }
    for (uint32_t i = n_lights; i < MR_MAX_LIGHTS; i++) a.lights[i] = a.lights[0];
    if (!d_rays || !d_hits || (!d_rgb && !d_ray_rgb)) return fail(MR_ERR_INVALID, "%s: NULL argument", who);
    if (spp == 0) return fail(MR_ERR_INVALID, "%s: spp is 0", who);
    if (n > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "%s: at most 2^32-1 rays per batch (the sample keys hold the ray index in 32 bits)", who);
    if (flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT | MR_TRACE_ANY))
        return fail(MR_ERR_INVALID, "%s: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT, MR_TRACE_ANY only", who);
    if ((reinterpret_cast<uintptr_t>(d_rays) & 15) || (reinterpret_cast<uintptr_t>(d_hits) & 15) || (reinterpret_cast<uintptr_t>(d_counts) & 7) ||
        (reinterpret_cast<uintptr_t>(d_uv_in) & 7) || (reinterpret_cast<uintptr_t>(d_rgb) & 3) || (reinterpret_cast<uintptr_t>(d_ray_rgb) & 3))
        return fail(MR_ERR_INVALID, "%s: ray / hit buffers must be 16-byte aligned, counters and d_uv_in 8-byte aligned", who);
    if (!s->built) return fail(MR_ERR_STATE, "%s: mr_bvh_build has not been called on this scene", who);
    if (!s->on_device) return fail(MR_ERR_STATE, "%s: scene was built host_only: nothing is resident on a device and there is no CPU fallback", who);
    if (!s->tex.blob.empty())
        return fail(MR_ERR_STATE, "%s: the scene has a texture table (mr_scene_set_textures) and this call shades without the lookup", who);
    if ((flags & MR_TRACE_ANY) && s->dev.refractive)
        return fail(MR_ERR_STATE, "%s: MR_TRACE_ANY with a refractive material (the nearest occluder decides, Phong.cpp:99-113)", who);
    MR_HIP_CHECK(hipSetDevice(s->device));
    if (n == 0) return MR_OK;
    const DeviceScene &ds = s->dev;
    a.tp = scene_trace_params(ds);
    a.tp.rays = d_rays; a.tp.n = n;
    a.m = rec::mesh_of(ds);
    a.hits = d_hits; a.weights = d_weights; a.pixels = d_pixels; a.uv_in = d_uv_in;
    a.spp = spp; a.n_lights = n_lights; a.side = side; a.samples = samples;
    a.hseed = rec::pcg32(seed ^ kSquareDomain);
    a.inv_spp = 1.0f / (float)spp; a.fsamples = (float)samples;
    a.rgb = d_rgb; a.ray_rgb = d_ray_rgb; a.counts = reinterpret_cast<unsigned long long *>(d_counts);
    const bool any = flags & MR_TRACE_ANY;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_trace_variant(ds.n_planes || ds.n_spheres, flags & MR_MATH_PRODUCT, flags & MR_TRACE_INCOHERENT,
                              [&](auto var) { return launch_square_a<decltype(var)::value>(a, any, st); });
}

}  // extern "C"
