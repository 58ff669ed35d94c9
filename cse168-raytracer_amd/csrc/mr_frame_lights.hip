// mr_frame_lights.hip -- the reference's per-pixel loop (Scene::raytraceImage, Scene.cpp:112-141) over the scene's LIGHT LIST
// as ONE launch (mr_render_lights):
//
//   Camera::eyeRay (Camera.cpp:104-161)  ->  Scene::trace (Scene.cpp:278)  ->  Phong::shade's loop over Scene::lights()
//   (Phong.cpp:59-63): per light the shadow ray (:80-92), Scene::trace (:97), the occluder's light scale (:97-113), the
//   light's diffuse term times the scale plus its highlight (:116-156) added to L  ->  mean over the pixel's samples
//   (Scene.cpp:126-139)
//
// It is mr_frame.hip's frame with mr_lights.hip's light loop in the place of its one shadow ray.  One sample per lane: the
// primary ray is generated in registers (eye_sample_of / eye_ray_of, mr_eye.h) and traced (trace_hit, mr_traverse.h); P, N and
// the material come from the hit still in registers; the walk over the list is shade_light_list (mr_light_loop.h), the loop
// of shade_lights_body (mr_lights_body.h), with the material's own colour -- the list (at most MR_MAX_LIGHTS records) sits in the kernel arguments and the loop
// index is wave-uniform --; the pixel's samples meet in frame_kernel's xor-butterfly.  No ray, hit or per-ray colour buffer
// exists: the batched form (mr_gen_eye_rays[_tiled] -> mr_trace -> mr_shade_lights) keeps 32 + 16 + 12 bytes per sample
// resident and moves them through HBM twice; this kernel writes 12 bytes per PIXEL (plus, on request, the 16-byte hit record
// and the 12-byte L of every sample, which is what the parity tests compare).
//
// Every piece is the shared definition the batched kernels use, called in their order under -ffp-contract=off, so hit
// records, per-sample L and pixels are the batched chain's bits -- tests/test_frame_lights.py compares them.
//
// Across a shadow traversal a lane keeps P, N, the ray direction, the running L and the material pointer; the shadow ray is
// rebuilt from P afterwards, pixel and row are computed again after the loop (frame_kernel does the same).
//
// NOT here, on purpose: mr_frame.hip's eye-relative tables, its uniform-run scalar walk, its pulled tail with the counter
// ring and its 128-lane build.  Each was tuned on the single-light kernel against that kernel's register envelope; this
// kernel takes the plain grid-stride loop of the batched kernels (trace_grid workgroups, xcd_block_id) until it has been
// measured.  mr_frame.hip itself is untouched: the window arithmetic of its launcher is written again in mr_frame_window.h,
// which the textured form of this frame (mr_frame_lights_surface.hip) reads too.
#include <hip/hip_runtime.h>

#include "mr_eye.h"
#include "mr_frame_window.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_light_loop.h"
#include "mr_phong.h"
#include "mr_surface.h"
#include "mr_tile.h"
#include "mr_traverse.h"

namespace mr {
namespace {

using namespace rec;

struct FrameLightsArgs {
    EyeFrame eye;
    TraceParams tp;              // scene arrays, root box; rays / hits / n unused
    MeshMat m;
    mr_hit *hits;                // optional: primary hit record of sample k
    float *sample_rgb;           // optional: the un-weighted L of sample k (0 for a miss)
    float *rgb;                  // [rows * W][3], window rows in band order, image order inside a row
    unsigned long long *counts;  // optional: [0] += primary rays, [1] += shadow rays traced by this launch
    uint32_t n_lights;
    ShadeLight lights[MR_MAX_LIGHTS];
};

// VAR: the traversal variant of trace_ray (mr_traverse.h) for both kinds of ray; ANY: the shadow rays stop at their first
// accepted hit (scenes without a refractive material only: every occluder then scales the light to 0, whichever it is).
// The arguments are taken BY VALUE, as shade_lights_body takes them (mr_lights_body.h says why).
// Waves per SIMD: shade_lights_kernel's six (80 registers), except five (96 registers) for kTraceExactObj -- with two traversals
// in one kernel that variant has 37 spilled VGPRs and 132 bytes of scratch per lane at six, beyond the worst kernel of
// tests/golden/kernel_budget.json (30 / 108), and 3 / 80 at five; every other variant stays at 11 / 108 or less at six.
// Occupancy is what this kernel's time follows (profiles/frame_lights_waves_ab.log, sponza stand-in 1080p x 4 spp, 1 / 2 / 4
// lights): five everywhere 1.63 / 2.15 / 3.59 ms, six 1.49 / 1.96 / 3.28 ms, seven (72 registers, up to 57 spilled and 220 bytes:
// outside the envelope) 1.42 / 1.86 / 3.10 ms, against 1.53 / 1.99 / 3.28 ms of the batched route; the two-light room, which is
// kTraceExactObj, 1.495 ms at five, 1.452 at six, 1.484 at seven against 1.503 batched.  MIRO_FRAME_LIGHTS_WAVES (A/B builds)
// sets one value for every variant.
#ifdef MIRO_FRAME_LIGHTS_WAVES
constexpr int frame_lights_waves(int) { return MIRO_FRAME_LIGHTS_WAVES; }
#else
constexpr int frame_lights_waves(int var) { return var == kTraceExactObj ? 5 : 6; }
#endif
template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(frame_lights_waves(VAR), 8))) void frame_lights_kernel(const FrameLightsArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    const int tid = threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTraceBlock;
    const unsigned long long n = a.eye.n;
    const unsigned long long n_round = whole_workgroups(n);
    const uint32_t spp = a.eye.spp;
    Stats st = {0ull, 0ull};
    unsigned my_shadow_rays = 0;

    // whole workgroups run every iteration (n_round): the traversals and the butterfly are called by whole waves
    for (unsigned long long idx = (unsigned long long)xcd_block_id() * kTraceBlock + tid; idx < n_round; idx += stride) {
        const bool live = idx < n;
        uint32_t x = 0, row = 0, y = 0, sm = 0;
        float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = make_float4(1.f, 1.f, 1.f, -1.f);
        if (live) {
            eye_sample_of(a.eye, idx, x, row, y, sm);
            eye_ray_of(a.eye, x, y, sm, ra, rb);
        }
        // ---- primary ray: a closest hit; a lane past the end of the window gets the miss record
        const mr_hit h = trace_hit<true, false, false, VAR>(a.tp, ra, rb, rb.w, live, s_stack, tid, st);
        if (a.hits && live) reinterpret_cast<float4 *>(a.hits)[idx] = *reinterpret_cast<const float4 *>(&h);

        // ---- Phong::shade over the light list (the material's own colour, as kColorMaterial); a miss contributes nothing (m_bgColor = 0)
        const bool hit = live && h.prim != MR_MISS;
        float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 1.f, 0.f};
        const float d[3] = {rb.x, rb.y, rb.z};
        const float *mt = a.m.mats;
        if (hit) {
            // the ray's origin is the eye (a hit lane is a live one): read from the arguments, uniform, where it is used
            surface_point_od(a.m, a.eye.eye[0], a.eye.eye[1], a.eye.eye[2], rb.x, rb.y, rb.z, h.t, h.prim, h.beta, h.gamma, P, N);
            mt = material_of(a.m, h.prim);
            my_shadow_rays += a.n_lights;
        }
        float L[3] = {0.f, 0.f, 0.f};
        shade_light_list<VAR, ANY>(a.tp, a.m, a.lights, a.n_lights, hit, P, N, mt, mt, d, s_stack, tid, st, L);
        if (a.sample_rgb && live) { a.sample_rgb[3 * idx] = L[0]; a.sample_rgb[3 * idx + 1] = L[1]; a.sample_rgb[3 * idx + 2] = L[2]; }

        // ---- the pixel's mean (Scene.cpp:126-139), as frame_kernel forms it: spp is a power of two <= 64 (checked by the
        // host), a pixel's samples are `spp` consecutive, aligned lanes; the summation tree depends on the sample index only
        for (uint32_t off = 1; off < spp; off <<= 1) {
            L[0] += __shfl_xor(L[0], (int)off, 64);
            L[1] += __shfl_xor(L[1], (int)off, 64);
            L[2] += __shfl_xor(L[2], (int)off, 64);
        }
        if (live) eye_sample_of(a.eye, idx, x, row, y, sm);      // recomputed: cheaper than live registers across the traversals
        if (live && sm == 0) {
            if (spp > 1) {
                const float inv_spp = 1.0f / (float)spp;
                L[0] *= inv_spp; L[1] *= inv_spp; L[2] *= inv_spp;
            }
            float *o = a.rgb + 3 * ((size_t)row * a.eye.W + x);
            o[0] = L[0]; o[1] = L[1]; o[2] = L[2];
        }
    }

    // rays traced.  Shadow rays: one atomic per workgroup; primary rays: the launch's sample count, added once.
    if (a.counts) {
        workgroup_add<kTraceBlock>(my_shadow_rays, &a.counts[1]);
        if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.counts[0], n);
    }
}

}  // namespace

mr_status check_frame_lights(const char *who, const mr_frame_desc &fd) {
    EyeFrame eye;
    const mr_status st = frame_window_of(who, fd, eye);
    if (st != MR_OK) return st;
    if (fd.flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT | MR_TRACE_ANY))
        return fail(MR_ERR_INVALID, "%s: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT, MR_TRACE_ANY only", who);
    return MR_OK;
}

mr_status launch_frame_lights(const DeviceScene &ds, const ShadeLight *lights, uint32_t n_lights, const mr_frame_desc &fd, float *d_rgb,
                              mr_hit *d_hits, float *d_sample_rgb, unsigned long long *d_counts, hipStream_t stream) {
    FrameLightsArgs a;
    const mr_status st = frame_window_of("mr_render_lights", fd, a.eye);
    if (st != MR_OK) return st;
    if (a.eye.n == 0) return MR_OK;
    a.tp = scene_trace_params(ds);
    a.tp.n = a.eye.n;
    a.m = mesh_of(ds);
    a.hits = d_hits; a.sample_rgb = d_sample_rgb; a.rgb = d_rgb; a.counts = d_counts;
    a.n_lights = n_lights;
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) a.lights[i] = lights[i < n_lights ? i : 0];

    // the traversal variants of launch_shade_lights: the same hit records from each of them
    const bool any = fd.flags & MR_TRACE_ANY;
    return with_trace_variant(ds.n_planes || ds.n_spheres, fd.flags & MR_MATH_PRODUCT, fd.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        const auto kern = any ? &frame_lights_kernel<VAR, true> : &frame_lights_kernel<VAR, false>;
        return launch_traversal(kern, trace_grid(a.eye.n), a.tp.stack_depth, stream, a);
    });
}

}  // namespace mr
