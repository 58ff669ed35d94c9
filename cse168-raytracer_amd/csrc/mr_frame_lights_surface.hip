// mr_frame_lights_surface.hip -- mr_frame_lights.hip's frame on ANY scene (mr_render_lights_surface): the reference's per-pixel
// loop (Scene::raytraceImage, Scene.cpp:112-141) over the scene's light list as one launch, with what Scene::trace and
// Phong::shade do on a TexturedPhong in between:
//
//   Camera::eyeRay  ->  Scene::trace, which bump-maps the normal of a STONE hit and normalises (Scene.cpp:234-263)  ->
//   diffuseColor = the texture's lookup (Phong.cpp:51-56, all seven kinds)  ->  the loop over Scene::lights() (:59-156)  ->
//   the pixel's mean (Scene.cpp:126-139)
//
// It is frame_lights_kernel with a TexParams argument and one more step: between the primary trace and the light loop the
// per-hit step of the surface pass, hit_color_normal (mr_hit_surface_body.h), and then the loop of shade_lights_body
// (mr_lights_body.h) as its kColorSurface source runs it -- the colour where `dc` goes, the bumped normal everywhere N goes,
// the occluder's light scale from the occluder's own geometric normal (light_scale_of).  Every piece is the shared definition
// under -ffp-contract=off, called in the batched chain's order, so hit records, per-sample colour, normal and L and the pixels
// are the bits of mr_gen_eye_rays[_tiled] -> mr_trace -> mr_hit_surface -> mr_shade_lights_surface(d_ray_rgb) -> pairwise
// mean; tests/test_frame_lights_surface.py compares them.  That chain keeps 32 + 16 + 12 + 12 + 12 bytes per sample resident;
// this kernel writes 12 bytes per pixel (plus, on request, the hit record, L, colour and normal of every sample).
//
// Why the lookup may sit in a kernel that traverses (mr_procedural.hip's header says it may not): as in the photon walk on
// textured scenes, it lies BETWEEN two traversals.  Across it a lane keeps the sample index, the hit's primitive, P and N; the
// eye ray's direction is computed again after it (eye_sample_of / eye_ray_of give the same bits), as pixel and row are after
// the loop.  Across a shadow traversal a lane keeps what frame_lights_kernel keeps and the colour: three registers more.
// The 512 bytes of the two noise tables are static LDS beside the dynamic stack, staged once per workgroup
// (photon_walk_surface_kernel does the same).  hit_color_normal's test of mat_tex is taken out of the loop as
// hit_surface_kernel takes it out: without a texture table the plain arm alone runs, and the frame is mr_render_lights'.
//
// A miss contributes 0 (m_bgColor = 0), as in mr_render_lights: the environment (mr_shade_environment) needs the ray and hit
// buffers and stays with the batched route.
//
// Waves per SIMD, spilled VGPRs and scratch bytes per lane of the 12 kernels (hipcc, gfx950, the Makefile's flags); the
// envelope is the worst kernel of tests/golden/kernel_budget.json, 30 spilled VGPRs / 108 bytes / 4 waves, and every variant
// takes the most waves at which both of its shadow-ray forms stay inside it (frame_lights_surface_waves):
//
//   variant                     waves   closest-hit shadow rays   any-hit shadow rays
//   kTraceExact (1818)            4          0 / 100                  0 / 100
//   kTraceExactObj (826)          4          0 / 100                  0 / 100
//   kTraceProduct (267)           5          6 /  92                  4 /  84
//   kTraceProductObj (43)         4          0 / 100                  0 / 100
//   kTraceVote (88)               5          4 /  84                  4 /  84
//   kTraceVoteProduct (73)        5          5 /  88                  5 /  88
//
// One wave more is outside it: at five kTraceExact has 10 / 140, kTraceExactObj 14 / 156, kTraceProductObj 10 / 140 and 8 / 132;
// at six only the any-hit form of kTraceProduct (10 / 108) is inside.  Of the scratch figure 68 bytes (100 for the variants at
// four waves) are reported without a spilled VGPR, and the four-wave code holds no scratch instruction.  Carrying the eye
// ray's direction across the lookup instead of computing it again puts kTraceProduct at 120 / 116 bytes at five waves; one
// hit_color_normal call for both cases of mat_tex costs 2 to 4 more spilled VGPRs in every variant.  Times against the batched
// chain: DESIGN section 5c, profiles/frame_lights_surface_ab.log.
#include <hip/hip_runtime.h>

#include "mr_eye.h"
#include "mr_frame_window.h"
#include "mr_hit_surface_body.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_noise.h"
#include "mr_phong.h"
#include "mr_surface.h"
#include "mr_tile.h"
#include "mr_traverse.h"

namespace mr {
namespace {

using namespace rec;

struct FrameLightsSurfaceArgs {
    EyeFrame eye;
    TraceParams tp;              // scene arrays, root box; rays / hits / n unused
    MeshMat m;
    TexParams t;                 // recs / mat_tex nullptr: the scene has no texture table
    mr_hit *hits;                // optional: primary hit record of sample k
    float *sample_rgb;           // optional: the un-weighted L of sample k (0 for a miss)
    float *sample_color;         // optional: diffuseColor of sample k's hit; a miss keeps what the buffer held
    float *sample_normal;        // optional: the normal Scene::trace hands on for sample k's hit; likewise
    float *rgb;                  // [rows * W][3], window rows in band order, image order inside a row
    unsigned long long *counts;  // optional: [0] += primary rays, [1] += shadow rays, [2] += hits whose lookup is undefined
    uint32_t n_lights;
    ShadeLight lights[MR_MAX_LIGHTS];
};

// MIRO_FRAME_LIGHTS_SURFACE_WAVES (A/B builds) sets one value for every variant.
#ifdef MIRO_FRAME_LIGHTS_SURFACE_WAVES
constexpr int frame_lights_surface_waves(int) { return MIRO_FRAME_LIGHTS_SURFACE_WAVES; }
#else
constexpr int frame_lights_surface_waves(int var) { return var == kTraceProduct || var == kTraceVote || var == kTraceVoteProduct ? 5 : 4; }
#endif

// VAR, ANY: as in frame_lights_kernel.  The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(frame_lights_surface_waves(VAR), 8))) void frame_lights_surface_kernel(
    const FrameLightsSurfaceArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const int tid = threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTraceBlock;
    const unsigned long long n = a.eye.n;
    const unsigned long long n_round = whole_workgroups(n);
    const uint32_t spp = a.eye.spp;
    const bool table = a.t.mat_tex != nullptr;        // wave-uniform, out of the loop (hit_surface_kernel)
    Stats st = {0ull, 0ull};
    unsigned my_shadow_rays = 0, my_undefined = 0;

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

        // ---- HitInfo::P, the normal as Scene::trace leaves it and diffuseColor: the surface pass's step for this hit
        const bool hit = live && h.prim != MR_MISS;
        float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 1.f, 0.f}, col[3] = {0.f, 0.f, 0.f};
        const float *mt = a.m.mats;
        if (hit) {
            // the ray's origin is the eye (a hit lane is a live one): read from the arguments, uniform, where it is used
            surface_od<true>(a.m.s, a.eye.eye[0], a.eye.eye[1], a.eye.eye[2], rb.x, rb.y, rb.z, h.t, h.prim, h.beta, h.gamma, P, N);
            bool ok = true;
            if (table) {
                hit_color_normal(a.m, a.t, nt, h.prim, P, N, col, ok);
            } else {
                TexParams t0 = a.t;
                t0.mat_tex = nullptr;
                hit_color_normal(a.m, t0, nt, h.prim, P, N, col, ok);
            }
            if (!ok) my_undefined++;
            if (a.sample_color) { a.sample_color[3 * idx] = col[0]; a.sample_color[3 * idx + 1] = col[1]; a.sample_color[3 * idx + 2] = col[2]; }
            if (a.sample_normal) { a.sample_normal[3 * idx] = N[0]; a.sample_normal[3 * idx + 1] = N[1]; a.sample_normal[3 * idx + 2] = N[2]; }
            mt = material_of(a.m, h.prim);
            my_shadow_rays += a.n_lights;
        }
        // the eye ray's direction, computed again: cheaper than three registers live across the lookup
        float d[3] = {0.f, 0.f, 0.f};
        if (hit) {
            eye_sample_of(a.eye, idx, x, row, y, sm);
            eye_ray_of(a.eye, x, y, sm, ra, rb);
            d[0] = rb.x; d[1] = rb.y; d[2] = rb.z;
        }

        // ---- Phong::shade over the light list (shade_lights_body with kColorSurface); a miss contributes nothing (m_bgColor = 0)
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
                        lit = disc_terms(lt, mt, col, P, N, l, d[0], d[1], d[2], diffuse, highlight);
                    } else {
                        phong_terms(lt.position, lt.color, lt.wattage, mt, col, P, N, d[0], d[1], d[2], diffuse, highlight);
                    }
                }
                if (lit) phong_combine(diffuse, highlight, scale, out);
                L[0] += out[0]; L[1] += out[1]; L[2] += out[2];
            }
        }
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

    // rays traced and undefined lookups.  Per-lane counts: one atomic per workgroup each; primary rays: the launch's sample
    // count, added once.
    if (a.counts) {
        workgroup_add<kTraceBlock>(my_shadow_rays, &a.counts[1]);
        workgroup_add<kTraceBlock>(my_undefined, &a.counts[2]);
        if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.counts[0], n);
    }
}

}  // namespace

mr_status launch_frame_lights_surface(const DeviceScene &ds, const TexParams &tex, const ShadeLight *lights, uint32_t n_lights,
                                      const mr_frame_desc &fd, float *d_rgb, mr_hit *d_hits, float *d_sample_rgb, float *d_sample_color,
                                      float *d_sample_normal, unsigned long long *d_counts, hipStream_t stream) {
    FrameLightsSurfaceArgs a;
    const mr_status st = frame_window_of("mr_render_lights_surface", fd, a.eye);
    if (st != MR_OK) return st;
    if (a.eye.n == 0) return MR_OK;
    a.tp = scene_trace_params(ds);
    a.tp.n = a.eye.n;
    a.m = mesh_of(ds);
    a.t = tex;
    a.hits = d_hits; a.sample_rgb = d_sample_rgb; a.sample_color = d_sample_color; a.sample_normal = d_sample_normal;
    a.rgb = d_rgb; a.counts = d_counts;
    a.n_lights = n_lights;
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) a.lights[i] = lights[i < n_lights ? i : 0];

    // the traversal variants of launch_frame_lights: the same hit records from each of them
    const bool any = fd.flags & MR_TRACE_ANY;
    return with_trace_variant(ds.n_planes || ds.n_spheres, fd.flags & MR_MATH_PRODUCT, fd.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        const auto kern = any ? &frame_lights_surface_kernel<VAR, true> : &frame_lights_surface_kernel<VAR, false>;
        size_t lds = 0;
        const mr_status ls = stack_lds(kern, a.tp.stack_depth, kStackLdsShared, lds);
        if (ls != MR_OK) return ls;
        hipLaunchKernelGGL(kern, dim3(trace_grid(a.eye.n)), dim3(kTraceBlock), lds, stream, a);
        MR_HIP_CHECK(hipGetLastError());
        return MR_OK;
    });
}

}  // namespace mr
