// mr_level_lights.hip -- ONE level of Scene::traceScene's recursion (Scene.cpp:270-346) for a queue of rays in ONE launch on ANY
// scene (mr_trace_level_lights): the scene's light list, its texture table or none, its environment for rays that miss --
//
//   Scene::trace (Scene.cpp:278), the bump-mapped normal included  ->  a ray that leaves the scene: getEnvironmentMap(ray)
//   (Scene.cpp:338-342, 657-688)  ->  a hit: diffuseColor of a TexturedPhong, Phong::shade's loop over Scene::lights() -- per light
//   the shadow ray, Scene::trace, the occluder's light scale, the point or disc terms  ->  times the ray's path weight, added to
//   its pixel  ->  the children of the next level: Ray::reflect / getReflectionCoefficient / refract (Scene.cpp:302-336),
//   compacted into the next queue
//
// One ray per lane.  It joins two kernels: mr_level.hip's level (queue in, accumulate_runs, ChildGen<false>, write_children), which
// shades by one point light with the plain material table, and the per-sample body of the fused light-list frames
// (mr_frame_lights_surface_body.h: hit_color_normal, shade_light_list, env_lookup_full), which stops at the eye ray's hit.  The
// batched route runs such a level as five launches,
//   mr_trace -> mr_shade_environment -> mr_hit_surface -> mr_shade_lights_surface -> mr_gen_secondary_rays,
// each of which streams the queue again and hands a hit record, a colour and a normal per ray on through HBM (40 bytes written and
// read back); here the lane keeps them in registers.  Every piece is the shared definition those kernels call, under
// -ffp-contract=off: hit records, per-ray colour, normal and L are their bits, the children are the same set, the pixel sums
// differ by the order of the float atomics (tests/test_level_lights.py compares level by level on the same queues).
//
// The children bounce about the normal and material mr_gen_secondary_rays uses -- the object's own normal, normalised, not the
// bumped one; a stone material has ks = kt = 0 by rule and no children.  The environment is a wave-uniform runtime branch
// (a.environment, then env.full), not a template argument, as in mr_frame_lights_env.hip.  A specular child is never isDiffuse:
// the low-res image is not read.
//
// What it does NOT buy is what mr_level.hip's header says of its own level: the light loop and the generators run at the hit rate
// of the queue, where the batched calls stream compactly.  Times against the batched route: DESIGN section 5c,
// profiles/level_lights_ab.log.
//
// Live state is held down the way the frame body does it: the ray's direction is read again after the primary traversal, the
// shadow ray is rebuilt after its traversal (shade_light_list), the weight and pixel are read after the light loop, and the
// children's own normal is computed again from the hit record.  Four waves per SIMD, as every frame_lights_env_kernel: at six the
// specular level_kernel of mr_level.hip already spills 30 VGPRs without a light loop or a lookup.
#include <hip/hip_runtime.h>

#include "mr_environment_body.h"
#include "mr_hit_surface_body.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_light_loop.h"
#include "mr_noise.h"
#include "mr_phong.h"
#include "mr_recursion.h"
#include "mr_surface.h"
#include "mr_traverse.h"

namespace mr {
namespace {

using namespace rec;

struct LevelLightsArgs {
    TraceParams tp;              // scene arrays, root box; tp.rays = the queue, tp.n its length
    MeshMat m;
    TexParams t;                 // recs / mat_tex nullptr: the scene has no texture table
    EnvParams env;               // read with `environment` only; full nullptr: colour only (bg)
    const float *weights;        // rgb per ray or NULL (= 1)
    const uint32_t *pixels;      // pixel per ray or NULL (= ray index / spp)
    uint32_t spp, environment;
    float inv_spp;
    mr_hit *hits;                // optional: hit record of ray k
    float *ray_rgb;              // optional: the un-weighted L of ray k (a miss: 0, or the environment's value)
    float *color, *normal;       // optional: diffuseColor / the normal Scene::trace hands on of ray k's hit; a miss keeps its rows
    float *rgb;                  // may be NULL (then ray_rgb is not)
    ChildQueue out;              // CHILDREN == 0: not read
    unsigned long long *counts;  // optional: [0] += rays, [1] += shadow rays, [2] += undefined texture lookups, [3] += misses,
                                 // [4] += undefined environment lookups
    uint32_t n_lights;
    ShadeLight lights[MR_MAX_LIGHTS];
};

#ifndef MIRO_LEVEL_LIGHTS_WAVES
#define MIRO_LEVEL_LIGHTS_WAVES 4
#endif

// VAR: the traversal variant of trace_ray (mr_traverse.h) for the ray and its shadow rays; CHILDREN: 0 none, 1 specular.
// The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, int CHILDREN>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_LEVEL_LIGHTS_WAVES, 8))) void level_lights_kernel(
    const LevelLightsArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const int tid = threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTraceBlock;
    const unsigned long long n = a.tp.n;
    const unsigned long long n_round = whole_workgroups(n);
    const bool table = a.t.mat_tex != nullptr;        // wave-uniform, out of the loop (hit_surface_kernel)
    const float4 *rays = reinterpret_cast<const float4 *>(a.tp.rays);
    Stats st = {0ull, 0ull};
    unsigned my_shadow_rays = 0, my_undefined = 0, my_misses = 0, my_env_undefined = 0;

    // whole workgroups run every iteration (n_round): the traversals, accumulate_runs and write_children are called by whole waves
    for (unsigned long long k = (unsigned long long)xcd_block_id() * kTraceBlock + tid; k < n_round; k += stride) {
        const bool live = k < n;
        float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = make_float4(1.f, 1.f, 1.f, -1.f);
        if (live) { ra = rays[2 * k]; rb = rays[2 * k + 1]; }
        // ---- the ray (Scene.cpp:278): a closest hit; a lane past the end of the queue gets the miss record
        const mr_hit h = trace_hit<true, false, false, VAR>(a.tp, ra, rb, rb.w, live, s_stack, tid, st);
        if (a.hits && live) reinterpret_cast<float4 *>(a.hits)[k] = *reinterpret_cast<const float4 *>(&h);

        // ---- HitInfo::P, the normal as Scene::trace leaves it and diffuseColor: the surface pass's step for this hit
        const bool hit = live && h.prim != MR_MISS;
        float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 1.f, 0.f}, col[3] = {0.f, 0.f, 0.f};
        const float *mt = a.m.mats;
        if (hit) {
            surface_od<true>(a.m.s, ra.x, ra.y, ra.z, rb.x, rb.y, rb.z, h.t, h.prim, h.beta, h.gamma, P, N);
            bool ok = true;
            if (table) {
                hit_color_normal(a.m, a.t, nt, h.prim, P, N, col, ok);
            } else {
                TexParams t0 = a.t;
                t0.mat_tex = nullptr;
                hit_color_normal(a.m, t0, nt, h.prim, P, N, col, ok);
            }
            if (!ok) my_undefined++;
            if (a.color) { a.color[3 * k] = col[0]; a.color[3 * k + 1] = col[1]; a.color[3 * k + 2] = col[2]; }
            if (a.normal) { a.normal[3 * k] = N[0]; a.normal[3 * k + 1] = N[1]; a.normal[3 * k + 2] = N[2]; }
            mt = material_of(a.m, h.prim);
            my_shadow_rays += a.n_lights;
        }
        asm volatile("" ::: "memory");                   // the ray is read again rather than kept in registers across the lookup
        float d[3] = {0.f, 0.f, 0.f};
        if (live) {
            rb = rays[2 * k + 1];
            d[0] = rb.x; d[1] = rb.y; d[2] = rb.z;
        }

        // ---- a ray that leaves the scene (Scene.cpp:338-342): the environment's value, or 0 (m_bgColor = 0)
        float L[3] = {0.f, 0.f, 0.f};
        if (live && !hit) {
            my_misses++;
            if (a.environment) {                                       // wave-uniform
                if (a.env.full) {                                      // wave-uniform
                    if (!env_lookup_full(a.env, d[0], d[1], d[2], L)) my_env_undefined++;
                } else {
                    L[0] = a.env.bg[0]; L[1] = a.env.bg[1]; L[2] = a.env.bg[2];                // Scene.cpp:685
                }
            }
        }
        // ---- Phong::shade over the light list
        shade_light_list<VAR, false>(a.tp, a.m, a.lights, a.n_lights, hit, P, N, mt, col, d, s_stack, tid, st, L);
        if (a.ray_rgb && live) { a.ray_rgb[3 * k] = L[0]; a.ray_rgb[3 * k + 1] = L[1]; a.ray_rgb[3 * k + 2] = L[2]; }

        // ---- weight * L / spp to the ray's pixel: one add per ray, hit or miss
        uint32_t pix = 0xFFFFFFFFu;
        float w0[3] = {1.f, 1.f, 1.f};
        if (live) {
            pix = pixel_of(a.pixels, k, a.spp);
            weight_of(a.weights, k, w0);
        }
        if (a.rgb) {                                                   // wave-uniform
            float v[3] = {0.f, 0.f, 0.f};
            if (live)
                for (int c = 0; c < 3; c++) v[c] = L[c] * w0[c] * a.inv_spp;
            accumulate_runs(a.rgb, pix, v[0], v[1], v[2]);
        }

        // ---- the children (Scene.cpp:302-336), about the object's own normal as mr_gen_secondary_rays takes it
        if (CHILDREN != 0) {
            ChildGen<false> g;
            bool emit[4] = {false, false, false, false};
            if (hit) {
                g.mt = mt;
                const bool refl = any_pos(g.mt + 3), refr = any_pos(g.mt + 6);
                if (refl || refr) {
                    ra = rays[2 * k];
                    surface_point_od(a.m, ra.x, ra.y, ra.z, d[0], d[1], d[2], h.t, h.prim, h.beta, h.gamma, g.P, g.N);
                    g.d[0] = d[0]; g.d[1] = d[1]; g.d[2] = d[2];
                    g.w0[0] = w0[0]; g.w0[1] = w0[1]; g.w0[2] = w0[2];
                    g.plan(refl, refr, false, emit);
                }
            }
            write_children<kTraceBlock, false>(a.out, g, emit, pix, 0u);
        }
    }

    // per-lane counts: one atomic per workgroup each; rays: the queue's length, added once
    if (a.counts) {
        const unsigned mine[4] = {my_shadow_rays, my_undefined, my_misses, my_env_undefined};
        workgroup_add<kTraceBlock>(mine, &a.counts[1]);
        if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.counts[0], n);
    }
}

// d_out_count = 0 on the launch's stream, as a kernel.  mr_trace_level and the generators use hipMemsetAsync for this word; captured
// into a graph, that 8-byte memset node has been seen to fill the word with a wrong byte on replay (each byte 0x04 or 0x10
// instead of 0, depending on where the word lies in its allocation; the direct call is always right).  A store from a kernel node
// replays as written.
__global__ void zero_count_kernel(unsigned long long *count) {
    if (threadIdx.x == 0) *count = 0ull;
}

template <int VAR, int CHILDREN>
mr_status launch_level_lights_t(const LevelLightsArgs &a, hipStream_t stream) {
    size_t lds = 0;
    const mr_status st = stack_lds(&level_lights_kernel<VAR, CHILDREN>, a.tp.stack_depth, kStackLdsShared, lds);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL((level_lights_kernel<VAR, CHILDREN>), dim3(trace_grid(a.tp.n)), dim3(kTraceBlock), lds, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace

mr_status launch_level_lights(const DeviceScene &ds, const TexParams &tex, const EnvParams &env, const ShadeLight *lights,
                              uint32_t n_lights, const mr_level_lights_desc &ld, const mr_ray *d_rays, const float *d_weights,
                              const uint32_t *d_pixels, unsigned long long n, float *d_rgb, mr_hit *d_hits, float *d_ray_rgb,
                              float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                              unsigned long long *d_out_count, unsigned long long *d_counts, hipStream_t stream) {
    if (ld.children != MR_LEVEL_LAST) {
        hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(64), 0, stream, d_out_count);
        MR_HIP_CHECK(hipGetLastError());
    }
    if (n == 0) return MR_OK;
    LevelLightsArgs a;
    a.tp = scene_trace_params(ds);
    a.tp.rays = d_rays; a.tp.n = n;
    a.m = mesh_of(ds);
    a.t = tex;
    a.env = env;
    a.weights = d_weights; a.pixels = d_pixels;
    a.spp = ld.spp; a.environment = ld.environment; a.inv_spp = 1.0f / (float)ld.spp;
    a.hits = d_hits; a.ray_rgb = d_ray_rgb; a.color = d_color; a.normal = d_normal; a.rgb = d_rgb;
    a.out.rays = d_out_rays; a.out.weights = d_out_weights; a.out.pixels = d_out_pixels; a.out.ids = nullptr; a.out.count = d_out_count;
    a.out.capacity = ((unsigned long long)ld.out_capacity_hi << 32) | ld.out_capacity_lo;
    a.out.octants = ld.d_out_octants;
    a.counts = d_counts;
    a.n_lights = n_lights;
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) a.lights[i] = lights[i < n_lights ? i : 0];

    // the traversal variants of launch_level / launch_frame_lights_env: the same hit records from each of them
    return with_trace_variant(ds.n_planes || ds.n_spheres, ld.flags & MR_MATH_PRODUCT, ld.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        return ld.children == MR_LEVEL_LAST ? launch_level_lights_t<VAR, 0>(a, stream) : launch_level_lights_t<VAR, 1>(a, stream);
    });
}

}  // namespace mr
