// mr_level_lights_path.hip -- ONE level of Scene::traceScene's recursion (Scene.cpp:270-346) of a PATH_TRACING build for a queue of
// rays in ONE launch on ANY scene (mr_trace_level_lights_path): mr_level_lights.hip's per-ray sequence --
//
//   Scene::trace, the bump-mapped normal included  ->  a ray that leaves the scene: getEnvironmentMap(ray), from the FULL image or,
//   for a ray made by Ray::random (ray.isDiffuse, Scene.cpp:678-681), from its 24-texel-wide low-res copy  ->  a hit: diffuseColor,
//   Phong::shade's loop over Scene::lights()  ->  times the ray's path weight, added to its pixel
//
// -- and then the children of mr_gen_path_rays_surface in place of those of mr_gen_secondary_rays: the PATH_TRACING build of
// Ray::reflect / getReflectionCoefficient / refract (Ray.h:149-158, 235-239) plus Ray::random's diffuse bounce (Ray.h:124-140),
// every one of them about the normal Scene::trace hands on -- the BUMPED one on stone -- and the diffuse child with weight x
// diffuseColor, the looked-up colour.  The batched route runs such a level as five launches,
//   mr_trace -> mr_shade_environment -> mr_hit_surface -> mr_shade_lights_surface -> mr_gen_path_rays_surface,
// which hand a hit record, a colour and a normal per ray on through HBM (40 bytes written and read back); here the lane keeps
// them.  Every piece is the shared definition those kernels call, under -ffp-contract=off: hit records, per-ray colour, normal and
// L are their bits, the children are the same set with the same ids, the pixel sums differ by the order of the float atomics
// (tests/test_level_lights_path.py compares level by level on the same queues).
//
// The queue carries what the path tracer's queues carry: stable ray ids (d_ids, NULL: the ray's index), from which a child's
// random numbers and its own id derive (rec::ChildGen<true>, rec::child_id), and one byte per ray that says whether Ray::random
// made it (d_lowres, or MR_ENV_LOWRES for the whole queue).  The kernel that generates the children knows each child's kind, so
// it writes that byte for the next level (d_out_lowres: 1 for kind 3): a diffuse bounce next to a refraction under an
// environment image, which the batched driver has to refuse, works here.
//
// The low-res copy (at most 24 x 96 texels) is read from global memory, not staged in LDS as shade_environment_kernel does: a
// miss of a diffuse ray fetches four 16-byte records of an image that stays in the L2, and the workgroup's LDS remains the
// traversal stack's.  The texels, and so the values, are the same either way (env_texels / env_blend on env.low with lw x lh).
// The environment, the texture table and the two masks are wave-uniform runtime branches, not template arguments.
//
// What it does NOT buy is what mr_level.hip's header says of its own level: the light loop and the generators run at the hit rate
// of the queue, where the batched calls stream compactly -- and diffuse bounce queues in open scenes hit rarely.  Times against
// the batched route: DESIGN section 5c, profiles/level_lights_path_ab.log.
//
// Live state is held down the way mr_level_lights.hip lists: the ray's direction is read again after the primary traversal, the
// shadow ray is rebuilt after its traversal, the weight and pixel are read after the light loop, the origin and the hit point
// are rebuilt for the children.  Unlike the specular form, which recomputes the object's own normal for its children, this form
// keeps the bumped normal and the colour across the light loop: six values.  Four waves per SIMD, as level_lights_kernel.
// d_out_count is zeroed by a one-word kernel of this unit, not a memset node (mr_level_lights.hip says why).
#include <hip/hip_runtime.h>

#include "mr_children_col.h"
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

struct LevelLightsPathArgs {
    TraceParams tp;              // scene arrays, root box; tp.rays = the queue, tp.n its length
    MeshMat m;
    TexParams t;                 // recs / mat_tex nullptr: the scene has no texture table
    EnvParams env;               // read with `environment` only; full nullptr: colour only (bg)
    const float *weights;        // rgb per ray or NULL (= 1)
    const uint32_t *pixels;      // pixel per ray or NULL (= ray index / spp)
    const uint32_t *ids;         // stable ray ids or NULL (= ray index)
    const uint8_t *lowres;       // per ray or NULL: non-zero = the ray is isDiffuse, a miss reads the low-res image
    uint32_t all_lowres;         // MR_ENV_LOWRES: every ray is
    uint32_t spp, environment;
    uint32_t hbase, bounce, kinds;
    float inv_spp;
    mr_hit *hits;                // optional: hit record of ray k
    float *ray_rgb;              // optional: the un-weighted L of ray k (a miss: 0, or the environment's value)
    float *color, *normal;       // optional: diffuseColor / the normal Scene::trace hands on of ray k's hit; a miss keeps its rows
    float *rgb;                  // may be NULL (then ray_rgb is not)
    ChildQueue out;              // CHILDREN == 0: not read
    uint8_t *out_lowres;         // optional: per stored child, 1 for the child of Ray::random (kind 3), 0 otherwise
    unsigned long long *counts;  // optional: [0] += rays, [1] += shadow rays, [2] += undefined texture lookups, [3] += misses,
                                 // [4] += undefined environment lookups
    uint32_t n_lights;
    ShadeLight lights[MR_MAX_LIGHTS];
};

#ifndef MIRO_LEVEL_LIGHTS_PATH_WAVES
#define MIRO_LEVEL_LIGHTS_PATH_WAVES 4
#endif

// env_lookup (the image a missing ray reads, full or low-res) and write_children_col (the children, the diffuse one with the
// looked-up colour, and their low-res bytes) are mr_children_col.h: the frame that emits level 1 ends in the same step.

// VAR: the traversal variant of trace_ray (mr_traverse.h) for the ray and its shadow rays; CHILDREN: 0 none, 1 path tracing.
// The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, int CHILDREN>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_LEVEL_LIGHTS_PATH_WAVES, 8))) void level_lights_path_kernel(
    const LevelLightsPathArgs a) {
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

    // whole workgroups run every iteration (n_round): the traversals, accumulate_runs and write_children_col are called by whole waves
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
                    const bool low = a.all_lowres || (a.lowres && a.lowres[k]);                // ray.isDiffuse (Scene.cpp:678-681)
                    if (!env_lookup(a.env, low, d[0], d[1], d[2], L)) my_env_undefined++;
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

        // ---- the children of the PATH_TRACING build (Scene.cpp:302-336, Ray::random), about the normal Scene::trace handed on and
        // with the looked-up colour, as mr_gen_path_rays_surface takes them; WHICH children exist is the material record's
        if (CHILDREN != 0) {
            ChildGen<true> g;
            bool emit[4] = {false, false, false, false};
            uint32_t id = 0;
            if (hit) {
                g.mt = mt;
                const bool refl = any_pos(g.mt + 3) && (a.kinds & 1u), refr = any_pos(g.mt + 6) && (a.kinds & 2u);
                const bool diff = any_pos(g.mt) && (a.kinds & 4u);
                if (refl || refr || diff) {
                    ra = rays[2 * k];
                    surface_point_od(a.m, ra.x, ra.y, ra.z, d[0], d[1], d[2], h.t, h.prim, h.beta, h.gamma, g.P, g.N);
                    g.N[0] = N[0]; g.N[1] = N[1]; g.N[2] = N[2];       // (the object's normal is overwritten before anything reads it)
                    g.d[0] = d[0]; g.d[1] = d[1]; g.d[2] = d[2];
                    g.w0[0] = w0[0]; g.w0[1] = w0[1]; g.w0[2] = w0[2];
                    id = a.ids ? a.ids[k] : (uint32_t)k;
                    g.hray = pcg32(a.hbase ^ id) + a.bounce * 4u;
                    g.plan(refl, refr, diff, emit);
                }
            }
            write_children_col<kTraceBlock>(a.out, a.out_lowres, g, col, emit, pix, id);
        }
    }

    // per-lane counts: one atomic per workgroup each; rays: the queue's length, added once
    if (a.counts) {
        const unsigned mine[4] = {my_shadow_rays, my_undefined, my_misses, my_env_undefined};
        workgroup_add<kTraceBlock>(mine, &a.counts[1]);
        if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.counts[0], n);
    }
}

// d_out_count = 0 on the launch's stream, as a kernel: a store from a kernel node replays from a graph as written
// (mr_level_lights.hip, zero_count_kernel)
__global__ void zero_path_count_kernel(unsigned long long *count) {
    if (threadIdx.x == 0) *count = 0ull;
}

template <int VAR, int CHILDREN>
mr_status launch_level_lights_path_t(const LevelLightsPathArgs &a, hipStream_t stream) {
    size_t lds = 0;
    const mr_status st = stack_lds(&level_lights_path_kernel<VAR, CHILDREN>, a.tp.stack_depth, kStackLdsShared, lds);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL((level_lights_path_kernel<VAR, CHILDREN>), dim3(trace_grid(a.tp.n)), dim3(kTraceBlock), lds, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace

mr_status launch_level_lights_path(const DeviceScene &ds, const TexParams &tex, const EnvParams &env, const ShadeLight *lights,
                                   uint32_t n_lights, const mr_level_lights_path_desc &ld, const mr_ray *d_rays, const float *d_weights,
                                   const uint32_t *d_pixels, const uint32_t *d_ids, unsigned long long n, float *d_rgb, mr_hit *d_hits,
                                   float *d_ray_rgb, float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights,
                                   uint32_t *d_out_pixels, uint32_t *d_out_ids, unsigned long long *d_out_count,
                                   unsigned long long *d_counts, hipStream_t stream) {
    if (ld.children != MR_LEVEL_LAST) {
        hipLaunchKernelGGL(zero_path_count_kernel, dim3(1), dim3(64), 0, stream, d_out_count);
        MR_HIP_CHECK(hipGetLastError());
    }
    if (n == 0) return MR_OK;
    LevelLightsPathArgs a;
    a.tp = scene_trace_params(ds);
    a.tp.rays = d_rays; a.tp.n = n;
    a.m = mesh_of(ds);
    a.t = tex;
    a.env = env;
    a.weights = d_weights; a.pixels = d_pixels; a.ids = d_ids; a.lowres = ld.d_lowres;
    a.all_lowres = (ld.flags & MR_ENV_LOWRES) ? 1u : 0u;
    a.spp = ld.spp; a.environment = ld.environment; a.inv_spp = 1.0f / (float)ld.spp;
    a.hbase = pcg32(ld.seed); a.bounce = ld.bounce; a.kinds = ld.path_kinds;
    a.hits = d_hits; a.ray_rgb = d_ray_rgb; a.color = d_color; a.normal = d_normal; a.rgb = d_rgb;
    a.out.rays = d_out_rays; a.out.weights = d_out_weights; a.out.pixels = d_out_pixels; a.out.ids = d_out_ids; a.out.count = d_out_count;
    a.out.capacity = ((unsigned long long)ld.out_capacity_hi << 32) | ld.out_capacity_lo;
    a.out.octants = ld.d_out_octants;
    a.out_lowres = ld.d_out_lowres;
    a.counts = d_counts;
    a.n_lights = n_lights;
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) a.lights[i] = lights[i < n_lights ? i : 0];

    // the traversal variants of launch_level_lights: the same hit records from each of them
    return with_trace_variant(ds.n_planes || ds.n_spheres, ld.flags & MR_MATH_PRODUCT, ld.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        return ld.children == MR_LEVEL_LAST ? launch_level_lights_path_t<VAR, 0>(a, stream) : launch_level_lights_path_t<VAR, 1>(a, stream);
    });
}

}  // namespace mr
