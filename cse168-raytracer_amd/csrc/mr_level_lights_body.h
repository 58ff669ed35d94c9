// mr_level_lights_body.h -- the body of level_lights_kernel (mr_level_lights.hip, mr_trace_level_lights) and of
// level_lights_path_kernel (mr_level_lights_path.hip, mr_trace_level_lights_path) as one __device__ template, with their argument
// blocks and what their launchers share: ONE level of Scene::traceScene's recursion (Scene.cpp:270-346) for a queue of rays in ONE
// launch on ANY scene -- the scene's light list, its texture table or none, its environment for rays that miss --
//
//   Scene::trace (Scene.cpp:278), the bump-mapped normal included  ->  a ray that leaves the scene: getEnvironmentMap(ray)
//   (Scene.cpp:338-342, 657-688)  ->  a hit: diffuseColor of a TexturedPhong, Phong::shade's loop over Scene::lights() -- per light
//   the shadow ray, Scene::trace, the occluder's light scale, the point or disc terms  ->  times the ray's path weight, added to
//   its pixel  ->  the children of the next level (Scene.cpp:302-336), compacted into the next queue
//
// One ray per lane.  PATH says which build of the reference the level is; the two differ in two steps only:
//   false  a miss reads the full image (env_lookup_full); the children are Ray::reflect / getReflectionCoefficient / refract:
//          rec::ChildGen<false>, rec::write_children (mr_level_lights.hip).  About which normal is BUMPED's to say (below)
//   true   a miss of a ray that is isDiffuse reads the low-res copy (env_lookup); the children are the PATH_TRACING build's, about
//          the normal Scene::trace hands on and with the looked-up colour: rec::ChildGen<true>, write_children_col
//          (mr_level_lights_path.hip).  Only this form reads the fields that LevelLightsPathArgs has besides.
// Every piece is the shared definition the batched route's five launches call, under -ffp-contract=off.  Those launches each
// stream the queue again and hand a hit record, a colour and a normal per ray on through HBM (40 bytes written and read back);
// here the lane keeps them in registers.  Hit records, per-ray colour, normal and L are their bits, the children are the same set,
// the pixel sums differ by the order of the float atomics.  The environment and the texture table are wave-uniform runtime
// branches (a.environment, then env.full; a.t.mat_tex), not template arguments, as in mr_frame_lights_env.hip.
//
// What it does NOT buy is what mr_level.hip's header says of its own level: the light loop and the generators run at the hit rate
// of the queue, where the batched calls stream compactly.
//
// Live state is held down the way the frame body does it: the ray's direction is read again after the primary traversal, the
// shadow ray is rebuilt after its traversal (shade_light_list), the weight and pixel are read after the light loop, the origin
// and the hit point are rebuilt for the children.
//
// The two argument blocks are flat near-copies on purpose: with the shared fields in a nested or a base struct every path kernel
// takes 32 bytes of scratch per lane or more.  The arguments are taken BY VALUE (mr_lights_body.h says why).
// Included by the .hip units that instantiate it (everything here is local to its unit).
#pragma once

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

struct LevelLightsPathArgs {
    TraceParams tp;              // as in LevelLightsArgs, field by field, with the path tracer's own between them
    MeshMat m;
    TexParams t;
    EnvParams env;
    const float *weights;
    const uint32_t *pixels;
    const uint32_t *ids;         // stable ray ids or NULL (= ray index)
    const uint8_t *lowres;       // per ray or NULL: non-zero = the ray is isDiffuse, a miss reads the low-res image
    uint32_t all_lowres;         // MR_ENV_LOWRES: every ray is
    uint32_t spp, environment;
    uint32_t hbase, bounce, kinds;
    float inv_spp;
    mr_hit *hits;
    float *ray_rgb;
    float *color, *normal;
    float *rgb;
    ChildQueue out;
    uint8_t *out_lowres;         // optional: per stored child, 1 for the child of Ray::random (kind 3), 0 otherwise
    unsigned long long *counts;
    uint32_t n_lights;
    ShadeLight lights[MR_MAX_LIGHTS];
};

// VAR: the traversal variant of trace_ray (mr_traverse.h) for the ray and its shadow rays; CHILDREN: 0 none, 1 the build's own.
// s_stack: the workgroup's dynamic LDS, [stack_depth][kTraceBlock]; s_tab: 128 words of static LDS for the two noise tables.
// QUEUED: where the queue's length comes from -- false: a.tp.n, the host knows it; true: n_queued, a wave-uniform word the kernel
// read from the device (mr_level_lights_queued.hip), and a.tp.n is not read.  A template argument and not a wrapper that hands
// a.tp.n on: a second by-value layer around the block moves it out of the scalar registers (mr_lights_body.h).
// BUMPED (read with PATH false and CHILDREN 1 only): about which normal the specular children bounce --
//   false  the object's own, rebuilt from the hit record with the hit point (surface_point_od): mr_gen_secondary_rays' bits.  The
//          launchers pick it on every scene without a reflective STONE material, where the surface step's N is that normal
//          wherever a child exists;
//   true   the surface step's N, the one Scene::trace hands on (Scene.cpp:234-263), as the PATH arm takes it: the bits
//          mr_gen_secondary_rays_surface reads from mr_hit_surface's buffer.  For a scene with bumped_specular
//          (mr_level_lights_bump.hip, mr_level_lights_queued_bump.hip).  N is live through the light loop either way.
template <int VAR, int CHILDREN, bool PATH, bool QUEUED = false, bool BUMPED = false, typename ARGS>
__device__ __forceinline__ void level_lights_body(const ARGS a, int *s_stack, uint32_t (&s_tab)[128], const unsigned long long n_queued = 0ull) {
    const NoiseTables nt = stage_noise_tables(s_tab);
    const int tid = threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTraceBlock;
    const unsigned long long n = QUEUED ? n_queued : a.tp.n;
    const unsigned long long n_round = whole_workgroups(n);
    const bool table = a.t.mat_tex != nullptr;        // wave-uniform, out of the loop (hit_surface_kernel)
    const float4 *rays = reinterpret_cast<const float4 *>(a.tp.rays);
    Stats st = {0ull, 0ull};
    unsigned my_shadow_rays = 0, my_undefined = 0, my_misses = 0, my_env_undefined = 0;

    // whole workgroups run every iteration (n_round): the traversals, accumulate_runs and write_children[_col] are called by whole waves
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
                    bool defined;
                    if constexpr (PATH) {
                        const bool low = a.all_lowres || (a.lowres && a.lowres[k]);            // ray.isDiffuse (Scene.cpp:678-681)
                        defined = env_lookup(a.env, low, d[0], d[1], d[2], L);
                    } else {
                        defined = env_lookup_full(a.env, d[0], d[1], d[2], L);
                    }
                    if (!defined) my_env_undefined++;
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

        // ---- the children (Scene.cpp:302-336; PATH: of the PATH_TRACING build, Ray::random's included).  WHICH children exist is
        // the material record's; PATH: and the call's (a.kinds)
        if (CHILDREN != 0) {
            ChildGen<PATH> g;
            bool emit[4] = {false, false, false, false};
            uint32_t id = 0, kinds = 3u;
            if constexpr (PATH) kinds = a.kinds;
            if (hit) {
                g.mt = mt;
                const bool refl = any_pos(g.mt + 3) && (kinds & 1u), refr = any_pos(g.mt + 6) && (kinds & 2u);
                const bool diff = PATH && any_pos(g.mt) && (kinds & 4u);
                if (refl || refr || diff) {
                    ra = rays[2 * k];
                    surface_point_od(a.m, ra.x, ra.y, ra.z, d[0], d[1], d[2], h.t, h.prim, h.beta, h.gamma, g.P, g.N);
                    g.d[0] = d[0]; g.d[1] = d[1]; g.d[2] = d[2];
                    g.w0[0] = w0[0]; g.w0[1] = w0[1]; g.w0[2] = w0[2];
                    if constexpr (PATH || BUMPED) {
                        g.N[0] = N[0]; g.N[1] = N[1]; g.N[2] = N[2];   // (the object's normal is overwritten before anything reads it)
                    }
                    if constexpr (PATH) {
                        id = a.ids ? a.ids[k] : (uint32_t)k;
                        g.hray = pcg32(a.hbase ^ id) + a.bounce * 4u;
                    }
                    g.plan(refl, refr, diff, emit);
                }
            }
            if constexpr (PATH) write_children_col<kTraceBlock>(a.out, a.out_lowres, g, col, emit, pix, id);
            else write_children<kTraceBlock, false>(a.out, g, emit, pix, id);
        }
    }

    // per-lane counts: one atomic per workgroup each; rays: the queue's length, added once
    if (a.counts) {
        const unsigned mine[4] = {my_shadow_rays, my_undefined, my_misses, my_env_undefined};
        workgroup_add<kTraceBlock>(mine, &a.counts[1]);
        if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.counts[0], n);
    }
}

// A queue whose length is a word on the device (mr_level_lights_queued.hip says why): the length, and whether this workgroup has
// a ray of it
__device__ __forceinline__ bool queued_length(const unsigned long long *d_n, unsigned long long n_cap, unsigned long long &n) {
    const unsigned long long have = *d_n;             // every lane, one address: wave-uniform
    n = have < n_cap ? have : n_cap;
    return (unsigned long long)xcd_block_id() * kTraceBlock < n;
}

// what every level launch puts into its block, of either build.  in: the queue the level reads, its first n rays (rays, weights,
// pixels; only read); out: the queue of its children (rays, weights, pixels, ids), counted into d_out_count; out_capacity,
// d_out_octants: the output queue's, as the level's descriptor names them
template <typename ARGS>
void fill_level_lights_args(ARGS &a, const LightScene &ls, uint32_t spp, uint32_t environment, const RayQueue &in, unsigned long long n,
                            float *d_rgb, mr_hit *d_hits, float *d_ray_rgb, float *d_color, float *d_normal, const RayQueue &out,
                            unsigned long long *d_out_count, unsigned long long out_capacity, uint8_t *d_out_octants,
                            unsigned long long *d_counts) {
    a.tp = scene_trace_params(*ls.ds);
    a.tp.rays = in.rays; a.tp.n = n;
    a.m = mesh_of(*ls.ds);
    a.t = ls.tex;
    a.env = ls.env;
    a.weights = in.weights; a.pixels = in.pixels;
    a.spp = spp; a.environment = environment; a.inv_spp = 1.0f / (float)spp;
    a.hits = d_hits; a.ray_rgb = d_ray_rgb; a.color = d_color; a.normal = d_normal; a.rgb = d_rgb;
    a.out.rays = out.rays; a.out.weights = out.weights; a.out.pixels = out.pixels; a.out.ids = out.ids; a.out.count = d_out_count;
    a.out.capacity = out_capacity;
    a.out.octants = d_out_octants;
    a.counts = d_counts;
    a.n_lights = ls.n_lights;
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) a.lights[i] = ls.lights[i < ls.n_lights ? i : 0];
}
// ... and what the PATH_TRACING build's block holds besides: the queue's ids and low-res bytes (every ray's with MR_ENV_LOWRES in
// `flags`), the children's generators and the low-res bytes of the output queue
inline void fill_level_lights_path_args(LevelLightsPathArgs &a, const uint32_t *d_ids, const uint8_t *d_lowres, uint32_t flags, uint32_t seed,
                                        uint32_t bounce, uint32_t path_kinds, uint8_t *d_out_lowres) {
    a.ids = d_ids; a.lowres = d_lowres;
    a.all_lowres = (flags & MR_ENV_LOWRES) ? 1u : 0u;
    a.hbase = pcg32(seed); a.bounce = bounce; a.kinds = path_kinds;
    a.out_lowres = d_out_lowres;
}

}  // namespace
}  // namespace mr
