// mr_frame_lights_surface_body.h -- the body of frame_lights_surface_kernel (mr_frame_lights_surface.hip, where the kernel and
// its register figures are described) as a __device__ template, so that the frame that gives a ray that misses the scene's
// environment (mr_frame_lights_env.hip, mr_render_lights_environment) is the same code with one more step.  ENV says what a
// live sample whose primary ray misses is worth:
//   false  0 (m_bgColor = 0): mr_render_lights_surface
//   true   Scene::getEnvironmentMap(ray) (Scene.cpp:338-342, 657-688): bg_color, or the lookup of the full-resolution image at
//          the eye ray's direction (env_lookup_full, mr_environment_body.h; an eye ray is never isDiffuse, so the low-res copy
//          is not read).  The value is the sample's L: it goes to d_sample_rgb and into the pixel's butterfly as a hit's L does.
// The lookup lies between the primary traversal and the shadow traversals, on the lanes that missed, and writes into L, which
// is live across the light loop anyway; the eye ray's direction is computed again for it, as the hit arm computes it again.
// Colour or image is a wave-uniform branch on env.full.  Two counters more: live samples that missed, undefined lookups.
// With ENV false nothing of `env` is read and the code is the kernel's as it stood (the figures of
// tests/golden/kernel_budget_frame_lights_surface.json hold).  The arguments are taken BY VALUE (mr_lights_body.h says why).
// CHILDREN says whether the frame, being level 0 of Scene::traceScene's recursion, also emits the rays of level 1
// (mr_frame_level_lights.hip, mr_render_level_lights):
//   0  none: the two frames above; nothing of FrameChildArgs is read and the code is what it was (their records hold)
//   1  the reflect / Fresnel / refract children of mr_level_lights.hip's last step: rec::ChildGen<false>, rec::write_children,
//      about the normal of the surface step, the one Scene::trace hands on (the step bumps it on a STONE material only): the
//      object's own wherever no STONE material reflects, the bumped one on a reflective STONE (the children step says which
//      level kernels that matches)
//   2  the PATH_TRACING children of mr_level_lights_path.hip's last step: rec::ChildGen<true> about the normal of the surface
//      step (the bumped one on stone), the diffuse child with the looked-up colour, write_children_col -- the bumped normal and
//      the colour are the light loop's own
// In both the ray's origin is the eye, its path weight 1, its pixel row * W + x of this call's d_rgb, and (2) its id the sample
// index in the launch's own order.  The step stands between the surface step and the light loop, where all it reads is at hand.
// Included by the .hip units that instantiate it (everything here is local to its unit).
#pragma once

#include <hip/hip_runtime.h>

#include "mr_environment_body.h"
#include "mr_eye.h"
#include "mr_frame_window.h"
#include "mr_hit_surface_body.h"
#include "mr_children_col.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_light_loop.h"
#include "mr_noise.h"
#include "mr_phong.h"
#include "mr_recursion.h"
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
    float *sample_rgb;           // optional: the un-weighted L of sample k (a miss: 0, or the environment's value with ENV)
    float *sample_color;         // optional: diffuseColor of sample k's hit; a miss keeps what the buffer held
    float *sample_normal;        // optional: the normal Scene::trace hands on for sample k's hit; likewise
    float *rgb;                  // [rows * W][3], window rows in band order, image order inside a row
    unsigned long long *counts;  // optional: [0] += primary rays, [1] += shadow rays, [2] += hits whose lookup is undefined;
                                 // with ENV besides [3] += live samples that missed, [4] += undefined environment lookups
    uint32_t n_lights;
    ShadeLight lights[MR_MAX_LIGHTS];
};

// what every launcher of this frame puts into the block; `who`: the entry point the window's messages name
inline mr_status fill_frame_lights_surface_args(FrameLightsSurfaceArgs &a, const char *who, const LightScene &ls, const mr_frame_desc &fd,
                                                const FrameOutputs &o) {
    const mr_status st = frame_window_of(who, fd, a.eye);
    if (st != MR_OK) return st;
    a.tp = scene_trace_params(*ls.ds);
    a.tp.n = a.eye.n;
    a.m = mesh_of(*ls.ds);
    a.t = ls.tex;
    a.hits = o.hits; a.sample_rgb = o.sample_rgb; a.sample_color = o.sample_color; a.sample_normal = o.sample_normal;
    a.rgb = o.rgb; a.counts = o.counts;
    a.n_lights = ls.n_lights;
    for (uint32_t i = 0; i < MR_MAX_LIGHTS; i++) a.lights[i] = ls.lights[i < ls.n_lights ? i : 0];
    return MR_OK;
}

// the queue of level 1 (CHILDREN != 0)
struct FrameChildArgs {
    ChildQueue out;
    uint8_t *out_lowres;         // CHILDREN == 2, optional: per stored child, 1 for the child of Ray::random (kind 3), 0 otherwise
    uint32_t kinds, hbase;       // CHILDREN == 2: MR_PATH_* wanted, pcg32(path seed)
};
// the queue `out`, counted into d_out_count, as level 0's descriptor has it (out.low takes the place of ld.d_out_lowres)
inline void fill_frame_child_args(FrameChildArgs &ch, const mr_frame_level_desc &ld, const RayQueue &out, unsigned long long *d_out_count) {
    ch.out.rays = out.rays; ch.out.weights = out.weights; ch.out.pixels = out.pixels;
    ch.out.ids = ld.children == MR_LEVEL_PATH ? out.ids : nullptr;
    ch.out.count = d_out_count;
    ch.out.capacity = out_capacity_of(ld);
    ch.out.octants = ld.d_out_octants;
    ch.out_lowres = out.low;
    ch.kinds = ld.path_kinds; ch.hbase = pcg32(ld.path_seed);
}

// One pass of a frame of S samples per pixel (PASS; mr_frame_passes.hip): the launch renders samples [base, base + eye.spp) of every
// pixel of the window.  add: the pixel's lane adds its value to what rgb holds (a plain load, add and store) instead of storing it
struct PassParams {
    uint32_t S, base, add;
};

// VAR, ANY: as in frame_lights_kernel.  s_stack: the workgroup's dynamic LDS, [stack_depth][kTraceBlock]; s_tab: 128 words of
// static LDS for the two noise tables.
// LENS: the eye ray is Camera::eyeRay under -DDOF (eye_ray_lens_of, mr_eye.h; ln: the focus point and the aperture) -- the
// three places that make the eye ray make the lens ray, and the hit point of a sphere or a plane starts from the sample's own
// point on the lens, which is made again there, not held across the traversal.  With LENS false nothing of `ln` is read.
// PASS: the launch is one pass of a frame of ps.S samples per pixel, whose samples are numbered 0 .. S - 1 whatever the passes --
// the sample's random numbers are those of sample ps.base + sm (at the three places that make the ray), the path tracer's hash
// and the child's id come from the frame-wide index pixel * S + base + sm (the index a single launch at spp = S would give the
// sample; the window is in image order), the pixel's value is its lanes' sum times 1 / S, stored or added (ps.add).  With PASS
// false nothing of `ps` is read.
template <int VAR, bool ANY, bool ENV, int CHILDREN, bool LENS, bool PASS = false>
__device__ __forceinline__ void frame_lights_surface_body(const FrameLightsSurfaceArgs a, const EnvParams env, const FrameChildArgs &ch, const LensParams &ln,
                                                          int *s_stack, uint32_t (&s_tab)[128], const PassParams &ps = PassParams{}) {
    const NoiseTables nt = stage_noise_tables(s_tab);
    const int tid = threadIdx.x;
    const unsigned long long stride = (unsigned long long)gridDim.x * kTraceBlock;
    const unsigned long long n = a.eye.n;
    const unsigned long long n_round = whole_workgroups(n);
    const uint32_t spp = a.eye.spp;
    // the number the sample's key is made from
    auto key_sample = [&](uint32_t sm) -> uint32_t { if constexpr (PASS) return ps.base + sm; else return sm; };
    const bool table = a.t.mat_tex != nullptr;        // wave-uniform, out of the loop (hit_surface_kernel)
    Stats st = {0ull, 0ull};
    unsigned my_shadow_rays = 0, my_undefined = 0, my_misses = 0, my_env_undefined = 0;

    // whole workgroups run every iteration (n_round): the traversals, the butterfly and (CHILDREN) write_children are called
    // by whole waves
    for (unsigned long long idx = (unsigned long long)xcd_block_id() * kTraceBlock + tid; idx < n_round; idx += stride) {
        const bool live = idx < n;
        uint32_t x = 0, row = 0, y = 0, sm = 0;
        float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = make_float4(1.f, 1.f, 1.f, -1.f);
        if (live) {
            eye_sample_of(a.eye, idx, x, row, y, sm);
            if constexpr (LENS) eye_ray_lens_of(a.eye, ln, x, y, key_sample(sm), ra, rb);
            else eye_ray_of(a.eye, x, y, key_sample(sm), ra, rb);
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
            // (LENS: the sample's point on the lens and its direction, made again)
            if constexpr (LENS) {
                eye_sample_of(a.eye, idx, x, row, y, sm);
                eye_ray_lens_of(a.eye, ln, x, y, key_sample(sm), ra, rb);
                surface_od<true>(a.m.s, ra.x, ra.y, ra.z, rb.x, rb.y, rb.z, h.t, h.prim, h.beta, h.gamma, P, N);
            } else {
                surface_od<true>(a.m.s, a.eye.eye[0], a.eye.eye[1], a.eye.eye[2], rb.x, rb.y, rb.z, h.t, h.prim, h.beta, h.gamma, P, N);
            }
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
        // the eye ray's direction, computed again: cheaper than three registers live across the lookup.  With ENV a live lane
        // that missed needs it too (a lane past the end of the window is no miss)
        float d[3] = {0.f, 0.f, 0.f};
        if (ENV ? live : hit) {
            eye_sample_of(a.eye, idx, x, row, y, sm);
            if constexpr (LENS) eye_ray_lens_of(a.eye, ln, x, y, key_sample(sm), ra, rb);
            else eye_ray_of(a.eye, x, y, key_sample(sm), ra, rb);
            d[0] = rb.x; d[1] = rb.y; d[2] = rb.z;
        }

        // ---- the rays of level 1 (Scene.cpp:302-336): the last step of level_lights_kernel / level_lights_path_kernel for a ray
        // that starts at the eye with weight 1.  It stands HERE, before the light loop, not after the pixel's mean where the level
        // kernels have it: everything it reads is at hand (x and row are the sample's, computed just above), the children are a
        // set whose order is not part of the contract, and nothing of it -- the queue's arguments, the generators' state -- then
        // lives across the shadow traversals, where the registers are scarcest.  A lane past the end of the window has no pixel
        // and no children
        if (CHILDREN != 0) {
            const uint32_t pix = (ENV ? live : hit) ? row * a.eye.W + x : 0xFFFFFFFFu;
            // the sample's index in the launch's order, or (PASS) in the frame's: x, row and sm are the sample's, computed just above
            uint32_t id = (uint32_t)idx;
            if constexpr (PASS) id = (row * a.eye.W + x) * ps.S + ps.base + sm;
            ChildGen<CHILDREN == 2> g;
            bool emit[4] = {false, false, false, false};
            if (hit) {
                g.mt = mt;
                const bool refl = any_pos(g.mt + 3) && (CHILDREN == 1 || (ch.kinds & 1u));
                const bool refr = any_pos(g.mt + 6) && (CHILDREN == 1 || (ch.kinds & 2u));
                const bool diff = CHILDREN == 2 && any_pos(g.mt) && (ch.kinds & 4u);
                if (refl || refr || diff) {
                    // The hit point and the normal of the surface step, not rebuilt from the hit record.  P is surface_od's for this very ray and record: the bits
                    // surface_point_od(eye, d, h) gives the level kernels.  N is normalize3 of surface_od's normal, bumped before
                    // on a STONE material only (hit_color_normal): the normal Scene::trace hands on, which is what both builds'
                    // children bounce about (Ray.h:156).  CHILDREN == 2 asks for it on every scene.  For CHILDREN == 1 it is
                    // the level kernels' N on every scene too: where no STONE material reflects (mr_scene_set_textures:
                    // bumped_specular; none transmits) N is surface_point_od's normalize3 of the same three values wherever a
                    // child exists, and where one does the level kernels run their BUMPED form (mr_level_lights_body.h), which
                    // takes the surface step's N as this step does.
                    for (int c = 0; c < 3; c++) { g.P[c] = P[c]; g.N[c] = N[c]; }
                    g.d[0] = d[0]; g.d[1] = d[1]; g.d[2] = d[2];
                    g.w0[0] = 1.f; g.w0[1] = 1.f; g.w0[2] = 1.f;
                    if (CHILDREN == 2) g.hray = pcg32(ch.hbase ^ id);                          // bounce 0
                    g.plan(refl, refr, diff, emit);
                }
            }
            if constexpr (CHILDREN == 2)
                write_children_col<kTraceBlock>(ch.out, ch.out_lowres, g, col, emit, pix, id);
            else
                write_children<kTraceBlock, false>(ch.out, g, emit, pix, 0u);
        }

        // ---- Phong::shade over the light list (shade_light_list, mr_light_loop.h: shade_lights_body's loop with kColorSurface); a miss contributes nothing (m_bgColor = 0)
        // or, with ENV, what Scene::traceScene returns for it (Scene.cpp:338-342)
        float L[3] = {0.f, 0.f, 0.f};
        if (ENV) {
            if (live && !hit) {
                my_misses++;
                if (env.full) {                                        // wave-uniform
                    if (!env_lookup_full(env, d[0], d[1], d[2], L)) my_env_undefined++;
                } else {
                    L[0] = env.bg[0]; L[1] = env.bg[1]; L[2] = env.bg[2];                      // Scene.cpp:685
                }
            }
        }
        shade_light_list<VAR, ANY>(a.tp, a.m, a.lights, a.n_lights, hit, P, N, mt, col, d, s_stack, tid, st, L);
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
            const uint32_t mean_of = PASS ? ps.S : spp;
            if (mean_of > 1) {
                const float inv_spp = 1.0f / (float)mean_of;
                L[0] *= inv_spp; L[1] *= inv_spp; L[2] *= inv_spp;
            }
            float *o = a.rgb + 3 * ((size_t)row * a.eye.W + x);
            if (PASS && ps.add) { L[0] += o[0]; L[1] += o[1]; L[2] += o[2]; }
            o[0] = L[0]; o[1] = L[1]; o[2] = L[2];
        }
    }

    // rays traced, undefined lookups and misses.  Per-lane counts: one atomic per workgroup each; primary rays: the launch's
    // sample count, added once.
    if (a.counts) {
        workgroup_add<kTraceBlock>(my_shadow_rays, &a.counts[1]);
        workgroup_add<kTraceBlock>(my_undefined, &a.counts[2]);
        if (ENV) {
            workgroup_add<kTraceBlock>(my_misses, &a.counts[3]);
            workgroup_add<kTraceBlock>(my_env_undefined, &a.counts[4]);
        }
        if (blockIdx.x == 0 && tid == 0) atomicAdd(&a.counts[0], n);
    }
}

// the frames of the pinhole camera
template <int VAR, bool ANY, bool ENV, int CHILDREN>
__device__ __forceinline__ void frame_lights_surface_body(const FrameLightsSurfaceArgs a, const EnvParams env, const FrameChildArgs &ch, int *s_stack,
                                                          uint32_t (&s_tab)[128]) {
    const LensParams none = {};
    frame_lights_surface_body<VAR, ANY, ENV, CHILDREN, false>(a, env, ch, none, s_stack, s_tab);
}

// the two frames that stop at level 0
template <int VAR, bool ANY, bool ENV>
__device__ __forceinline__ void frame_lights_surface_body(const FrameLightsSurfaceArgs a, const EnvParams env, int *s_stack, uint32_t (&s_tab)[128]) {
    const FrameChildArgs none = {};
    frame_lights_surface_body<VAR, ANY, ENV, 0>(a, env, none, s_stack, s_tab);
}

}  // namespace
}  // namespace mr
