// mr_children_body.h -- the body of children_kernel (mr_bounce.hip, where the kernels are listed) as a __device__ template, so
// that the surface-pass form of the PATH_TRACING generators (mr_path_surface.hip) is the same two passes with two loads per
// listed ray, the way mr_lights_body.h / mr_square_body.h serve the shading kernels.  SRC (ColorSource, mr_texture.h) says where a
// hit's N and the diffuse child's colour come from:
//   kColorMaterial  the object's normal, computed here, and the material's own m_diffuse (mr_gen_secondary_rays, mr_gen_path_rays)
//   kColorSurface   both loaded from the surface pass's per-ray buffers (mr_hit_surface): N as Scene::trace hands it on
//                   (Scene.cpp:234-263), bumped on a STONE material, for BOTH passes and every generator -- Ray::reflect, the
//                   Fresnel term, Ray::refract, Ray::random -- and diffuseColor (Phong.cpp:51-56) as the diffuse child's factor,
//                   what Scene::tracePhoton carries on (Scene.cpp:545-553, :608).  P is still rebuilt from ray and hit.  WHICH
//                   children a hit has stays the material record's (isDiffuse / isReflective / isRefractive): a diffuse child
//                   whose looked-up colour is 0 is emitted with weight 0, so the counts do not depend on the texture.
// Every source calls surface_point, as in mr_accumulate_body.h: the N it would compute is overwritten from the buffer before
// anything reads it, so no code is generated for it.  Both buffers are read for LISTED rays only -- a listed ray has a hit, and
// mr_hit_surface leaves the six floats of a miss untouched -- with three scalar float loads per vector (12-byte stride).
// rec::ChildGen is shared with mr_level.hip and stays as it is: the surface form fills g.N itself and replaces the diffuse
// child's weight after make() (write_children_col_at below).  The arguments are taken BY VALUE, as in mr_lights_body.h: either
// way the existing kernels keep their registers, scratch and waves (one pair of spilled SGPRs fewer in children_kernel<true>),
// by value with fewer instructions; the two buffers are kernel arguments of their own, so that the plain kernels' argument
// block is what it was.
// Included by the .hip units that instantiate it (everything here is local to its unit).
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_recursion.h"
#include "mr_texture.h"

namespace mr {
namespace {

struct BounceArgs {
    rec::MeshMat m;
    const mr_ray *rays;
    const mr_hit *hits;
    const float *weights;
    const uint32_t *pixels;
    const uint32_t *ids;          // path tracing: stable id per ray (NULL: the ray's index); children get ids derived from it
    uint32_t spp, hbase, bounce, kinds;
    unsigned long long n;
    rec::ChildQueue out;
};

// what launch_path_rays and its surface-pass form fill in the same way
inline BounceArgs path_args_of(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                               const uint32_t *d_pixels, const uint32_t *d_ids, unsigned long long n, uint32_t spp, uint32_t seed,
                               uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                               uint32_t *d_out_ids, unsigned long long *d_count, unsigned long long out_capacity, uint8_t *d_out_octants) {
    BounceArgs a;
    a.m = rec::mesh_of(ds); a.rays = d_rays; a.hits = d_hits; a.weights = d_weights; a.pixels = d_pixels; a.ids = d_ids;
    a.spp = spp; a.bounce = bounce; a.kinds = kinds; a.n = n;
    a.hbase = pcg32(seed);
    a.out.rays = d_out_rays; a.out.weights = d_out_weights; a.out.pixels = d_out_pixels; a.out.ids = d_out_ids; a.out.count = d_count; a.out.capacity = out_capacity; a.out.octants = d_out_octants;
    return a;
}

// A workgroup takes chunks of kGenIter * kBlock rays: it first lists the rays of the chunk that have children at all (a hit
// on a material with the wanted terms) in LDS, in ray order, counts their children, reserves the chunk's output slots with
// one atomic, then generates from the list with full waves.  Run straight
// over the rays the generators work at the hit rate of the queue -- the diffuse bounce rays of an open scene hit something
// 2 % of the time, nearly every wave still holds a hit, and the launch cost what the dense first level costs.
constexpr int kGenIter = 8;

#ifndef MIRO_CHILDREN_WAVES
#define MIRO_CHILDREN_WAVES 5      /* 90 registers, no spill; unconstrained the scheduler took 160 (3 waves) for the same speed */
#endif

// ray k's N as the generators take it: kColorSurface replaces surface_point's.  Pass 1 and pass 2 both come through here, so
// that they decide a refractive hit's Fresnel child (plan(): Rs > 0.01) from the same bits -- if they decided differently, one
// ray's children would land in another ray's slots.
template <ColorSource SRC>
__device__ __forceinline__ void child_normal(const float *normal, unsigned long long k, float N[3]) {
    if (SRC == kColorSurface) { N[0] = normal[3 * k]; N[1] = normal[3 * k + 1]; N[2] = normal[3 * k + 2]; }
}

// rec::write_children_at whose diffuse child (kind 3) carries w0 * col instead of make()'s w0 * m_diffuse
template <bool PATH>
__device__ __forceinline__ void write_children_col_at(const rec::ChildQueue &q, const rec::ChildGen<PATH> &g, const float col[3],
                                                      const bool emit[4], uint32_t pix, uint32_t id, unsigned long long s) {
    constexpr int NK = PATH ? 4 : 3;
#pragma unroll
    for (int j = 0; j < NK; j++) {
        if (emit[j]) {
            if (s < q.capacity) {
                float org[3], dir[3], wgt[3];
                g.make(j, org, dir, wgt);
                if (j == 3)
                    for (int c = 0; c < 3; c++) wgt[c] = g.w0[c] * col[c];
                reinterpret_cast<float4 *>(q.rays)[2 * s] = make_float4(org[0], org[1], org[2], 0.0f);
                reinterpret_cast<float4 *>(q.rays)[2 * s + 1] = make_float4(dir[0], dir[1], dir[2], 1e12f);
                q.weights[3 * s] = wgt[0]; q.weights[3 * s + 1] = wgt[1]; q.weights[3 * s + 2] = wgt[2];
                q.pixels[s] = pix;
                if (q.ids) q.ids[s] = rec::child_id(id, j);
                if (q.octants) q.octants[s] = rec::octant_of(dir);
            }
            s++;
        }
    }
}

// PATH = false: Ray::reflect / getReflectionCoefficient / refract (Ray.h:143-243) for every hit on a reflective or
// refractive material, up to three children per ray.  PATH = true: the PATH_TRACING build of those generators plus
// Ray::random's diffuse bounce (an EXTENSION: the reference defines Ray::random but traceScene at HEAD never calls it,
// SURVEY.md section 8d, config 3), up to four.
// color, normal: three floats per ray each, read by kColorSurface only
template <bool PATH, ColorSource SRC>
__device__ __forceinline__ void children_body(const BounceArgs a, const float *color, const float *normal) {
    using namespace rec;
    __shared__ unsigned s_list[kGenIter * kBlock];            // offsets into the chunk
    __shared__ unsigned s_cnt[kGenIter][kBlock / 64];
    __shared__ unsigned s_slot[kGenIter * kBlock];            // per listed ray: (children of earlier lanes of its wave << 3) | its own
    __shared__ unsigned long long s_chunk_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long chunk = (unsigned long long)kBlock * kGenIter;
    const unsigned long long n_chunks = (a.n + chunk - 1) / chunk;
    for (unsigned long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {      // uniform per workgroup
        const unsigned long long base = c * chunk;
        unsigned long long wants[kGenIter];
#pragma unroll
        for (int it = 0; it < kGenIter; it++) {
            const unsigned long long k = base + (unsigned long long)it * kBlock + threadIdx.x;
            bool want = false;
            if (k < a.n) {
                const uint32_t prim = __float_as_uint(reinterpret_cast<const float4 *>(a.hits)[k].y);
                if (prim != MR_MISS) {
                    const float *mt = material_of(a.m, prim);
                    want = (any_pos(mt + 3) && (!PATH || (a.kinds & 1u))) || (any_pos(mt + 6) && (!PATH || (a.kinds & 2u))) ||
                           (PATH && any_pos(mt) && (a.kinds & 4u));
                }
            }
            wants[it] = __ballot(want);
            if (lane == 0) s_cnt[it][wave] = (unsigned)__popcll(wants[it]);
        }
        __syncthreads();
        unsigned listed = 0;
#pragma unroll
        for (int it = 0; it < kGenIter; it++) {
            unsigned at = listed;
            for (int w = 0; w < kBlock / 64; w++) {
                const unsigned cw = s_cnt[it][w];
                if (w < wave) at += cw;
                listed += cw;
            }
            if ((wants[it] >> lane) & 1ull)
                s_list[at + (unsigned)__popcll(wants[it] & ((1ull << lane) - 1ull))] = (unsigned)(it * kBlock) + threadIdx.x;
        }
        __syncthreads();
        // Two passes over the list, so that the whole chunk takes ONE reservation: a single counter word drains ~88 atomics
        // per microsecond, and one atomic per 256 listed rays (65 k for the 16.8 M rays of a bunny frame) was what the launch
        // took -- 0.75 ms of atomics around 0.4 ms of work.
        // pass 1: how many children each listed ray has.  Without refraction that is the material alone; a refractive hit
        // needs its Fresnel term (the hit point is rebuilt again in pass 2 -- for those rays only).
        const int rounds = (int)((listed + kBlock - 1) / kBlock);
        for (int it = 0; it < kGenIter; it++) {              // (not unrolled: the generators would be inlined eight times)
            if (it >= rounds) { if (lane == 63) s_cnt[it][wave] = 0; continue; }
            const unsigned j = (unsigned)it * kBlock + threadIdx.x;
            unsigned cnt = 0;
            if (j < listed) {
                const unsigned long long k = base + s_list[j];
                const float4 h = reinterpret_cast<const float4 *>(a.hits)[k];
                const uint32_t prim = __float_as_uint(h.y);
                const float *mt = material_of(a.m, prim);
                const bool refl = any_pos(mt + 3) && (!PATH || (a.kinds & 1u)), refr = any_pos(mt + 6) && (!PATH || (a.kinds & 2u));
                const bool diff = PATH && any_pos(mt) && (a.kinds & 4u);
                cnt = (refl ? 1u : 0u) + (diff ? 1u : 0u);
                if (refr) {
                    ChildGen<PATH> g;
                    bool emit[4];
                    g.mt = mt;
                    surface_point(a.m, a.rays, k, h, g.P, g.N);
                    child_normal<SRC>(normal, k, g.N);
                    const float4 rb = reinterpret_cast<const float4 *>(a.rays)[2 * k + 1];
                    g.d[0] = rb.x; g.d[1] = rb.y; g.d[2] = rb.z;
                    g.plan(refl, refr, diff, emit);
                    cnt += 1u + (emit[1] ? 1u : 0u);
                }
            }
            unsigned incl = cnt;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            if (j < listed) s_slot[j] = ((incl - cnt) << 3) | cnt;      // children of earlier lanes of my wave | my own
            if (lane == 63) s_cnt[it][wave] = incl;          // s_cnt is free again: the list is complete
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned tot = 0;
            for (int it = 0; it < kGenIter; it++)
                for (int w = 0; w < kBlock / 64; w++) tot += s_cnt[it][w];
            s_chunk_base = tot ? atomicAdd(a.out.count, (unsigned long long)tot) : 0ull;
        }
        __syncthreads();
        // pass 2: generate, every ray's children next to one another
        unsigned long long round_base = s_chunk_base;
        for (int it = 0; it < rounds; it++) {
            unsigned before = 0, round_total = 0;
            for (int w = 0; w < kBlock / 64; w++) {
                const unsigned cw = s_cnt[it][w];
                if (w < wave) before += cw;
                round_total += cw;
            }
            const unsigned j = (unsigned)it * kBlock + threadIdx.x;
            const unsigned mine = j < listed ? s_slot[j] : 0u;
            if (mine & 7u) {
                const unsigned long long k = base + s_list[j];
                ChildGen<PATH> g;
                bool emit[4] = {false, false, false, false};
                const float4 h = reinterpret_cast<const float4 *>(a.hits)[k];
                const uint32_t prim = __float_as_uint(h.y);
                g.mt = material_of(a.m, prim);
                const bool refl = any_pos(g.mt + 3) && (!PATH || (a.kinds & 1u)), refr = any_pos(g.mt + 6) && (!PATH || (a.kinds & 2u));
                const bool diff = PATH && any_pos(g.mt) && (a.kinds & 4u);
                surface_point(a.m, a.rays, k, h, g.P, g.N);
                child_normal<SRC>(normal, k, g.N);
                const float4 rb = reinterpret_cast<const float4 *>(a.rays)[2 * k + 1];
                g.d[0] = rb.x; g.d[1] = rb.y; g.d[2] = rb.z;
                weight_of(a.weights, k, g.w0);
                const uint32_t pix = pixel_of(a.pixels, k, a.spp);
                uint32_t id = 0;
                if (PATH) {
                    id = a.ids ? a.ids[k] : (uint32_t)k;
                    g.hray = pcg32(a.hbase ^ id) + a.bounce * 4u;
                }
                g.plan(refl, refr, diff, emit);
                const unsigned long long slot = round_base + before + (mine >> 3);
                if (SRC == kColorSurface) {
                    float col[3] = {0.f, 0.f, 0.f};
                    if (emit[3]) { col[0] = color[3 * k]; col[1] = color[3 * k + 1]; col[2] = color[3 * k + 2]; }
                    write_children_col_at<PATH>(a.out, g, col, emit, pix, id, slot);
                } else {
                    write_children_at<PATH>(a.out, g, emit, pix, id, slot);
                }
            }
            round_base += round_total;
        }
        __syncthreads();                                                             // s_list / s_cnt are reused by the next chunk
    }
}

}  // namespace
}  // namespace mr
