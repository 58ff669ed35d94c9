// mr_photon_walk_body.h -- the photon walk itself (Scene::tracePhoton, Scene.cpp:529-655, per emitted photon of one
// DirectionalAreaLight), written once for its two kernels:
//
//   photon_walk_kernel<VAR>           (mr_photon_walk.hip)          photon_walk_body<VAR, WalkMaterialSource>
//   photon_walk_surface_kernel<VAR>   (mr_photon_walk_surface.hip)  photon_walk_body<VAR, WalkSurfaceSource>
//
// One lane owns one photon for its whole life: emission (sampleDisc, Utility.h:82-95) -> Scene::trace -> the roulette over
// the averages of the hit's diffuse colour and the material's ks / kt -> store / absorb / the next segment (Ray::random,
// Ray::reflect, the Fresnel draw, Ray::refract).  Origin, direction, power, emission index and depth stay in registers
// between bounces; the traversal is trace_ray (mr_traverse.h) with the default exact arithmetic, so every hit is the record
// mr_trace returns for the same segment.  Lanes whose photon has died re-arm from the round's emission counter between
// whole segments: wave64 ballot + prefix sum, one atomic per wave.  Everything a photon does is keyed by its emission index
// (random numbers, record slots), never by the lane that walks it.
//
// The source policy SRC says where a hit's diffuse colour, point and normal come from.  It is asked twice per hit:
//   color(a, o, d, h, mt)   for every hit, before the roulette: the colour whose average is prob[0] (Scene.cpp:545-551)
//   point(a, o, d, h, P, N) for a hit that survives rnd > prob[2]: HitInfo::P and HitInfo::N as Scene::trace leaves them
// The arguments and the source travel BY VALUE, as in mr_lights_body.h (DESIGN section 4 records why).
// Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_recursion.h"
#include "mr_traverse.h"

namespace mr {
namespace {

using namespace rec;

constexpr uint32_t kNoPhoton = 0xFFFFFFFFu;
constexpr int kDiscAttempts = 64;             // sampleDisc's rejection loop, bounded: (1 - pi/4)^64 ~ 1e-43, then the centre

struct WalkArgs {
    TraceParams tp;
    MeshMat m;
    float pos[3], dir[3], t1[3], t2[3], power[3], radius;
    uint32_t hdir, hevent, hdisc;             // pcg32 of the seed in its three domains (directions, events, disc)
    uint32_t caustic, max_depth;
    uint32_t first, count;                    // the round: emissions first ... first + count - 1
    float4 *slots;                            // count * max_depth records of 3 float4
    uint32_t *words;                          // count packed words
    unsigned *next;                           // the round's emission counter (zeroed by the host)
};

// the arguments of one round's walk, whichever kernel walks it
inline WalkArgs walk_args_of(const DeviceScene &ds, const PhotonWalkLight &lt, uint32_t seed, uint32_t caustic, uint32_t max_depth,
                             uint32_t first, uint32_t count, const PhotonRoundBuffers &b) {
    WalkArgs a;
    a.tp = scene_trace_params(ds);
    a.tp.n = count;
    a.m = mesh_of(ds);
    for (int c = 0; c < 3; c++) { a.pos[c] = lt.position[c]; a.dir[c] = lt.direction[c]; a.t1[c] = lt.t1[c]; a.t2[c] = lt.t2[c]; a.power[c] = lt.power[c]; }
    a.radius = lt.radius;
    a.hdir = pcg32(seed); a.hevent = pcg32(seed ^ kPhotonEventDomain); a.hdisc = pcg32(seed ^ kPhotonDiscDomain);
    a.caustic = caustic; a.max_depth = max_depth; a.first = first; a.count = count;
    a.slots = b.slots; a.words = b.words; a.next = b.next;
    return a;
}

// the launch both kernels share: dynamic LDS stacks, and a resident grid -- every wave keeps pulling emissions until the
// round is handed out (the occupancy query behind resident_grid counts the kernel's static LDS with the stacks)
template <typename K, typename... Extra>
mr_status launch_walk(K kern, const WalkArgs &a, hipStream_t stream, Extra... extra) {
    size_t lds = 0;
    unsigned grid = 1;
    mr_status st = stack_lds(kern, a.tp.stack_depth, kStackLdsShared, lds);
    if (st == MR_OK) st = resident_grid(kern, lds, ((unsigned long long)a.count + kTraceBlock - 1) / kTraceBlock, grid);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kTraceBlock), lds, stream, a, extra...);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

// state word of a lane: depth (bits 0-7), stores (8-15), first bounce specular (16)
__device__ __forceinline__ float avg3(const float *c) { return ((c[0] + c[1]) + c[2]) / 3.0f; }      // Vector3::average

// the plain walk's source: the material's own kd, read where it is used, and the geometric normal, normalised
struct WalkMaterialSource {
    const float *col;
    __device__ __forceinline__ void color(const WalkArgs &a, const float o[3], const float d[3], const mr_hit &h, const float *mt) { col = mt; }
    __device__ __forceinline__ void point(const WalkArgs &a, const float o[3], const float d[3], const mr_hit &h, float P[3], float N[3]) const {
        surface_point_od(a.m, o[0], o[1], o[2], d[0], d[1], d[2], h.t, h.prim, h.beta, h.gamma, P, N);
    }
};

template <int VAR, typename SRC>
__device__ __forceinline__ void photon_walk_body(WalkArgs a, SRC src) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    const int tid = threadIdx.x, lane = tid & 63;
    Stats st = {0ull, 0ull};

    uint32_t my = kNoPhoton, state = 0;               // local emission index of the lane's photon
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {1.f, 1.f, 1.f}, pw[3] = {0.f, 0.f, 0.f};
    bool exhausted = false;                           // wave-uniform: the counter has passed the round's end

    while (true) {
        // ---- re-arm the idle lanes with the next emissions
        const unsigned long long idle = __ballot(my == kNoPhoton);
        if (idle && !exhausted) {
            const unsigned n_idle = (unsigned)__popcll(idle);
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(a.next, n_idle);
            base = __shfl(base, 0, 64);
            const unsigned cand = base + (unsigned)__popcll(idle & ((1ull << lane) - 1ull));
            if (my == kNoPhoton && cand < a.count) {
                my = cand;
                state = 0;
                // DirectionalAreaLight::samplePhotonOrigin (DirectionalAreaLight.h:20-24)
                const uint32_t hd = pcg32(a.hdisc ^ (a.first + cand));
                float x = 0.0f, y = 0.0f;
                for (int k = 0; k < kDiscAttempts; k++) {
                    const uint32_t hk = pcg32(hd + (uint32_t)k);
                    const float xr = (2 * unit01(pcg32(hk)) - 1) * a.radius, yr = (2 * unit01(pcg32(hk ^ 0x68bc21ebu)) - 1) * a.radius;
                    if (!(xr * xr + yr * yr > a.radius * a.radius)) { x = xr; y = yr; break; }
                }
                for (int c = 0; c < 3; c++) {
                    const float p = a.pos[c] + (x * a.t1[c] + y * a.t2[c]);
                    d[c] = a.dir[c]; pw[c] = a.power[c];
                    o[c] = p + kEps * d[c];                                          // Scene.cpp:535
                }
            }
            exhausted = base + n_idle >= a.count;
        }
        const bool live = my != kNoPhoton;
        if (!__any(live)) break;

        // ---- Scene::trace(hit, ray, 0, MIRO_TMAX) (Scene.cpp:539)
        const mr_hit h = trace_hit<true, false, false, VAR>(a.tp, make_float4(o[0], o[1], o[2], 0.0f), make_float4(d[0], d[1], d[2], 1e12f), 1e12f,
                                                            live, s_stack, tid, st);
        if (live) {
            state += 1u;                                                                 // ++depth (:538)
            const uint32_t depth = state & 255u;
            bool alive = false;
            if (h.prim != MR_MISS) {
                const float *mt = material_of(a.m, h.prim);
                const uint32_t e = a.first + my;
                const uint32_t hev = pcg32(a.hevent ^ e) + depth * 2u;
                const float rnd = unit01(pcg32(pcg32(hev)));
                src.color(a, o, d, h, mt);                                               // diffuseColor (:545-549)
                const float p0 = avg3(src.col), p1 = p0 + avg3(mt + 3), p2 = p1 + avg3(mt + 6);      // :551-553
                if (!(rnd > p2)) {
                    ChildGen<true> g;
                    g.mt = mt;
                    src.point(a, o, d, h, g.P, g.N);
                    for (int c = 0; c < 3; c++) { g.d[c] = d[c]; g.w0[c] = 1.0f; }
                    g.Rs = 1.0f;
                    float org[3], nd[3], wgt[3];
                    if (rnd < p0) {                                                      // diffuse (:564-609)
                        bool go = true;
                        if (depth > 1u && ((state >> 8) & 255u) < a.max_depth) {      // (the second test always holds: at most one store per hit)
                            const uint32_t stores = (state >> 8) & 255u;
                            float4 *rec = a.slots + 3 * ((size_t)my * a.max_depth + stores);
                            rec[0] = make_float4(g.P[0], g.P[1], g.P[2], d[0]);
                            rec[1] = make_float4(d[1], d[2], pw[0], pw[1]);
                            rec[2] = make_float4(pw[2], __uint_as_float(e), __uint_as_float(depth), __uint_as_float((state >> 16) & 1u));
                            state += 1u << 8;
                        } else if (a.caustic) {
                            go = false;                                                  // :597-598
                        }
                        if (go) {
                            g.hray = pcg32(a.hdir ^ e) + depth * 4u;
                            g.make(3, org, nd, wgt);                                     // Ray::random: starts at P + epsilon * dir
                            const float inv = 1.0f / p0;
                            for (int c = 0; c < 3; c++) {
                                pw[c] = (src.col[c] * pw[c]) * inv;                      // diffuseColor * power / prob[0] (:608)
                                d[c] = nd[c];
                                o[c] = org[c] + kEps * nd[c];                            // ... and tracePhoton offsets it again (:535)
                            }
                            alive = true;
                        }
                    } else if (rnd < p2 && !(!a.caustic && depth == 1u)) {               // mirror or transmit (:610-649)
                        ChildGen<false> s;
                        s.mt = mt;
                        for (int c = 0; c < 3; c++) { s.P[c] = g.P[c]; s.N[c] = g.N[c]; s.d[c] = d[c]; s.w0[c] = 1.0f; }
                        s.Rs = 1.0f;
                        int kind = 0;
                        if (!(rnd < p1)) {
                            bool emit[4];
                            g.plan(false, true, false, emit);                            // getReflectionCoefficient on miro_math.h
                            const float rnd2 = unit01(pcg32(pcg32(hev + 1u)));
                            kind = rnd2 < g.Rs ? 0 : 2;                                  // :637
                        }
                        s.make(kind, org, nd, wgt);
                        if (depth == 1u) state |= 1u << 16;
                        for (int c = 0; c < 3; c++) { d[c] = nd[c]; o[c] = g.P[c] + kEps * nd[c]; }      // tracePhoton(hit.P, dir, ...)
                        alive = true;
                    }
                }
            }
            if (alive && depth > a.max_depth) alive = false;                             // :532
            if (!alive) {
                a.words[my] = ((state >> 8) & 255u) | (depth << 8);
                my = kNoPhoton;
            }
        }
    }
}

}  // namespace
}  // namespace mr
