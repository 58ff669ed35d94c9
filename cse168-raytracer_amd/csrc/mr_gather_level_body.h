// mr_gather_level_body.h -- the per-ray steps of the two streaming kernels around the photon-map estimates (Scene.cpp:286-299), with
// their argument blocks: ONE definition for the kernels that take the length of their queue from the host (mr_gather_level.hip:
// mr_final_gather, mr_gather_level) and for the ones that read it from a device word or re-create level 0's eye rays
// (mr_gather_queued.hip: mr_render_recursion_photons).
//
//   gather_query_step       hit point and normal of a ray whose hit has a diffuse material (Phong::isDiffuse, Phong.cpp:39-42), a NaN
//                           normal elsewhere ("no query": irradiance_kernel answers 0).  The ray is asked for only where there is a
//                           query: ray_of(k, ra, rb) loads it from a queue, or makes the eye ray of sample k again.
//   gather_accumulate_step  E = irradiance + caustic of a ray (Scene.cpp:298) to ray_rgb, and weight * E / spp to the ray's pixel in
//                           the expression shape of store_shaded (mr_lights_body.h).  Called by whole waves: accumulate_runs shuffles.
// Included by the .hip units that instantiate it (everything here is local to its unit).
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_recursion.h"
#include "mr_surface.h"
#include "mr_traverse.h"

namespace mr {
namespace {

struct QueryArgs {
    rec::MeshMat m;
    const mr_ray *rays;
    const mr_hit *hits;
    const float *normal;          // may be NULL: three floats per ray (mr_hit_surface), read for query rays only
    unsigned long long n;
    float *pos, *nrm;             // 3 n floats each
    unsigned long long *counts;   // optional: [0] += queries made, [1] += rays seen
};

// ray k of the queue a.rays
struct QueueRayOf {
    const mr_ray *rays;
    __device__ __forceinline__ void operator()(unsigned long long k, float4 &ra, float4 &rb) const {
        ra = reinterpret_cast<const float4 *>(rays)[2 * k];
        rb = reinterpret_cast<const float4 *>(rays)[2 * k + 1];
    }
};

// ray k's query into pos / nrm; returns whether there is one
template <typename RAY_OF>
__device__ __forceinline__ bool gather_query_step(const rec::MeshMat &m, const mr_hit *hits, const float *normal, unsigned long long k,
                                                  float *pos, float *nrm, const RAY_OF &ray_of) {
    const float4 h = reinterpret_cast<const float4 *>(hits)[k];
    const uint32_t prim = __float_as_uint(h.y);
    float P[3] = {0.f, 0.f, 0.f}, N[3];
    N[0] = N[1] = N[2] = __uint_as_float(0x7fc00000u);
    bool query = false;
    if (prim != MR_MISS && rec::any_pos(rec::material_of(m, prim))) {
        float4 ra, rb;
        ray_of(k, ra, rb);
        rec::surface_point_od(m, ra.x, ra.y, ra.z, rb.x, rb.y, rb.z, h.x, prim, h.z, h.w, P, N);
        if (normal)                                                    // wave-uniform
            for (int c = 0; c < 3; c++) N[c] = normal[3 * k + c];
        query = true;
    }
    for (int c = 0; c < 3; c++) { pos[3 * k + c] = P[c]; nrm[3 * k + c] = N[c]; }
    return query;
}

struct AccumulateArgs {
    const float *irr_a, *irr_b;   // the two estimates, 3 n floats each; either may be NULL
    const float *weights;         // rgb per ray or NULL (= 1)
    const uint32_t *pixels;       // pixel per ray or NULL (= ray index / spp)
    unsigned long long n;
    uint32_t spp;
    float inv_spp;
    float *rgb;                   // may be NULL (then ray_rgb is not)
    float *ray_rgb;               // may be NULL: the un-weighted E of every ray
};

// live: k is a ray of the queue (a lane past its end only takes part in the shuffles)
__device__ __forceinline__ void gather_accumulate_step(const AccumulateArgs &a, unsigned long long k, bool live) {
    float E[3] = {0.f, 0.f, 0.f};
    if (live)
        for (int c = 0; c < 3; c++) {                                  // a non-query's estimates are 0
            float v = 0.0f;
            if (a.irr_a) v = a.irr_a[3 * k + c];
            if (a.irr_b) v = a.irr_a ? v + a.irr_b[3 * k + c] : a.irr_b[3 * k + c];      // Scene.cpp:298
            E[c] = v;
        }
    if (a.ray_rgb && live) { a.ray_rgb[3 * k] = E[0]; a.ray_rgb[3 * k + 1] = E[1]; a.ray_rgb[3 * k + 2] = E[2]; }
    if (a.rgb) {                                                       // wave-uniform
        uint32_t pix = 0xFFFFFFFFu;
        float v[3] = {0.f, 0.f, 0.f};
        if (live) {
            pix = rec::pixel_of(a.pixels, k, a.spp);
            float w[3];
            rec::weight_of(a.weights, k, w);
            for (int c = 0; c < 3; c++) v[c] = E[c] * w[c] * a.inv_spp;
        }
        rec::accumulate_runs(a.rgb, pix, v[0], v[1], v[2]);
    }
}

}  // namespace
}  // namespace mr
