// mr_gather_level.hip -- the photon-map term of Scene::traceScene (Scene.cpp:286-299) for ANY queue of the recursion
// (mr_gather_level): the eye rays, or the reflect / Fresnel / refract children of a later level with their path weights and
// pixels.  Two streaming kernels, one lane per ray, around the k-NN estimates of mr_photon.hip (launch_irradiance).  The
// query kernel is the library's only one: mr_final_gather launches it too, without a normal buffer and without counts, and
// then accumulates with its own kernel (gather_accumulate_kernel of mr_shade.hip: sample order, one float add per pixel).
//
//   gather_level_queries_kernel     hit point and normal of every ray whose hit has a diffuse material (Phong::isDiffuse,
//                                   Phong.cpp:39-42), a NaN normal elsewhere ("no query": irradiance_kernel answers 0).  The
//                                   normal is the object's, normalised (Scene.cpp:262), or, given the surface pass's
//                                   buffer, that buffer's (bumped on STONE):
//                                   what Scene.cpp:290 hands to irradiance_estimate.  Queries stay in place, not compacted.
//   gather_level_accumulate_kernel  E = irradiance + caustic per ray (Scene.cpp:298) to d_ray_rgb, and weight * E / spp to the
//                                   ray's pixel in the expression shape of store_shaded (mr_lights_body.h).  Whole waves:
//                                   accumulate_runs shuffles.
//
// Both are memory-bound: 32 + 16 bytes in and 24 out per ray for the first (the mesh lookups of a triangle hit on top), 24
// in and up to 12 out plus the run's atomics for the second.  The time of a level is the k-NN estimates between them
// (DESIGN.md section 5b).
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

__global__ __launch_bounds__(kBlock) void gather_level_queries_kernel(QueryArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_queries = 0, my_rays = 0;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < a.n; k += stride) {
        const float4 h = reinterpret_cast<const float4 *>(a.hits)[k];
        const uint32_t prim = __float_as_uint(h.y);
        float P[3] = {0.f, 0.f, 0.f}, N[3];
        N[0] = N[1] = N[2] = __uint_as_float(0x7fc00000u);
        my_rays++;
        if (prim != MR_MISS && rec::any_pos(rec::material_of(a.m, prim))) {
            rec::surface_point(a.m, a.rays, k, h, P, N);
            if (a.normal)                                                  // wave-uniform
                for (int c = 0; c < 3; c++) N[c] = a.normal[3 * k + c];
            my_queries++;
        }
        for (int c = 0; c < 3; c++) { a.pos[3 * k + c] = P[c]; a.nrm[3 * k + c] = N[c]; }
    }
    if (a.counts) {                                                        // all threads of the workgroup are here
        const unsigned mine[2] = {my_queries, my_rays};
        workgroup_add<kBlock>(mine, a.counts);
    }
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

__global__ __launch_bounds__(kBlock) void gather_level_accumulate_kernel(AccumulateArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const unsigned long long n_round = (a.n + 63ull) & ~63ull;             // whole waves: accumulate_runs shuffles
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n_round; k += stride) {
        const bool live = k < a.n;
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
}

}  // namespace

mr_status launch_gather_level_queries(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                                      unsigned long long n, float *d_pos, float *d_nrm, unsigned long long *d_counts,
                                      hipStream_t stream) {
    if (n == 0) return MR_OK;
    QueryArgs a;
    a.m = rec::mesh_of(ds);
    a.rays = d_rays; a.hits = d_hits; a.normal = d_normal; a.n = n;
    a.pos = d_pos; a.nrm = d_nrm; a.counts = d_counts;
    hipLaunchKernelGGL(gather_level_queries_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_gather_level_accumulate(const float *d_irr_a, const float *d_irr_b, const float *d_weights, const uint32_t *d_pixels,
                                         unsigned long long n, uint32_t spp, float *d_rgb, float *d_ray_rgb, hipStream_t stream) {
    if (n == 0) return MR_OK;
    AccumulateArgs a;
    a.irr_a = d_irr_a; a.irr_b = d_irr_b; a.weights = d_weights; a.pixels = d_pixels;
    a.n = n; a.spp = spp; a.inv_spp = 1.0f / (float)spp;
    a.rgb = d_rgb; a.ray_rgb = d_ray_rgb;
    hipLaunchKernelGGL(gather_level_accumulate_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
