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
// The per-ray step of each is mr_gather_level_body.h's, which the kernels of mr_gather_queued.hip (a queue whose length is a device
// word) call too.  Both are memory-bound: 32 + 16 bytes in and 24 out per ray for the first (the mesh lookups of a triangle hit on top), 24
// in and up to 12 out plus the run's atomics for the second.  The time of a level is the k-NN estimates between them
// (DESIGN.md section 5b).
#include <hip/hip_runtime.h>

#include "mr_gather_level_body.h"

namespace mr {
namespace {

__global__ __launch_bounds__(kBlock) void gather_level_queries_kernel(QueryArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_queries = 0, my_rays = 0;
    const QueueRayOf ray_of = {a.rays};
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < a.n; k += stride) {
        my_rays++;
        if (gather_query_step(a.m, a.hits, a.normal, k, a.pos, a.nrm, ray_of)) my_queries++;
    }
    if (a.counts) {                                                        // all threads of the workgroup are here
        const unsigned mine[2] = {my_queries, my_rays};
        workgroup_add<kBlock>(mine, a.counts);
    }
}

__global__ __launch_bounds__(kBlock) void gather_level_accumulate_kernel(AccumulateArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const unsigned long long n_round = (a.n + 63ull) & ~63ull;             // whole waves: accumulate_runs shuffles
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n_round; k += stride)
        gather_accumulate_step(a, k, k < a.n);
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
