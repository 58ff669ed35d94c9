// mr_gather_queued.hip -- the photon-map term of Scene::traceScene (Scene.cpp:286-299) for a queue whose LENGTH is a word on the
// device (mr_render_recursion_photons, mr_api.cpp): the three steps of mr_gather_level -- queries, one k-NN estimate per map,
// accumulate -- as kernels that read
//
//   n = min(*d_n, bound)      d_n: the word a level counted its rays or children into, bound: what the host knows the length
//                             cannot exceed, at most what the queue can hold (the kernels take it as the queue's capacity)
//
// themselves, by every lane from the same address before anything else: a wave-uniform load from a kernel argument's pointer,
// which comes out as a scalar load (mr_level_lights_queued.hip has the pattern).  The host sizes every grid from that bound,
// never from n.  The per-ray steps are the definitions the host-n kernels call (mr_gather_level_body.h,
// mr_irradiance_body.h), so a level's queries, estimates and pixel adds are what mr_gather_level makes of the same queue.
//
//   gather_queued_queries_kernel     gather_level_queries_kernel's step for rays [0, n); the queries made are counted into one
//                                    word.  A workgroup whose first index is at or beyond n returns before touching anything;
//                                    the others stride over the queue.
//   gather_eye_queries_kernel        level 0 of the one-call frame has no eye-ray buffer (mr_render_level_lights keeps rays in
//                                    registers): the eye ray of sample k is made again with mr_eye.h (eye_sample_of / eye_ray_of,
//                                    the code the frame kernel itself runs) and joined with the hit record the frame wrote.  The
//                                    queries are the bits gather_level_queries_kernel writes for mr_gen_eye_rays' buffer of the same
//                                    window.  Its n is the window's, known on the host.
//   irradiance_queued_kernel<STATS>  irradiance_kernel<STATS>'s body with nq read here.  Its grid is min(ceil(bound / 4), 1536)
//                                    workgroups whatever nq is; every wave reads the same nq, so exactly one wave sees the value
//                                    that re-arms the hand-out counter -- with nq == 0 each wave pulls once and the last re-arms.
//   gather_queued_accumulate_kernel  gather_level_accumulate_kernel's step for rays [0, n), whole waves (accumulate_runs shuffles).
//
// An empty queue costs each grid its exits.  tests/golden/kernel_budget_gather_queued.json holds every kernel; the estimate
// without STATS keeps five waves per SIMD like its host-n twin.  Times against the per-level driver: DESIGN section 5c,
// profiles/recursion_photons_ab.log.
#include <hip/hip_runtime.h>

#include "mr_eye.h"
#include "mr_frame_window.h"
#include "mr_gather_level_body.h"
#include "mr_irradiance_body.h"

namespace mr {
namespace {

// the queue's length, and whether this workgroup has a ray of it
__device__ __forceinline__ bool queued_length(const unsigned long long *d_n, unsigned long long n_cap, unsigned long long &n) {
    const unsigned long long have = *d_n;             // every lane, one address: wave-uniform
    n = have < n_cap ? have : n_cap;
    return (unsigned long long)blockIdx.x * kBlock < n;
}

// a.n: the queue's capacity; a.counts: ONE word, += queries made (not optional)
__global__ __launch_bounds__(kBlock) void gather_queued_queries_kernel(QueryArgs a, const unsigned long long *d_n) {
    unsigned long long n;
    if (!queued_length(d_n, a.n, n)) return;          // workgroup-uniform
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_queries = 0;
    const QueueRayOf ray_of = {a.rays};
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride)
        if (gather_query_step(a.m, a.hits, a.normal, k, a.pos, a.nrm, ray_of)) my_queries++;
    workgroup_add<kBlock>(my_queries, a.counts);      // all threads of the workgroup are here
}

struct EyeQueryArgs {
    EyeFrame eye;                 // the frame's window: eye.n samples
    rec::MeshMat m;
    const mr_hit *hits;           // the frame's hit record of sample k
    const float *normal;          // may be NULL: the frame's normal of sample k's hit
    float *pos, *nrm;             // 3 eye.n floats each
    unsigned long long *queries;  // += queries made
};

// Camera::eyeRay of sample k of the window, as the frame kernel makes it
struct EyeRayOf {
    const EyeFrame &f;
    __device__ __forceinline__ void operator()(unsigned long long k, float4 &ra, float4 &rb) const {
        uint32_t x, row, y, sm;
        eye_sample_of(f, k, x, row, y, sm);
        eye_ray_of(f, x, y, sm, ra, rb);
    }
};

__global__ __launch_bounds__(kBlock) void gather_eye_queries_kernel(EyeQueryArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_queries = 0;
    const EyeRayOf ray_of = {a.eye};
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < a.eye.n; k += stride)
        if (gather_query_step(a.m, a.hits, a.normal, k, a.pos, a.nrm, ray_of)) my_queries++;
    workgroup_add<kBlock>(my_queries, a.queries);
}

// The map is taken by value and handed on by const reference (mr_irradiance_body.h).  Five waves per SIMD without STATS, as
// irradiance_kernel.
template <bool STATS>
__global__ __launch_bounds__(kIrrBlock) __attribute__((amdgpu_waves_per_eu(STATS ? 4 : 5, 8))) void irradiance_queued_kernel(
    PhotonMapDev pm, const float *qpos, const float *qnrm, const unsigned long long *d_n, unsigned long long n_cap, float max_dist, int k,
    float *irrad, unsigned long long *stats, int stack_cap, unsigned *work_counter) {
    extern __shared__ int s_lds[];
    const unsigned long long have = *d_n;             // every lane of every wave, one address: the same nq throughout the grid
    const unsigned long long nq = have < n_cap ? have : n_cap;
    irradiance_body<STATS>(pm, qpos, qnrm, nq, max_dist, k, irrad, nullptr, nullptr, stats, stack_cap, work_counter, s_lds);
}

// a.n: the queue's capacity
__global__ __launch_bounds__(kBlock) void gather_queued_accumulate_kernel(AccumulateArgs a, const unsigned long long *d_n) {
    unsigned long long n;
    if (!queued_length(d_n, a.n, n)) return;          // workgroup-uniform
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const unsigned long long n_round = (n + 63ull) & ~63ull;               // whole waves: accumulate_runs shuffles
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n_round; k += stride)
        gather_accumulate_step(a, k, k < n);
}

}  // namespace

mr_status launch_gather_eye_queries(const DeviceScene &ds, const char *who, const mr_frame_desc &fd, const mr_hit *d_hits,
                                    const float *d_normal, float *d_pos, float *d_nrm, unsigned long long *d_queries, hipStream_t stream) {
    EyeQueryArgs a;
    const mr_status st = frame_window_of(who, fd, a.eye);
    if (st != MR_OK) return st;
    if (a.eye.n == 0) return MR_OK;
    a.m = rec::mesh_of(ds);
    a.hits = d_hits; a.normal = d_normal; a.pos = d_pos; a.nrm = d_nrm; a.queries = d_queries;
    hipLaunchKernelGGL(gather_eye_queries_kernel, dim3(grid_for(a.eye.n)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_gather_queued_queries(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                                       const unsigned long long *d_n, unsigned long long bound, float *d_pos, float *d_nrm,
                                       unsigned long long *d_queries, hipStream_t stream) {
    if (bound == 0) return MR_OK;
    QueryArgs a;
    a.m = rec::mesh_of(ds);
    a.rays = d_rays; a.hits = d_hits; a.normal = d_normal; a.n = bound;
    a.pos = d_pos; a.nrm = d_nrm; a.counts = d_queries;
    hipLaunchKernelGGL(gather_queued_queries_kernel, dim3(grid_for(bound)), dim3(kBlock), 0, stream, a, d_n);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_irradiance_queued(const PhotonMapDev &pm, unsigned *work_counter, const float *d_pos, const float *d_normal,
                                   const unsigned long long *d_n, unsigned long long bound, float max_dist, uint32_t k, float *d_irrad,
                                   unsigned long long *d_stats, hipStream_t stream) {
    if (bound == 0) return MR_OK;
    int stack_cap = 0;
    size_t lds = 0;
    unsigned blocks = 0;
    const mr_status st = irradiance_launch_shape(pm, work_counter, bound, stack_cap, lds, blocks);
    if (st != MR_OK) return st;
    if (d_stats)
        hipLaunchKernelGGL(irradiance_queued_kernel<true>, dim3(blocks), dim3(kIrrBlock), lds, stream, pm, d_pos, d_normal, d_n, bound,
                           max_dist, (int)k, d_irrad, d_stats, stack_cap, work_counter);
    else
        hipLaunchKernelGGL(irradiance_queued_kernel<false>, dim3(blocks), dim3(kIrrBlock), lds, stream, pm, d_pos, d_normal, d_n, bound,
                           max_dist, (int)k, d_irrad, d_stats, stack_cap, work_counter);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_gather_queued_accumulate(const float *d_irr_a, const float *d_irr_b, const float *d_weights, const uint32_t *d_pixels,
                                          const unsigned long long *d_n, unsigned long long bound, uint32_t spp, uint32_t spp_total,
                                          float *d_rgb, hipStream_t stream) {
    if (bound == 0) return MR_OK;
    AccumulateArgs a;
    a.irr_a = d_irr_a; a.irr_b = d_irr_b; a.weights = d_weights; a.pixels = d_pixels;
    a.n = bound; a.spp = spp; a.inv_spp = 1.0f / (float)spp_total;
    a.rgb = d_rgb; a.ray_rgb = nullptr;
    hipLaunchKernelGGL(gather_queued_accumulate_kernel, dim3(grid_for(bound)), dim3(kBlock), 0, stream, a, d_n);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
