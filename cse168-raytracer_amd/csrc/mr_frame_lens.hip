// mr_frame_lens.hip -- the level-0 frame of mr_frame_level_lights.hip for the thin-lens camera (mr_render_level_lights_lens,
// mr_render_recursion_lens, mr_render_recursion_photons_lens; include/miro_hip_lens.h): the reference's depth-of-field frame
// (Scene::raytraceImage under -DDOF, Scene.cpp:126-139; Camera::eyeRay, Camera.cpp:135-160; DOF_APERTURE / DOF_FOCUS_PLANE,
// Miro.h:18-19) and the first level of Scene::traceScene's recursion as one launch --
//
//   Camera::eyeRay through a point of the lens  ->  Scene::trace, the bump-mapped normal included  ->  a ray that leaves the scene:
//   getEnvironmentMap(ray)  ->  a hit: diffuseColor, Phong::shade's loop over Scene::lights()  ->  the pixel's mean, a plain store
//   ->  the children of the next level, compacted into its queue
//
// The lens changes the ray's prologue and nothing else.  The kernel is frame_lights_surface_body<VAR, false, true, CHILDREN, true>
// (mr_frame_lights_surface_body.h): where the pinhole frame makes eye_ray_of, this one makes eye_ray_lens_of (mr_eye.h), the
// definition eye_rays_lens_kernel (mr_distribution.hip, mr_gen_eye_rays_lens) calls with d_samples_in == NULL -- the sample's
// key, its jitter, sampleDisc's rejection loop of at most 32 rounds, the point on the lens, the direction through the focus
// point -- and the hit point of a sphere or a plane starts from that point instead of the uniform eye.  A triangle's hit point
// is barycentric and reads no origin.  So every output of the frame half is, bit for bit, what the batched chain writes for
// mr_gen_eye_rays_lens' rays of the same window, seed, spp and lens, and the children are the set the level calls emit on that
// queue.  The children step reads P, N, d, colour and material: a child starts at the hit point and does not know what camera
// made its parent.  Levels >= 1 are the kernels of mr_level_lights_queued.hip, untouched.
//
// Live state: the sample's ray is made again at each of the three places that need it (before the primary traversal; at the hit,
// origin and direction; after it, the direction for the environment, the children and the light loop), not held across a
// traversal: a point on the lens is three registers more than the pinhole frame keeps, the rejection loop's draws are integer
// hashes, and the two places after the traversal have nothing between them, so the compiler is free to make them one.  An exhausted
// rejection loop leaves the lens centre, as in the generator; it is not counted here.
//
// Nineteen kernels: the six traversal variants x CHILDREN 0 (MR_LEVEL_LAST), 1 (MR_LEVEL_SPECULAR), 2 (MR_LEVEL_PATH), and
// gather_eye_queries_lens_kernel, level 0 of the photon-map term (mr_gather_queued.hip's gather_eye_queries_kernel with the
// lens ray made again for sample k: gather_query_step reads the ray's origin for a sphere or a plane).
//
// Compiled like mr_frame_level_lights.hip, without machine-level loop-invariant code motion (the Makefile's FRAME_LEVEL_FLAGS;
// that unit's header says what the pass does to the sample loop).
//
// Waves per SIMD, VGPRs, spilled VGPRs and scratch bytes per lane (hipcc, gfx950, the Makefile's flags); the envelope is the worst
// kernel of tests/golden/kernel_budget.json, 30 spilled VGPRs / 108 bytes / 4 waves:
//
//                                 MR_LEVEL_LAST                   MR_LEVEL_SPECULAR               MR_LEVEL_PATH
//   variant                     waves  VGPRs  spilled / scratch   waves  VGPRs  spilled / scratch   waves  VGPRs  spilled / scratch
//   kTraceExact (1818)            5      93      0 /   0            4     110      0 /   0            4     111      0 /   0
//   kTraceExactObj (826)          4      98      0 /   0            4     116      0 /   0            4     116      0 /  20
//   kTraceProduct (267)           5      88      0 /   0            4     100      0 /   0            4     101      0 /   0
//   kTraceProductObj (43)         5      90      0 /   0            4     105      0 /   0            4     106      0 /  20
//   kTraceVote (88)               5      85      0 /   0            4     100      0 /   0            4     100      0 /  20
//   kTraceVoteProduct (73)        5      85      0 /   0            5      95      0 /   0            4      98      0 /  20
//   gather_eye_queries_lens_kernel: 7 waves, 47 VGPRs, 0 / 0
//
// No kernel spills a VGPR and every one is inside the envelope, with the sample's ray made again at each site; so it is not held
// across a traversal.  The kernels with children are within 2 VGPRs of their pinhole twins in mr_frame_level_lights.hip.
//
// Times against the batched lens route and against the pinhole one-call frame: DESIGN section 5c, profiles/recursion_lens_ab.log.
#include <hip/hip_runtime.h>

#include "mr_frame_lights_surface_body.h"
#include "mr_gather_level_body.h"

namespace mr {
namespace {

struct FrameLensArgs {
    FrameLightsSurfaceArgs f;
    EnvParams env;               // all zero without `environment`; full nullptr: colour only (bg); low / lw / lh are not read
    FrameChildArgs ch;           // CHILDREN == 0: not read
    LensParams ln;
};

#ifndef MIRO_FRAME_LENS_WAVES
#define MIRO_FRAME_LENS_WAVES 4
#endif

// VAR: as in frame_lights_kernel; CHILDREN: 0 none, 1 specular, 2 path tracing.  The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, int CHILDREN>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_FRAME_LENS_WAVES, 8))) void frame_lens_kernel(const FrameLensArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    frame_lights_surface_body<VAR, false, true, CHILDREN, true>(a.f, a.env, a.ch, a.ln, s_stack, s_tab);
}

// the focus point of fd's camera: m_viewDir is make_eye_frame's, as launch_eye_rays_lens takes it
LensParams lens_params_of_frame(const mr_frame_desc &fd, const mr_lens_desc &lens) {
    float view[3];
    make_eye_frame(fd.camera, fd.W, fd.H, 0, 0, fd.spp, fd.jitter, fd.seed, false, view);
    return lens_params_of(fd.camera, view, lens);
}

struct EyeLensQueryArgs {
    EyeFrame eye;                 // the frame's window: eye.n samples
    LensParams ln;
    rec::MeshMat m;
    const mr_hit *hits;           // the frame's hit record of sample k
    const float *normal;          // may be NULL: the frame's normal of sample k's hit
    float *pos, *nrm;             // 3 eye.n floats each
    unsigned long long *queries;  // += queries made
};

// Camera::eyeRay under -DDOF of sample k of the window, as the lens frame makes it
struct EyeLensRayOf {
    const EyeFrame &f;
    const LensParams &ln;
    __device__ __forceinline__ void operator()(unsigned long long k, float4 &ra, float4 &rb) const {
        uint32_t x, row, y, sm;
        eye_sample_of(f, k, x, row, y, sm);
        eye_ray_lens_of(f, ln, x, y, sm, ra, rb);
    }
};

__global__ __launch_bounds__(kBlock) void gather_eye_queries_lens_kernel(EyeLensQueryArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_queries = 0;
    const EyeLensRayOf ray_of = {a.eye, a.ln};
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < a.eye.n; k += stride)
        if (gather_query_step(a.m, a.hits, a.normal, k, a.pos, a.nrm, ray_of)) my_queries++;
    workgroup_add<kBlock>(my_queries, a.queries);
}

}  // namespace

mr_status launch_frame_lens(const char *who, const LightScene &ls, const mr_frame_desc &fd, const mr_lens_desc &lens, const mr_frame_level_desc &ld,
                            const FrameOutputs &o, const RayQueue &out, unsigned long long *d_out_count, hipStream_t stream) {
    FrameLensArgs a = {};
    const bool children = ld.children != MR_LEVEL_LAST;
    mr_status st = fill_frame_lights_surface_args(a.f, who, ls, fd, o);
    if (st != MR_OK || (children && (st = launch_zero_count(d_out_count, stream)) != MR_OK)) return st;
    if (a.f.eye.n == 0) return MR_OK;
    a.env = ls.env;
    a.ln = lens_params_of_frame(fd, lens);
    if (children) fill_frame_child_args(a.ch, ld, out, d_out_count);

    // the traversal variants of launch_frame_level_lights: the same hit records from each of them
    const DeviceScene &ds = *ls.ds;
    return with_trace_variant(ds.n_planes || ds.n_spheres, fd.flags & MR_MATH_PRODUCT, fd.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        auto kern = &frame_lens_kernel<VAR, 0>;
        if (children) kern = ld.children == MR_LEVEL_PATH ? &frame_lens_kernel<VAR, 2> : &frame_lens_kernel<VAR, 1>;
        return launch_traversal(kern, trace_grid(a.f.eye.n), a.f.tp.stack_depth, stream, a);
    });
}

mr_status launch_gather_eye_queries_lens(const DeviceScene &ds, const char *who, const mr_frame_desc &fd, const mr_lens_desc &lens,
                                         const mr_hit *d_hits, const float *d_normal, float *d_pos, float *d_nrm,
                                         unsigned long long *d_queries, hipStream_t stream) {
    EyeLensQueryArgs a;
    const mr_status st = frame_window_of(who, fd, a.eye);
    if (st != MR_OK) return st;
    if (a.eye.n == 0) return MR_OK;
    a.ln = lens_params_of_frame(fd, lens);
    a.m = rec::mesh_of(ds);
    a.hits = d_hits; a.normal = d_normal; a.pos = d_pos; a.nrm = d_nrm; a.queries = d_queries;
    hipLaunchKernelGGL(gather_eye_queries_lens_kernel, dim3(grid_for(a.eye.n)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
