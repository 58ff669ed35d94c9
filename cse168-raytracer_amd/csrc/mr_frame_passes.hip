// mr_frame_passes.hip -- level 0 of ONE PASS of a frame of S samples per pixel (mr_render_recursion_passes,
// mr_render_recursion_photons_passes; include/miro_hip_passes.h): the reference's own picture takes TRACE_SAMPLES = 1000 samples
// per pixel (Scene::raytraceImage, Scene.cpp:126-139; Miro.h:15), and a pixel's samples are the lanes of one wave here, 64 at
// the most.  A pass renders samples [base, base + p) of every pixel of the window, p a power of two <= 64, and the frame is its
// passes enqueued one after the other on one stream over one workspace.
//
// The kernel is frame_lights_surface_body<VAR, false, true, CHILDREN, LENS, true> (mr_frame_lights_surface_body.h): the pinhole
// frame of mr_frame_level_lights.hip / mr_frame_lights_env.hip and the lens frame of mr_frame_lens.hip with PASS on, which
// changes four things and nothing else --
//   the sample's key      eye_sample_key(f, x, y, base + sm): jitter and, under the lens, sampleDisc's draws, at the three places
//                         that make the ray
//   hash and child id     the path tracer's per-sample hash and the id handed to write_children_col come from
//                         pixel * S + base + sm, the index a single launch at spp = S would give the sample; levels >= 1 draw
//                         from (seed, ray id, bounce, kind) and so see the ids of that launch
//   the pixel's value     the butterfly sum over the pass's p lanes, times 1 / S (S > 1)
//   store or add          the pixel's lane stores the value, or adds it to what d_rgb holds with a plain load, add and store: the
//                         passes of a frame follow each other in stream order and a pixel has one owner lane.  No atomics.
// So a frame's samples have one numbering, 0 .. S - 1 per pixel, that no cut into passes changes; only the order in which a
// pixel's float terms are added depends on the plan (mr_render_passes_plan states it).  A pass with S = p, base = 0 that stores
// is the parent call's level 0, bit for bit.
//
// Levels >= 1 are the kernels of mr_level_lights_queued.hip and mr_gather_queued.hip, untouched: the host hands them S as the
// divisor.  Level 0 of the photon term is gather_eye_queries_pass_kernel<LENS>: gather_eye_queries[_lens]_kernel's body with the
// ray of sample base + sm made again.
//
// 36 frame kernels (the six traversal variants x CHILDREN 0 / 1 / 2 x pinhole / lens; ENV true, ANY false, as in the lens unit)
// and the two query kernels.  Compiled like mr_frame_level_lights.hip, without machine-level loop-invariant code motion (the
// Makefile's FRAME_LEVEL_FLAGS; that unit's header says what the pass does to the sample loop).
//
// VGPRs and scratch bytes per lane against the twin without PASS (hipcc, gfx950, the Makefile's flags; the pinhole twin of
// CHILDREN 0 is mr_frame_lights_env.hip's kernel, of 1 / 2 mr_frame_level_lights.hip's, the lens twins are mr_frame_lens.hip's);
// the envelope is the worst kernel of tests/golden/kernel_budget.json, 30 spilled VGPRs / 108 bytes / 4 waves.  No kernel of the
// unit spills a VGPR, every one runs four waves per SIMD or more:
//
//                            each cell: waves VGPRs scratch of the pass kernel | of its twin
//                            LAST pinhole          LAST lens             SPECULAR pinhole      SPECULAR lens         PATH pinhole          PATH lens
//   kTraceExact (1818)      4  97  68 | 4 123  68   5  93  68 | 5  93   0   4 109  68 | 4 109  68   4 110  68 | 4 110   0   4 110  68 | 4 110  68   4 112  68 | 4 111   0
//   kTraceExactObj (826)    4  97  68 | 4 128  68   4  98   0 | 4  98   0   4 115 100 | 4 114  68   4 115  36 | 4 116   0   4 116  68 | 4 115  68   4 117  68 | 4 116  20
//   kTraceProduct (267)     5  87  68 | 4 114  68   5  88  68 | 5  88   0   4  99  68 | 4  99  68   4 100  68 | 4 100   0   4 100  68 | 4 100  68   4 102  68 | 4 101   0
//   kTraceProductObj (43)   5  89  68 | 4 121  68   5  90   0 | 5  90   0   4 103  68 | 4 103  68   4 105   0 | 4 105   0   4 105  68 | 4 104  68   4 106  68 | 4 106  20
//   kTraceVote (88)         5  84   0 | 4 114  68   5  85   0 | 5  85   0   4  99   0 | 4  98   0   4 100   0 | 4 100   0   4  99  68 | 4  99  68   4 101  68 | 4 100  20
//   kTraceVoteProduct (73)  5  84   0 | 4 116  68   5  85   0 | 5  85   0   5  96   0 | 5  95   0   5  96   0 | 5  95   0   5  96  68 | 5  96 100   4  98  68 | 4  98  20
//   gather_eye_queries_pass_kernel<false | true>: 7 waves, 47 VGPRs, 0 bytes each, as gather_eye_queries[_lens]_kernel
//
// tests/golden/kernel_budget_frame_passes.json holds every kernel.  Times against summed parent calls: DESIGN section 5c, profiles/render_passes_ab.log.
#include <hip/hip_runtime.h>

#include "mr_frame_lights_surface_body.h"
#include "mr_gather_level_body.h"

namespace mr {
namespace {

struct FramePassArgs {
    FrameLightsSurfaceArgs f;
    EnvParams env;               // all zero without `environment`; full nullptr: colour only (bg); low / lw / lh are not read
    FrameChildArgs ch;           // CHILDREN == 0: not read
    LensParams ln;               // LENS false: not read
    PassParams ps;
};

#ifndef MIRO_FRAME_PASSES_WAVES
#define MIRO_FRAME_PASSES_WAVES 4
#endif

// VAR: as in frame_lights_kernel; CHILDREN: 0 none, 1 specular, 2 path tracing.  The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, int CHILDREN, bool LENS>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_FRAME_PASSES_WAVES, 8))) void frame_pass_kernel(const FramePassArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    frame_lights_surface_body<VAR, false, true, CHILDREN, LENS, true>(a.f, a.env, a.ch, a.ln, s_stack, s_tab, a.ps);
}

// the focus point of fd's camera (mr_frame_lens.hip's lens_params_of_frame)
LensParams lens_params_of_frame(const mr_frame_desc &fd, const mr_lens_desc &lens) {
    float view[3];
    make_eye_frame(fd.camera, fd.W, fd.H, 0, 0, fd.spp, fd.jitter, fd.seed, false, view);
    return lens_params_of(fd.camera, view, lens);
}

struct EyePassQueryArgs {
    EyeFrame eye;                 // the pass's window: eye.n samples, eye.spp per pixel
    LensParams ln;                // LENS false: not read
    uint32_t base;                // sample k of the window is sample base + k % eye.spp of its pixel
    rec::MeshMat m;
    const mr_hit *hits;           // the pass's hit record of sample k
    const float *normal;          // may be NULL: the pass's normal of sample k's hit
    float *pos, *nrm;             // 3 eye.n floats each
    unsigned long long *queries;  // += queries made
};

// Camera::eyeRay of sample k of the pass's window, as the pass kernel makes it
template <bool LENS>
struct EyePassRayOf {
    const EyePassQueryArgs &a;
    __device__ __forceinline__ void operator()(unsigned long long k, float4 &ra, float4 &rb) const {
        uint32_t x, row, y, sm;
        eye_sample_of(a.eye, k, x, row, y, sm);
        if constexpr (LENS) eye_ray_lens_of(a.eye, a.ln, x, y, a.base + sm, ra, rb);
        else eye_ray_of(a.eye, x, y, a.base + sm, ra, rb);
    }
};

template <bool LENS>
__global__ __launch_bounds__(kBlock) void gather_eye_queries_pass_kernel(EyePassQueryArgs a) {
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_queries = 0;
    const EyePassRayOf<LENS> ray_of = {a};
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < a.eye.n; k += stride)
        if (gather_query_step(a.m, a.hits, a.normal, k, a.pos, a.nrm, ray_of)) my_queries++;
    workgroup_add<kBlock>(my_queries, a.queries);
}

}  // namespace

mr_status launch_frame_pass(const char *who, const LightScene &ls, const mr_frame_desc &fd, const mr_lens_desc *lens, const mr_frame_level_desc &ld,
                            const FramePass &pass, const FrameOutputs &o, const RayQueue &out, unsigned long long *d_out_count,
                            hipStream_t stream) {
    FramePassArgs a = {};
    const bool children = ld.children != MR_LEVEL_LAST;
    mr_status st = fill_frame_lights_surface_args(a.f, who, ls, fd, o);
    if (st != MR_OK || (children && (st = launch_zero_count(d_out_count, stream)) != MR_OK)) return st;
    if (a.f.eye.n == 0) return MR_OK;
    a.env = ls.env;
    if (lens) a.ln = lens_params_of_frame(fd, *lens);
    if (children) fill_frame_child_args(a.ch, ld, out, d_out_count);
    a.ps.S = pass.S; a.ps.base = pass.base; a.ps.add = pass.base != 0 ? 1u : 0u;

    // the traversal variants of launch_frame_level_lights: the same hit records from each of them
    const DeviceScene &ds = *ls.ds;
    return with_trace_variant(ds.n_planes || ds.n_spheres, fd.flags & MR_MATH_PRODUCT, fd.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        auto kern = lens ? &frame_pass_kernel<VAR, 0, true> : &frame_pass_kernel<VAR, 0, false>;
        if (ld.children == MR_LEVEL_PATH) kern = lens ? &frame_pass_kernel<VAR, 2, true> : &frame_pass_kernel<VAR, 2, false>;
        else if (children) kern = lens ? &frame_pass_kernel<VAR, 1, true> : &frame_pass_kernel<VAR, 1, false>;
        return launch_traversal(kern, trace_grid(a.f.eye.n), a.f.tp.stack_depth, stream, a);
    });
}

mr_status launch_gather_eye_queries_pass(const DeviceScene &ds, const char *who, const mr_frame_desc &fd, const mr_lens_desc *lens,
                                         const FramePass &pass, const mr_hit *d_hits, const float *d_normal, float *d_pos, float *d_nrm,
                                         unsigned long long *d_queries, hipStream_t stream) {
    EyePassQueryArgs a = {};
    const mr_status st = frame_window_of(who, fd, a.eye);
    if (st != MR_OK) return st;
    if (a.eye.n == 0) return MR_OK;
    if (lens) a.ln = lens_params_of_frame(fd, *lens);
    a.base = pass.base;
    a.m = rec::mesh_of(ds);
    a.hits = d_hits; a.normal = d_normal; a.pos = d_pos; a.nrm = d_nrm; a.queries = d_queries;
    if (lens) hipLaunchKernelGGL(gather_eye_queries_pass_kernel<true>, dim3(grid_for(a.eye.n)), dim3(kBlock), 0, stream, a);
    else hipLaunchKernelGGL(gather_eye_queries_pass_kernel<false>, dim3(grid_for(a.eye.n)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
