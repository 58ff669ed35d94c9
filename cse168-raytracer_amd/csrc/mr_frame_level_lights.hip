// mr_frame_level_lights.hip -- the level-0 frame of mr_frame_lights_env.hip that also writes the rays of level 1
// (mr_render_level_lights): the reference's per-pixel loop (Scene::raytraceImage, Scene.cpp:112-141) and the first level of
// Scene::traceScene's recursion (Scene.cpp:270-346) as one launch --
//
//   Camera::eyeRay  ->  Scene::trace, the bump-mapped normal included  ->  a ray that leaves the scene: getEnvironmentMap(ray)  ->
//   a hit: diffuseColor, Phong::shade's loop over Scene::lights()  ->  the pixel's mean (Scene.cpp:126-139), a plain store  ->
//   the children of the next level, compacted into its queue
//
// It joins the two families of single-launch kernels over the light list.  The frame family (frame_lights_surface_body<VAR, ANY,
// ENV>, mr_frame_lights_surface_body.h) holds the eye ray in registers and keeps 12 bytes per pixel, but stops at level 0.  The
// level family (mr_level_lights.hip, mr_level_lights_path.hip) emits children, but of a QUEUE: run at level 0 it needs the pixel
// slots zeroed, mr_gen_eye_rays' 32 bytes per sample written to HBM and read back twice, the pixel re-derived from the ray index
// and float atomics for a sum whose terms all sit in one wave.  Here the kernel is frame_lights_surface_body<VAR, false, true,
// CHILDREN>: the frame body with the level kernels' last step in it, with the eye as the ray's origin, weight 1 and pixel row * W + x --
//   CHILDREN 1 (MR_LEVEL_SPECULAR)  rec::ChildGen<false> about the normal Scene::trace hands on -- the surface step's, which only a STONE
//                                   material bumps (a reflective one's mirror child bounces about the bumped normal, as the
//                                   BUMPED level kernels' do) -- rec::write_children
//   CHILDREN 2 (MR_LEVEL_PATH)      rec::ChildGen<true> about the normal of the surface step, hray = pcg32(pcg32(seed) ^ sample
//                                   index), the diffuse child with the looked-up colour, write_children_col (mr_children_col.h)
// -- one body with one more template argument, not a second body: with CHILDREN == 0 nothing of it is compiled, and the records
// of the two frame units and the two level units hold as they stood.  Every piece is the shared definition under
// -ffp-contract=off: the frame half is mr_render_lights_environment's bits (with an all-zero environment,
// mr_render_lights_surface's), the children are the set the level kernels emit on mr_gen_eye_rays[_tiled]'s queue, in another
// order.  Level 0's pixels are stores: deterministic.
//
// The environment is a runtime matter (ENV = true; environment == 0 hands the body bg = 0 and no image, so a miss is worth 0 and
// is still counted), as are the texture table and the optional outputs: wave-uniform branches.  Shadow rays are closest-hit
// (ANY = false), what the level kernels trace.  Twelve kernels: the six traversal variants x two kinds of children.
//
// Live state: the sample and the eye ray are computed again where they are needed, as in the frame body.  The children step
// stands BEFORE the light loop (the body says why): it reads the hit point, the normal of the surface step, the colour, the
// direction and the material pointer, which the light loop needs anyway, and nothing of it -- not the hit record, not the queue's
// arguments -- lives across the shadow traversals.
//
// The unit is compiled WITHOUT machine-level loop-invariant code motion (the Makefile's FRAME_LEVEL_FLAGS).  With that pass, what
// the sample loop computes from uniform values alone -- the reciprocals of eye_sample_of's divisions, the double constants of the
// path tracer's generators, the compaction's lane mask -- is moved in front of the loop and stays live across every traversal in
// it: 166 to 289 spilled SGPRs and up to 10 spilled VGPRs per kernel, all 128 registers taken, every spill in the loop's prologue.
// Without it the values are made where they are used.
//
// Waves per SIMD, VGPRs, spilled VGPRs and scratch bytes per lane (hipcc, gfx950, the Makefile's flags); the envelope is the worst
// kernel of tests/golden/kernel_budget.json, 30 spilled VGPRs / 108 bytes / 4 waves:
//
//                                 MR_LEVEL_SPECULAR               MR_LEVEL_PATH                  with the pass (spilled / scratch)
//   variant                     waves  VGPRs  spilled / scratch   waves  VGPRs  spilled / scratch   specular     path
//   kTraceExact (1818)            4     109      0 /  68            4     110      0 /  68           4 /  84     6 /  92
//   kTraceExactObj (826)          4     114      0 /  68            4     115      0 /  68           9 / 104    10 / 140
//   kTraceProduct (267)           4      99      0 /  68            4     100      0 /  68           0 /  68     0 /  68
//   kTraceProductObj (43)         4     103      0 /  68            4     104      0 /  68           0 /  68     5 / 120
//   kTraceVote (88)               4      98      0 /   0            4      99      0 /  68           0 /  68     0 /  68
//   kTraceVoteProduct (73)        5      95      0 /   0            5      96      0 / 100           0 /  68     0 / 100
//
// No kernel spills a VGPR, every one is inside the envelope; with the pass the two path-traced kernels for scenes with spheres
// or planes were outside its scratch figure (140 and 120 bytes; at 128 VGPRs and four waves throughout).  Tried with the pass on,
// and not enough to get those two under 108 bytes: waves_per_eu(4, 4), the queue's arguments staged through LDS, per-wave counters
// in scalar registers, an opaque copy of the thread index for the compaction.  None of them is in the code.
//
// d_out_count is zeroed by a one-word kernel, not a memset node (launch_zero_count; mr_level_lights.hip says why).  Times against the
// level kernels at level 0: DESIGN section 5c, profiles/frame_level_lights_ab.log.
#include <hip/hip_runtime.h>

#include "mr_frame_lights_surface_body.h"

namespace mr {
namespace {

struct FrameLevelLightsArgs {
    FrameLightsSurfaceArgs f;
    EnvParams env;               // all zero without `environment`; full nullptr: colour only (bg); low / lw / lh are not read
    FrameChildArgs ch;
};

#ifndef MIRO_FRAME_LEVEL_LIGHTS_WAVES
#define MIRO_FRAME_LEVEL_LIGHTS_WAVES 4
#endif

// VAR: as in frame_lights_kernel; CHILDREN: 1 specular, 2 path tracing.  The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, int CHILDREN>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(MIRO_FRAME_LEVEL_LIGHTS_WAVES, 8))) void frame_level_lights_kernel(
    const FrameLevelLightsArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    frame_lights_surface_body<VAR, false, true, CHILDREN>(a.f, a.env, a.ch, s_stack, s_tab);
}

}  // namespace

mr_status frame_level_lights_samples(const char *who, const mr_frame_desc &fd, unsigned long long &n) {
    EyeFrame eye;
    const mr_status st = frame_window_of(who, fd, eye);
    if (st == MR_OK) n = eye.n;
    return st;
}

mr_status launch_frame_level_lights(const LightScene &ls, const mr_frame_desc &fd, const mr_frame_level_desc &ld, const FrameOutputs &o,
                                    const RayQueue &out, unsigned long long *d_out_count, hipStream_t stream) {
    FrameLevelLightsArgs a;
    mr_status st = fill_frame_lights_surface_args(a.f, "mr_render_level_lights", ls, fd, o);
    if (st != MR_OK || (st = launch_zero_count(d_out_count, stream)) != MR_OK) return st;
    if (a.f.eye.n == 0) return MR_OK;
    a.env = ls.env;
    fill_frame_child_args(a.ch, ld, out, d_out_count);

    // the traversal variants of launch_frame_lights_env / launch_level_lights: the same hit records from each of them
    const DeviceScene &ds = *ls.ds;
    return with_trace_variant(ds.n_planes || ds.n_spheres, fd.flags & MR_MATH_PRODUCT, fd.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        const auto kern = ld.children == MR_LEVEL_PATH ? &frame_level_lights_kernel<VAR, 2> : &frame_level_lights_kernel<VAR, 1>;
        return launch_traversal(kern, trace_grid(a.f.eye.n), a.f.tp.stack_depth, stream, a);
    });
}

}  // namespace mr
