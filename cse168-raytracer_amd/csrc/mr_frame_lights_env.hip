// mr_frame_lights_env.hip -- mr_frame_lights_surface.hip's frame with the environment for rays that miss
// (mr_render_lights_environment): the reference's per-pixel loop (Scene::raytraceImage, Scene.cpp:112-141) at level 0 as one
// launch, background included --
//
//   Camera::eyeRay  ->  Scene::traceScene: a hit is shaded as in mr_frame_lights_surface.hip (bump-mapped normal, diffuseColor,
//   the loop over Scene::lights()); a ray that leaves the scene returns getEnvironmentMap(ray) (Scene.cpp:338-342, 657-688)  ->
//   the pixel's mean (Scene.cpp:126-139)
//
// The kernel is frame_lights_surface_body<VAR, ANY, true> (mr_frame_lights_surface_body.h), the body mr_frame_lights_surface.hip
// instantiates with ENV = false: between the primary traversal and the light loop a live lane that missed computes its eye
// ray's direction again and takes m_bgColor, or LoadedTexture::lookup of the full-resolution lat-long image (env_lookup_full,
// mr_environment_body.h -- the definition shade_environment_kernel calls), as its L.  An eye ray is never isDiffuse: the
// low-res image is never read and no LDS is spent on it.  Every piece is the shared definition under -ffp-contract=off, so hit
// records, per-sample colour, normal and L and the pixels are the bits of
//   mr_gen_eye_rays[_tiled] -> mr_trace -> mr_hit_surface -> mr_shade_lights_surface(d_ray_rgb) || mr_shade_environment(d_ray_rgb)
//   -> pairwise mean
// (a sample's L: the light chain's row where it hit, the environment chain's row where it missed);
// tests/test_frame_lights_environment.py compares them.  That chain keeps 32 + 16 + 12 + 12 + 12 bytes per sample resident and
// streams every ray and hit record once more to find the misses; this kernel has the hit flag in a register.
//
// Colour or image is a wave-uniform branch on env.full, not a template argument: see the table.
//
// Waves per SIMD, spilled VGPRs and scratch bytes per lane of the 12 kernels (hipcc, gfx950, the Makefile's flags); the
// envelope is the worst kernel of tests/golden/kernel_budget.json, 30 spilled VGPRs / 108 bytes / 4 waves
// (frame_lights_env_waves):
//
//   variant                     waves   closest-hit shadow rays   any-hit shadow rays
//   kTraceExact (1818)            4          0 /  68                  0 /  68
//   kTraceExactObj (826)          4          0 /  68                  0 / 100
//   kTraceProduct (267)           4          0 /  68                  0 /  68
//   kTraceProductObj (43)         4          0 /  68                  0 / 100
//   kTraceVote (88)               4          0 /  68                  0 /  68
//   kTraceVoteProduct (73)        4          0 /  68                  0 /  68
//
// Every variant runs at four waves, where none spills a VGPR.  At five, with the lookup
// in, all twelve leave the envelope's scratch figure, the three that mr_frame_lights_surface.hip runs at five included:
// kTraceProduct 12 / 116 and 11 / 112, kTraceVote 11 / 112, kTraceVoteProduct 12 / 116 (kTraceExact 16 / 128, kTraceExactObj
// 25 / 152 and 25 / 184, kTraceProductObj 15 / 124 and 13 / 152).  With colour or image as a branch no variant loses a wave
// against four, so it is no template argument.  Times against the batched chain and against mr_render_lights_surface: DESIGN
// section 5c, profiles/frame_lights_env_ab.log.
#include <hip/hip_runtime.h>

#include "mr_frame_lights_surface_body.h"

namespace mr {
namespace {

struct FrameLightsEnvArgs {
    FrameLightsSurfaceArgs f;
    EnvParams env;               // full nullptr: colour only (bg); low / lw / lh are not read
};

// MIRO_FRAME_LIGHTS_ENV_WAVES (A/B builds) sets one value for every variant.
#ifdef MIRO_FRAME_LIGHTS_ENV_WAVES
constexpr int frame_lights_env_waves(int) { return MIRO_FRAME_LIGHTS_ENV_WAVES; }
#else
constexpr int frame_lights_env_waves(int) { return 4; }
#endif

// VAR, ANY: as in frame_lights_kernel.  The arguments are taken BY VALUE (mr_lights_body.h says why).
template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(frame_lights_env_waves(VAR), 8))) void frame_lights_env_kernel(
    const FrameLightsEnvArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    frame_lights_surface_body<VAR, ANY, true>(a.f, a.env, s_stack, s_tab);
}

}  // namespace

mr_status launch_frame_lights_env(const LightScene &ls, const mr_frame_desc &fd, const FrameOutputs &o, hipStream_t stream) {
    FrameLightsEnvArgs a;
    const mr_status st = fill_frame_lights_surface_args(a.f, "mr_render_lights_environment", ls, fd, o);
    if (st != MR_OK) return st;
    if (a.f.eye.n == 0) return MR_OK;
    a.env = ls.env;

    // the traversal variants of launch_frame_lights: the same hit records from each of them
    const bool any = fd.flags & MR_TRACE_ANY;
    const DeviceScene &ds = *ls.ds;
    return with_trace_variant(ds.n_planes || ds.n_spheres, fd.flags & MR_MATH_PRODUCT, fd.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        const auto kern = any ? &frame_lights_env_kernel<VAR, true> : &frame_lights_env_kernel<VAR, false>;
        return launch_traversal(kern, trace_grid(a.f.eye.n), a.f.tp.stack_depth, stream, a);
    });
}

}  // namespace mr
