// mr_frame_lights_surface.hip -- mr_frame_lights.hip's frame on ANY scene (mr_render_lights_surface): the reference's per-pixel
// loop (Scene::raytraceImage, Scene.cpp:112-141) over the scene's light list as one launch, with what Scene::trace and
// Phong::shade do on a TexturedPhong in between:
//
//   Camera::eyeRay  ->  Scene::trace, which bump-maps the normal of a STONE hit and normalises (Scene.cpp:234-263)  ->
//   diffuseColor = the texture's lookup (Phong.cpp:51-56, all seven kinds)  ->  the loop over Scene::lights() (:59-156)  ->
//   the pixel's mean (Scene.cpp:126-139)
//
// It is frame_lights_kernel with a TexParams argument and one more step: between the primary trace and the light loop the
// per-hit step of the surface pass, hit_color_normal (mr_hit_surface_body.h), and then the loop of shade_lights_body
// (mr_lights_body.h) as its kColorSurface source runs it -- the colour where `dc` goes, the bumped normal everywhere N goes,
// the occluder's light scale from the occluder's own geometric normal (light_scale_of).  Every piece is the shared definition
// under -ffp-contract=off, called in the batched chain's order, so hit records, per-sample colour, normal and L and the pixels
// are the bits of mr_gen_eye_rays[_tiled] -> mr_trace -> mr_hit_surface -> mr_shade_lights_surface(d_ray_rgb) -> pairwise
// mean; tests/test_frame_lights_surface.py compares them.  That chain keeps 32 + 16 + 12 + 12 + 12 bytes per sample resident;
// this kernel writes 12 bytes per pixel (plus, on request, the hit record, L, colour and normal of every sample).
//
// Why the lookup may sit in a kernel that traverses (mr_procedural.hip's header says it may not): as in the photon walk on
// textured scenes, it lies BETWEEN two traversals.  Across it a lane keeps the sample index, the hit's primitive, P and N; the
// eye ray's direction is computed again after it (eye_sample_of / eye_ray_of give the same bits), as pixel and row are after
// the loop.  Across a shadow traversal a lane keeps what frame_lights_kernel keeps and the colour: three registers more.
// The 512 bytes of the two noise tables are static LDS beside the dynamic stack, staged once per workgroup
// (photon_walk_surface_kernel does the same).  hit_color_normal's test of mat_tex is taken out of the loop as
// hit_surface_kernel takes it out: without a texture table the plain arm alone runs, and the frame is mr_render_lights'.
//
// A miss contributes 0 (m_bgColor = 0), as in mr_render_lights.  The frame that gives a miss the scene's environment is
// mr_frame_lights_env.hip (mr_render_lights_environment): the per-sample body of both is one template,
// frame_lights_surface_body<VAR, ANY, ENV> of mr_frame_lights_surface_body.h, instantiated here with ENV = false.
//
// Waves per SIMD, spilled VGPRs and scratch bytes per lane of the 12 kernels (hipcc, gfx950, the Makefile's flags); the
// envelope is the worst kernel of tests/golden/kernel_budget.json, 30 spilled VGPRs / 108 bytes / 4 waves, and every variant
// takes the most waves at which both of its shadow-ray forms stay inside it (frame_lights_surface_waves):
//
//   variant                     waves   closest-hit shadow rays   any-hit shadow rays
//   kTraceExact (1818)            4          0 / 100                  0 / 100
//   kTraceExactObj (826)          4          0 / 100                  0 / 100
//   kTraceProduct (267)           5          6 /  92                  4 /  84
//   kTraceProductObj (43)         4          0 / 100                  0 / 100
//   kTraceVote (88)               5          4 /  84                  4 /  84
//   kTraceVoteProduct (73)        5          5 /  88                  5 /  88
//
// One wave more is outside it: at five kTraceExact has 10 / 140, kTraceExactObj 14 / 156, kTraceProductObj 10 / 140 and 8 / 132;
// at six only the any-hit form of kTraceProduct (10 / 108) is inside.  Of the scratch figure 68 bytes (100 for the variants at
// four waves) are reported without a spilled VGPR, and the four-wave code holds no scratch instruction.  Carrying the eye
// ray's direction across the lookup instead of computing it again puts kTraceProduct at 120 / 116 bytes at five waves; one
// hit_color_normal call for both cases of mat_tex costs 2 to 4 more spilled VGPRs in every variant.  Times against the batched
// chain: DESIGN section 5c, profiles/frame_lights_surface_ab.log.
#include <hip/hip_runtime.h>

#include "mr_frame_lights_surface_body.h"

namespace mr {
namespace {

// MIRO_FRAME_LIGHTS_SURFACE_WAVES (A/B builds) sets one value for every variant.
#ifdef MIRO_FRAME_LIGHTS_SURFACE_WAVES
constexpr int frame_lights_surface_waves(int) { return MIRO_FRAME_LIGHTS_SURFACE_WAVES; }
#else
constexpr int frame_lights_surface_waves(int var) { return var == kTraceProduct || var == kTraceVote || var == kTraceVoteProduct ? 5 : 4; }
#endif

// VAR, ANY: as in frame_lights_kernel.  The arguments are taken BY VALUE (mr_lights_body.h says why).  The body is
// frame_lights_surface_body<VAR, ANY, false> (mr_frame_lights_surface_body.h): no environment.
template <int VAR, bool ANY>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(frame_lights_surface_waves(VAR), 8))) void frame_lights_surface_kernel(
    const FrameLightsSurfaceArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    __shared__ uint32_t s_tab[128];
    frame_lights_surface_body<VAR, ANY, false>(a, EnvParams{}, s_stack, s_tab);
}

}  // namespace

mr_status launch_frame_lights_surface(const LightScene &ls, const mr_frame_desc &fd, const FrameOutputs &o, hipStream_t stream) {
    FrameLightsSurfaceArgs a;
    const mr_status st = fill_frame_lights_surface_args(a, "mr_render_lights_surface", ls, fd, o);
    if (st != MR_OK) return st;
    if (a.eye.n == 0) return MR_OK;

    // the traversal variants of launch_frame_lights: the same hit records from each of them
    const bool any = fd.flags & MR_TRACE_ANY;
    const DeviceScene &ds = *ls.ds;
    return with_trace_variant(ds.n_planes || ds.n_spheres, fd.flags & MR_MATH_PRODUCT, fd.flags & MR_TRACE_INCOHERENT, [&](auto var) -> mr_status {
        constexpr int VAR = decltype(var)::value;
        const auto kern = any ? &frame_lights_surface_kernel<VAR, true> : &frame_lights_surface_kernel<VAR, false>;
        return launch_traversal(kern, trace_grid(a.eye.n), a.tp.stack_depth, stream, a);
    });
}

}  // namespace mr
