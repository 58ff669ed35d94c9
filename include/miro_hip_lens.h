/* miro_hip_lens.h -- the fused level-0 frame and the one-call recursive frames of the miro_hip C ABI for the THIN-LENS camera
 * (Camera::eyeRay under -DDOF, Camera.cpp:135-160; DOF_APERTURE / DOF_FOCUS_PLANE, Miro.h:18-19).
 * miro_hip_recursion_photons.h includes this file as its last line, below its declarations, so a caller includes miro_hip.h alone.
 * Why a seventh file: tests hold the lists of functions that the six others declare at 69, 9, 3, 1, 2 and 2 names; the three
 * entry points here are listed in miro_amd.binding.LENS_SYMBOLS, which load_library() requires of the library in the same way. */
#ifndef MIRO_HIP_LENS_H
#define MIRO_HIP_LENS_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the depth-of-field frame: mr_render_level_lights, mr_render_recursion and mr_render_recursion_photons through a lens ---------
 * The reference's final picture is a depth-of-field frame: under -DDOF Scene::raytraceImage takes its samples of a pixel through
 * points of a lens disc (Camera.cpp:135-160), with DOF_APERTURE = .20f and DOF_FOCUS_PLANE = 15.3f for the flower scene
 * (Miro.h:18-19).  mr_gen_eye_rays_lens (miro_hip.h) makes those rays for the batched calls: 32 bytes per sample in device memory,
 * level 0 through the level calls with zeroed pixel slots and float atomics, a child count read back after every level.  The three
 * calls here are the fused calls of miro_hip_render.h, miro_hip_recursion.h and miro_hip_recursion_photons.h with that camera:
 * the lens ray of a sample is made in registers, wherever the pinhole calls make the eye ray.
 *
 * `lens` (mr_lens_desc, miro_hip.h) follows `frame`; every other argument, output, counter, workspace
 * (mr_render_recursion_workspace, mr_render_recursion_photons_workspace: unchanged), upload and capture rule is that of the
 * call without `_lens`.
 *
 * The contract.  The eye ray of sample k of the window is the ray mr_gen_eye_rays_lens writes for it for the same camera, window,
 *   seed, spp, jitter and lens with d_samples_in == NULL (Camera.cpp:135-160): the sample's key, its jitter, sampleDisc's rejection
 *   loop of at most 32 rounds -- a sample that exhausts them takes the lens centre, as there; it is not counted here and cannot
 *   occur for a real aperture --, the point on the lens, the direction through the focus point.  aperture == 0 is a pinhole
 *   through the lens arithmetic.
 * mr_render_level_lights_lens: Camera.cpp:135-160 with Miro.h:18-19 as level 0.  d_rgb, d_hits, d_sample_rgb, d_sample_color,
 *   d_sample_normal and the five counters of d_counts are, bit for bit, what the batched chain mr_trace -> mr_shade_environment ->
 *   mr_hit_surface -> mr_shade_lights_surface (or mr_trace_level_lights[_path]) writes for those rays; a pixel is the butterfly mean
 *   of its samples, a plain store.  The children are the set mr_trace_level_lights (MR_LEVEL_SPECULAR) or
 *   mr_trace_level_lights_path (MR_LEVEL_PATH, bounce 0) emits on that queue with d_weights = NULL, d_ids = NULL and d_pixels[k]
 *   the window pixel of sample k, and d_out_count is equal.  MR_LEVEL_LAST is served by this call's own kernels: no children, the
 *   queue arguments and d_out_count are ignored.
 * mr_render_recursion_lens: Camera.cpp:135-160 with Miro.h:18-19 as level 0 of mr_render_recursion.  Level 0 is
 *   mr_render_level_lights_lens (depth 0: with MR_LEVEL_LAST); levels >= 1 are mr_render_recursion's own kernels -- a child does
 *   not know what camera made its parent.  d_level_counts keeps its meaning, [l][6] = [l][7] = 0.
 * mr_render_recursion_photons_lens: Camera.cpp:135-160 with Miro.h:18-19 as level 0 of mr_render_recursion_photons.  Level 0's
 *   queries are formed from the lens ray of sample k made again; d_level_counts[l][6] the queries made at level l, [l][7] = 0.
 *
 * Errors.  MR_ERR_INVALID from the arguments alone, before the scene's state is read and before any device call: the list of the
 *   call without `_lens`, in its order, under this call's name; then NULL lens, non-zero reserved words of mr_lens_desc, an
 *   aperture that is negative or not finite, a focus_plane that is not finite and > 0 (mr_gen_eye_rays_lens' checks); then
 *   frame->tiled != 0 (the generator these calls are held to makes image order only).  Bands and row windows are allowed: the
 *   sample's key uses the image row.  MR_ERR_STATE: the cases of the call without `_lens`.
 * Not part of these calls: caller-supplied lens samples (d_samples_in), square lights, MR_TRACE_ANY. */
mr_status mr_render_level_lights_lens(mr_scene *scene, const mr_frame_desc *frame, const mr_lens_desc *lens,
                                      const mr_frame_level_desc *level, float *d_rgb, mr_hit *d_hits, float *d_sample_rgb,
                                      float *d_sample_color, float *d_sample_normal, mr_ray *d_out_rays, float *d_out_weights,
                                      uint32_t *d_out_pixels, uint32_t *d_out_ids, uint64_t *d_out_count, uint64_t *d_counts,
                                      void *stream);
mr_status mr_render_recursion_lens(mr_scene *scene, const mr_frame_desc *frame, const mr_lens_desc *lens, const mr_recursion_desc *desc,
                                   float *d_rgb, void *d_workspace, uint64_t workspace_bytes,
                                   uint64_t *d_level_counts /* [depth+1][8] */, void *stream);
mr_status mr_render_recursion_photons_lens(mr_scene *scene, const mr_frame_desc *frame, const mr_lens_desc *lens,
                                           const mr_recursion_desc *desc, mr_photon_map *global_map, mr_photon_map *caustic_map,
                                           float max_dist, uint32_t nphotons, float *d_rgb, void *d_workspace,
                                           uint64_t workspace_bytes, uint64_t *d_level_counts /* [depth+1][8] */, void *stream);

#ifdef __cplusplus
}
#endif
/* the frames of more than 64 samples per pixel and the image finish, below the declarations they build on */
#include "miro_hip_passes.h"
#endif /* MIRO_HIP_LENS_H */
