/* miro_hip_frame.h -- the fused frame calls of the miro_hip C ABI declared outside miro_hip.h and miro_hip_surface.h.
 * miro_hip.h includes this file, so a caller includes miro_hip.h alone.  Why a third file: tests hold the list of functions
 * that miro_hip.h itself declares at 69 names and the list of miro_hip_surface.h at 9; an entry point added since is declared
 * here and listed in miro_amd.binding.FRAME_SYMBOLS, which load_library() requires of the library in the same way. */
#ifndef MIRO_HIP_FRAME_H
#define MIRO_HIP_FRAME_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the whole level-0 frame over the scene's light list in ONE launch, the environment of rays that miss included ------
 * mr_render_lights_surface (miro_hip_surface.h) in every respect -- window, bands, spp, jitter, tiled order, flags, lights,
 * materials, the texture table or none, optional outputs, alignment rules and the order of the errors -- but for three things.
 *
 * The value of a miss.  A live sample whose primary ray misses is worth Scene::getEnvironmentMap(ray) (Scene.cpp:657-688), what
 *   Scene::traceScene returns for a ray that leaves the scene (Scene.cpp:338-342), of the environment of
 *   mr_scene_set_environment: bg_color without an image; with one, LoadedTexture::lookup of the FULL-RESOLUTION image at the eye
 *   ray's direction (an eye ray is never isDiffuse: the low-res copy is not read).  The value is the sample's L: it goes to
 *   d_sample_rgb and into the pixel's mean exactly as a hit's L does.  A lookup the reference leaves undefined is defined as 0
 *   and counted, as in mr_shade_environment.  Samples past the end of the window are not misses.
 * The counters.  d_counts is FIVE words (8-byte aligned, not zeroed by the call): [0..2] as in mr_render_lights_surface,
 *   [3] += live samples that missed, [4] += undefined environment lookups -- mr_shade_environment's d_counts[0] and [1] on the
 *   same batch.
 * The upload.  The first call after mr_scene_set_environment with an image uploads it on `stream` -- an allocation and a copy --
 *   and must lie outside a stream capture, the rule of the texture table (every other call that reads the image uploads it
 *   too).  After that, with a texture table that is already on the device, the call enqueues ONE kernel on `stream` and can be
 *   captured into a graph.
 *
 * The contract.  Hit records, per-sample colour, per-sample normal, per-sample L and the three counters [0..2] are, bit for bit,
 * those of the batched
 *   mr_gen_eye_rays[_tiled] -> mr_trace -> mr_hit_surface -> mr_shade_lights_surface(d_ray_rgb) || mr_shade_environment(flags 0,
 *   d_ray_rgb) -> pairwise mean over each pixel's samples
 * on the same scene, camera, seed and sample order: the L of a sample is the light chain's row where it hit and the environment
 * chain's row where it missed.  With no environment set (bg_color 0, no image) every output is mr_render_lights_surface's, bit
 * for bit.  The batched route keeps 84 bytes per sample resident and streams every ray and hit record once more to find the
 * misses; this call keeps 12 bytes per pixel.
 * Errors: mr_render_lights_surface's, in its order, under this call's name. */
mr_status mr_render_lights_environment(mr_scene *scene, const mr_frame_desc *frame, float *d_rgb, mr_hit *d_hits,
                                       float *d_sample_rgb, float *d_sample_color, float *d_sample_normal, uint64_t *d_counts,
                                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRO_HIP_FRAME_H */
