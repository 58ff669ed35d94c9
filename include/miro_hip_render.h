/* miro_hip_render.h -- the frame call of the miro_hip C ABI that also emits the next level of the recursion, declared outside
 * miro_hip.h, miro_hip_surface.h and miro_hip_frame.h.  miro_hip.h includes this file, so a caller includes miro_hip.h alone.
 * Why a fourth file: tests hold the lists of functions that those three declare at 69, 9 and 3 names; an entry point added
 * since is declared here and listed in miro_amd.binding.RENDER_SYMBOLS, which load_library() requires of the library in the
 * same way. */
#ifndef MIRO_HIP_RENDER_H
#define MIRO_HIP_RENDER_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the level-0 frame over the scene's light list AND the rays of level 1, in ONE launch ----------------------------------
 * mr_render_lights_environment (miro_hip_frame.h) renders level 0 of a frame and stops there; mr_trace_level_lights and
 * mr_trace_level_lights_path run one level of Scene::traceScene's recursion for a queue and emit the next one.  A recursive frame
 * therefore ran level 0 through the level calls: pixel slots zeroed, mr_gen_eye_rays' 32 bytes per sample written and read back,
 * float atomics into the pixels.  This call is the frame that writes the children itself: a recursive frame is
 *   mr_render_level_lights -> mr_trace_level_lights[_path] per further level
 * with no eye-ray buffer, no zeroing pass and no atomics at level 0, whose pixels are plain stores and so deterministic.
 *
 * The frame half.  d_rgb, d_hits, d_sample_rgb, d_sample_color, d_sample_normal and the FIVE counters of d_counts are, bit for
 *   bit, those of mr_render_lights_environment on the same scene and descriptor when level->environment == 1.  With
 *   level->environment == 0 a miss is worth 0 whatever mr_scene_set_environment holds: the outputs are those of
 *   mr_render_lights_surface, and d_counts[3] (live samples that missed) is still counted ([4] stays as it was).  Window, bands,
 *   spp (a power of two <= 64), jitter, tiled order, optional outputs, alignment rules, the uploads (texture table; environment
 *   image with environment == 1) and the capture rule are that call's.  frame->flags: MR_MATH_PRODUCT and MR_TRACE_INCOHERENT
 *   only -- shadow rays are closest-hit, as in the level calls; MR_TRACE_ANY is refused.
 * The children half.  With level->children == MR_LEVEL_SPECULAR the output queue receives the children that
 *   mr_trace_level_lights(children = MR_LEVEL_SPECULAR) emits, with MR_LEVEL_PATH those that mr_trace_level_lights_path(children
 *   = MR_LEVEL_PATH, the same path_kinds, seed = path_seed, bounce = 0) emits, when that call runs on the queue that
 *   mr_gen_eye_rays[_tiled] makes for the same window, seed and order, with d_weights = NULL, d_ids = NULL and d_pixels[k] = the
 *   window pixel of sample k: the same set -- ray, weight, pixel, and with MR_LEVEL_PATH also id, octant and low-res byte of every
 *   child id -- in another order, and an equal d_out_count.  A child's pixel is row * W + x, the index of its pixel in THIS call's
 *   d_rgb (row counts the window's rows in band order), so a later level adds into the same buffer with spp = frame->spp.  A
 *   sample's id is its index in the launch's own sample order (image or tiled).  d_out_ids (optional) is written with
 *   MR_LEVEL_PATH only; d_out_octants and d_out_lowres are optional.  Capacity rule (a child whose slot lies beyond out_capacity
 *   is counted, not stored: none of its outputs is written) and d_out_count (zeroed by the call, then += children, stored or not)
 *   are mr_trace_level's.
 * With level->children == MR_LEVEL_LAST the call is mr_render_lights_environment (environment == 0: with a miss worth 0): no
 *   children, the queue arguments and d_out_count are ignored.
 * An empty window is MR_OK and launches nothing after zeroing d_out_count.  After the uploads the call enqueues the zeroing of
 *   d_out_count (a one-word kernel, so that a graph replays it as written) plus ONE kernel on `stream` and can be captured.
 *
 * Errors.  MR_ERR_INVALID from the arguments alone, before the scene's state is read and before any device call:
 *   mr_render_lights_environment's, in its order, under this call's name (NULL scene / frame / d_rgb, empty image, spp, bands,
 *   rows, size, flags it does not know, misaligned frame buffers); then NULL level; MR_TRACE_ANY; unknown children; environment
 *   > 1; with MR_LEVEL_PATH, path_kinds 0 or with unknown bits; non-zero reserved words; children without an output queue
 *   (d_out_rays, d_out_weights, d_out_pixels, d_out_count) or, on a window that is not empty, with out_capacity 0; misalignment
 *   (out rays 16 bytes, d_out_count 8, weights, pixels and ids 4; octants and low-res bytes may lie anywhere).  MR_ERR_STATE: a
 *   scene that is unbuilt, built host_only, or has no lights.  Square lights are not part of this call; the thin lens is
 *   mr_render_level_lights_lens (miro_hip_lens.h), this call with a mr_lens_desc. */
typedef struct mr_frame_level_desc {
    uint32_t children;                 /* MR_LEVEL_LAST, MR_LEVEL_SPECULAR or MR_LEVEL_PATH */
    uint32_t environment;              /* 0: a miss is worth 0.  1: Scene::getEnvironmentMap of mr_scene_set_environment */
    uint32_t path_kinds, path_seed;    /* as in mr_gen_path_rays; read with MR_LEVEL_PATH (bounce is 0) */
    uint32_t out_capacity_lo, out_capacity_hi;
    uint32_t reserved[6];              /* must be 0 */
    uint8_t *d_out_octants;            /* may be NULL */
    uint8_t *d_out_lowres;             /* may be NULL; MR_LEVEL_PATH: per stored child, 1 = made by Ray::random */
} mr_frame_level_desc;
mr_status mr_render_level_lights(mr_scene *scene, const mr_frame_desc *frame, const mr_frame_level_desc *level,
                                 float *d_rgb, mr_hit *d_hits, float *d_sample_rgb, float *d_sample_color, float *d_sample_normal,
                                 mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids,
                                 uint64_t *d_out_count, uint64_t *d_counts, void *stream);

#ifdef __cplusplus
}
#endif
#include "miro_hip_recursion.h"       /* the whole recursive frame as one call, which chains the call above with the level kernels */
#endif /* MIRO_HIP_RENDER_H */
