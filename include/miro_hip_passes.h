/* miro_hip_passes.h -- the one-call recursive frames of the miro_hip C ABI at ANY sample count, and the image finish
 * (Scene::raytraceImage under -DDOF / -DPATH_TRACING: TRACE_SAMPLES = 1000 samples per pixel, Miro.h:15, Scene.cpp:126-139; the
 * tone map whose NaN channels are first replaced by the image's maximum, Scene.cpp:150-163, 184-197; Image.cpp:47-52).
 * miro_hip_lens.h includes this file below its declarations, so a caller includes miro_hip.h alone.
 * Why an eighth file: tests hold the lists of functions that the seven others declare at 69, 9, 3, 1, 2, 2 and 3 names; the four
 * entry points here are listed in miro_amd.binding.PASSES_SYMBOLS, which load_library() requires of the library in the same way. */
#ifndef MIRO_HIP_PASSES_H
#define MIRO_HIP_PASSES_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- sample passes ----------------------------------------------------------------------------------------------------------
 * The fused frames take frame->spp as a power of two up to 64: a pixel's samples are the lanes of one wave.  A frame of
 * S = spp_total samples per pixel is rendered in PASSES: a pass renders samples [base, base + p) of every pixel of the window, p a
 * power of two <= 64, through the parent call's kernels at levels >= 1 and a level-0 kernel that differs from the parent's in four
 * places (csrc/mr_frame_passes.hip).  A frame's samples have ONE numbering, 0 .. S - 1 per pixel, that no cut into passes or calls
 * changes:
 *   - sample s of pixel (x, y) draws its jitter and its point on the lens from the key of sample s (what mr_gen_eye_rays[_lens]
 *     makes for spp = S);
 *   - its path hash and the id of its children come from pixel * S + s, the sample's index in a single launch at spp = S, so every
 *     level >= 1 draws from the ids that launch would hand it;
 *   - a pixel is the sum of its samples' terms times 1 / S (S > 1).
 * So the picture is defined by (seed, S) up to the order of float additions into a pixel, which is the plan's: per-level counts,
 * summed over the passes, are exactly those of one call at spp = S where such a call exists, and pixels agree to the bound the
 * project holds reordered float pixel sums to (rtol 1e-5, atol 1e-6 x max|rgb|).
 *
 * The plan (mr_render_passes_plan states it; host only, no device call):
 *   - sample_begin is a multiple of frame->spp;
 *   - whole passes of frame->spp run while they fit below sample_end;
 *   - the remainder follows as powers of two in descending order.
 *   S = 1000, spp = 64: 15 x 64, then 32, then 8.  *n_passes is the number of passes; the first min(capacity, *n_passes) of them are
 *   written to base[] and spp[] (either may be NULL).
 *
 * mr_render_recursion_passes is mr_render_recursion (lens == NULL) or mr_render_recursion_lens, enqueued once per pass of the
 *   plan on `stream`.  The workspace is the one the parent call needs for frame->spp (mr_render_recursion_workspace); the passes
 *   reuse it in stream order.  d_pass_counts is [n_passes][depth + 1][8]: each pass's block has the parent call's meaning and is
 *   zeroed by that pass's own zeroing kernel; the level kernels read their queue length from it.  Truncation is read per pass
 *   ([l][5] > queue_capacity).  The pass with base == 0 STORES its pixels, every other pass ADDS to what d_rgb holds (level 0: a
 *   plain load, add and store by the pixel's one owner lane): a call with sample_begin > 0 continues what an earlier call left in
 *   d_rgb.  After the uploads (texture table, environment: a first call outside a capture) the call only enqueues and can be
 *   captured into a graph.
 * mr_render_recursion_photons_passes is the same over mr_render_recursion_photons[_lens], with that call's maps, nphotons,
 *   max_dist and workspace (mr_render_recursion_photons_workspace for frame->spp); [l][6] of a pass's block are its queries.
 *
 * Errors.  MR_ERR_INVALID from the arguments alone, before the scene's state is read and before any device call: the parent
 *   call's list in its order under this call's name (with lens != NULL the lens checks); then frame->tiled != 0; NULL passes or
 *   non-zero reserved words; spp_total == 0; an empty range or one that runs past spp_total; sample_begin not a multiple of
 *   frame->spp; with depth >= 1, window pixels x spp_total > 2^32 - 1 (ray ids are 32 bits).  d_pass_counts NULL or not 8-byte
 *   aligned is refused with the parent's checks of its counters.  MR_ERR_STATE: the parent call's cases.
 * Not part of these calls: tiled order, caller-supplied lens samples, more than one band range per call, square lights. */
typedef struct mr_passes_desc {
    uint32_t spp_total;                 /* S >= 1 */
    uint32_t sample_begin, sample_end;  /* this call renders samples [begin, end) of every pixel; begin < end <= S */
    uint32_t reserved[5];               /* must be 0 */
} mr_passes_desc;

mr_status mr_render_passes_plan(uint32_t frame_spp, const mr_passes_desc *desc, uint32_t *n_passes, uint32_t *base, uint32_t *spp,
                                uint32_t capacity);
mr_status mr_render_recursion_passes(mr_scene *scene, const mr_frame_desc *frame, const mr_lens_desc *lens_or_NULL,
                                     const mr_recursion_desc *desc, const mr_passes_desc *passes, float *d_rgb, void *d_workspace,
                                     uint64_t workspace_bytes, uint64_t *d_pass_counts /* [n_passes][depth+1][8] */, void *stream);
mr_status mr_render_recursion_photons_passes(mr_scene *scene, const mr_frame_desc *frame, const mr_lens_desc *lens_or_NULL,
                                             const mr_recursion_desc *desc, const mr_passes_desc *passes, mr_photon_map *global_map,
                                             mr_photon_map *caustic_map, float max_dist, uint32_t nphotons, float *d_rgb,
                                             void *d_workspace, uint64_t workspace_bytes,
                                             uint64_t *d_pass_counts /* [n_passes][depth+1][8] */, void *stream);

/* ---- the image finish: Scene.cpp:150-163, 184-197 plus Image.cpp:47-52 -----------------------------------------------------------
 * d_rgb: n_pixels x 3 floats.  The maximum and the minimum run over all channel values with `>` and `<` from -inf and +inf, so a NaN
 * never wins; every NaN channel is replaced by that maximum; then mr_tonemap's sigmoid(6v - 3) and byte map, the same expression
 * and the same bits, into d_out8 (n_pixels x 3 bytes).  d_rgb is not changed.  Two kernels on `stream` and no read-back: a workgroup
 * reduction and one atomic per workgroup on an order-preserving integer image of the float, then the map.  d_minmax (may be NULL):
 * two floats, (maximum, minimum), written for the caller by the second kernel.  An image with no non-NaN value has maximum -inf
 * (minimum +inf) and is all zero bytes.  The first call on a scene allocates three words of device state and must lie outside a
 * stream capture; calls on one scene must follow each other in stream order (they share those words).
 * Errors: MR_ERR_INVALID for NULL scene / d_rgb / d_out8, n_pixels == 0 or > 2^32 - 1, d_rgb or d_minmax not 4-byte aligned. */
mr_status mr_finish_image(mr_scene *scene, const float *d_rgb, uint64_t n_pixels, uint8_t *d_out8, float *d_minmax, void *stream);

#ifdef __cplusplus
}
#endif
#include "miro_hip_bump.h"
#endif /* MIRO_HIP_PASSES_H */
