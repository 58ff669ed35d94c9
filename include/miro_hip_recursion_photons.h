/* miro_hip_recursion_photons.h -- the whole recursive frame of miro_hip_recursion.h WITH the photon-map term of Scene::traceScene
 * (irradiance_estimate of the global and the caustic map at every diffuse hit of every level, Scene.cpp:286-299) as ONE call.
 * miro_hip_recursion.h includes this file as its last line, below its declarations, so a caller includes miro_hip.h alone.  Why a
 * sixth file: tests hold the lists of functions that the five others declare at 69, 9, 3, 1 and 2 names; the two entry points
 * here are listed in miro_amd.binding.RECURSION_PHOTONS_SYMBOLS, which load_library() requires of the library in the same way. */
#ifndef MIRO_HIP_RECURSION_PHOTONS_H
#define MIRO_HIP_RECURSION_PHOTONS_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- mr_render_recursion + mr_gather_level at every level, on one stream --------------------------------------------------------
 * mr_gather_level (miro_hip.h) takes the length of its queue from the HOST, so a caller that wants the photon-map term at every
 * level chains mr_render_level_lights -> mr_gather_level -> mr_trace_level_lights[_path] -> mr_gather_level -> ... and reads a
 * child count back after every level.  This call chains them itself: its query, estimate and accumulate kernels read the length
 * of the level's queue from the device word that mr_render_recursion's levels read it from.  After the uploads there is no host
 * read, no allocation and no synchronisation: the call only enqueues kernels on `stream` and can be captured into a graph.
 *
 * What is enqueued.  mr_render_recursion's sequence as it stands -- the zeroing kernel, level 0, one kernel per further level --
 * with every level launch also writing its hit records (and, on a scene whose texture table holds a procedural texture, the
 * normals Scene::trace hands on, bumped on stone) into the workspace, and after each level l three steps:
 *   1. the query kernel on level l's queue: hit point and normal of every ray whose hit has a diffuse material, no query
 *      elsewhere.  Level 0 has no ray buffer; the eye ray of sample k is made again as the frame kernel made it and joined with
 *      the frame's hit record, the bits mr_gather_level forms from mr_gen_eye_rays' buffer of the same window.  Levels >= 1 read
 *      their queue, of min(d_level_counts[l-1][5], queue_capacity) rays;
 *   2. one k-NN estimate (mr_irradiance_estimate's search, nphotons, max_dist) per map given;
 *   3. the accumulate: weight x (irradiance + caustic) / spp added to the ray's pixel of d_rgb with float atomics; at level 0 the
 *      weight is 1 and the pixel is k / spp.
 *   Stream order keeps level l's three steps ahead of level l + 1, which overwrites queue l's storage.  The grids are sized from
 *   min(queue_capacity, fan^l x samples); a level whose queue is empty still launches them, and each estimate launch leaves the
 *   map's hand-out counter as it found it.  A captured call holds the hand-out counters the maps gave it.
 * d_level_counts[l]: [0..5] as in mr_render_recursion; [6] the queries made at level l (diffuse hits); [7] = 0.
 * Workspace: mr_render_recursion_workspace(desc) bytes (the two queues) first, then, with
 *   M = max(samples of frame's window, depth >= 1 ? queue_capacity : 0) and each array's size rounded up to 16 bytes:
 *   16 M bytes of hit records, 12 M bytes of normals, 48 M bytes of scratch (mr_gather_level's layout for the level's bound n:
 *   [0, 3n) positions, [3n, 6n) normals, [6n, 9n) the global map's estimates, [9n, 12n) the caustic map's, in floats).
 *   mr_render_recursion_photons_workspace returns the total; it is host-only and reads nothing but the two descriptors.
 *   d_workspace must be 16-byte aligned and workspace_bytes at least that total; with depth 0 a workspace is still needed.
 * The first call after mr_scene_set_textures / mr_scene_set_environment uploads, as in mr_render_recursion, and must lie outside
 *   a stream capture.
 *
 * Errors.  MR_ERR_INVALID from the arguments alone, before the scene's or a map's state is read and before any device call:
 *   mr_render_recursion's list under this call's name; both maps NULL; nphotons outside [1, 512]; max_dist that is not positive
 *   (NaN included); frame->tiled (the level-0 pixel is k / spp, image order); a NULL or misaligned workspace or workspace_bytes
 *   too small, at any depth; 2^31 samples or more, or a queue_capacity of 2^31 or more (one estimate launch answers at most
 *   2^31 - 1 queries).  MR_ERR_STATE: mr_render_recursion's cases; a map that is not balanced and resident, or lives on another
 *   device than the scene.  A scene with a procedural texture is accepted: the call passes the normal buffer itself.
 * The thin lens is not part of this call: mr_render_recursion_photons_lens (miro_hip_lens.h) is this call with it. */
mr_status mr_render_recursion_photons_workspace(const mr_frame_desc *frame, const mr_recursion_desc *desc, uint64_t *bytes);   /* host only */
mr_status mr_render_recursion_photons(mr_scene *scene, const mr_frame_desc *frame, const mr_recursion_desc *desc,
                                      mr_photon_map *global_map, mr_photon_map *caustic_map, float max_dist, uint32_t nphotons,
                                      float *d_rgb, void *d_workspace, uint64_t workspace_bytes,
                                      uint64_t *d_level_counts /* [depth+1][8] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRO_HIP_RECURSION_PHOTONS_H */
#include "miro_hip_lens.h"
