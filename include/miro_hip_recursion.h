/* miro_hip_recursion.h -- the whole recursive frame of the miro_hip C ABI as ONE call, declared outside miro_hip.h,
 * miro_hip_surface.h, miro_hip_frame.h and miro_hip_render.h.  miro_hip.h includes miro_hip_render.h, which includes this file, so
 * a caller includes miro_hip.h alone.  Why a fifth file: tests hold the lists of functions that those four declare at 69, 9, 3 and
 * 1 names; an entry point added since is declared here and listed in miro_amd.binding.RECURSION_SYMBOLS, which load_library()
 * requires of the library in the same way. */
#ifndef MIRO_HIP_RECURSION_H
#define MIRO_HIP_RECURSION_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Scene::raytraceImage -> Scene::traceScene (Scene.cpp:94-346) for one window: every level, on one stream -----------------
 * mr_render_level_lights (miro_hip_render.h) renders level 0 and writes the rays of level 1; mr_trace_level_lights[_path]
 * (miro_hip_frame.h) run one further level each, and take the length of their queue from the HOST: a caller chaining them reads the
 * child count back after every level.  This call chains them itself.  Its level kernels read the length of their queue from the
 * device word the level before counted its children into, so between the levels there is no read-back, no allocation and no
 * synchronisation: after the uploads (below) the call only enqueues kernels on `stream`, and can be captured into a graph.
 *
 * What is enqueued, for desc->depth = TRACE_DEPTH (levels 0 .. depth are run):
 *   1. one kernel that zeroes d_level_counts, all (depth + 1) x 8 words (a kernel, not a memset node);
 *   2. level 0: mr_render_level_lights' launches on `frame`, straight into d_rgb (plain stores, deterministic), children =
 *      desc->children, its children into queue A of the workspace, their count into d_level_counts[0][5], its five counters into
 *      d_level_counts[0][0..4].  With depth == 0: mr_render_lights_environment (desc->environment == 0: mr_render_lights_surface's
 *      outputs), bit for bit, and no workspace is needed (d_workspace may be NULL, workspace_bytes 0);
 *   3. level l = 1 .. depth: ONE kernel, the level of mr_trace_level_lights (MR_LEVEL_SPECULAR) or mr_trace_level_lights_path
 *      (MR_LEVEL_PATH: path_kinds, seed = path_seed, bounce = l, the queue's ids, and with desc->environment the queue's low-res
 *      bytes) on queue A or B in turn, of min(d_level_counts[l-1][5], queue_capacity) rays, with spp = frame->spp, flags =
 *      (frame->flags & MR_MATH_PRODUCT) | MR_TRACE_INCOHERENT, adding weight x L / spp into d_rgb with float atomics; its children
 *      go to the other queue and their count to d_level_counts[l][5]; the last level emits none.  The grid is sized from
 *      min(queue_capacity, fan^l x samples), fan = 3 (specular) or 4 (path): workgroups beyond the queue's end leave at once, and
 *      a level whose queue is empty still launches its grid.
 * d_level_counts[l], eight 64-bit words per level: [0] rays traced, [1] shadow rays, [2] undefined texture lookups, [3] misses,
 *   [4] undefined environment lookups, [5] children emitted, stored or not, [6] = [7] = 0.  d_level_counts[l][5] >
 *   queue_capacity says that the frame was TRUNCATED at level l: the children beyond the capacity were counted, not stored (the
 *   capacity rule of mr_trace_level), and level l + 1 ran on the first queue_capacity of them.  The call cannot report this
 *   itself; the caller reads the counts, once, after the stream has run.  fan x samples always suffices for level 1, and
 *   fan^depth x samples for every level.
 * Workspace: two queues of queue_capacity rays; per queue, in this order, each array's offset rounded up to 16 bytes: 32 bytes
 *   per ray (mr_ray), 12 per ray (weight), 4 per ray (pixel), with MR_LEVEL_PATH 4 per ray (id), with MR_LEVEL_PATH and
 *   environment 1 per ray (low-res byte).  mr_render_recursion_workspace returns the total (0 for depth 0); it is host-only and
 *   reads nothing but the descriptor.  d_workspace must be 16-byte aligned and workspace_bytes at least that total.
 * The first call after mr_scene_set_textures / mr_scene_set_environment uploads (texture table, environment image), before the
 *   first launch; that call must lie outside a stream capture, as for mr_render_lights_environment.
 *
 * Errors.  MR_ERR_INVALID from the arguments alone, before the scene's state is read and before any device call:
 *   mr_render_level_lights' own list under this call's name (NULL scene / frame / d_rgb, empty image, spp, bands, rows, size,
 *   flags it does not know, misaligned d_rgb; MR_TRACE_ANY; environment > 1; with MR_LEVEL_PATH, path_kinds 0 or with unknown
 *   bits; more samples than 2^32 - 1); NULL desc or NULL d_level_counts (8-byte aligned); depth > 64; with depth >= 1: children
 *   that is neither MR_LEVEL_SPECULAR nor MR_LEVEL_PATH, queue_capacity 0, a NULL or misaligned workspace, workspace_bytes too
 *   small; non-zero reserved words.  MR_ERR_STATE: a scene that is unbuilt, built host_only, or has no lights.
 * Not part of this call: photon maps (mr_render_recursion_photons, miro_hip_recursion_photons.h, is this call with them), square lights, the thin lens (mr_render_recursion_lens,
 *   miro_hip_lens.h, is this call with it), more than one band range per call, and octant bytes for grouped traversal (group_octants).  The per-level calls serve those. */
typedef struct mr_recursion_desc {
    uint32_t depth;                 /* TRACE_DEPTH: levels 0..depth are run */
    uint32_t children;              /* MR_LEVEL_SPECULAR or MR_LEVEL_PATH (depth 0: ignored) */
    uint32_t environment;           /* as in mr_frame_level_desc */
    uint32_t path_kinds, path_seed; /* MR_LEVEL_PATH */
    uint32_t queue_capacity_lo, queue_capacity_hi;   /* rays per queue; two queues */
    uint32_t reserved[5];           /* must be 0 */
} mr_recursion_desc;

mr_status mr_render_recursion_workspace(const mr_recursion_desc *desc, uint64_t *bytes);   /* host only */
mr_status mr_render_recursion(mr_scene *scene, const mr_frame_desc *frame, const mr_recursion_desc *desc,
                              float *d_rgb, void *d_workspace, uint64_t workspace_bytes,
                              uint64_t *d_level_counts /* [depth+1][8] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRO_HIP_RECURSION_H */
#include "miro_hip_recursion_photons.h"
