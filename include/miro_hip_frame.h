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

/* ---- ONE level of Scene::traceScene's recursion in ONE launch on any scene: light list, texture table, environment ----------
 * mr_trace_level (miro_hip.h) shades a queue by one point light with the plain material table.  This call takes the same queue
 * -- d_rays, optional d_weights (NULL: 1) and d_pixels (NULL: ray index / spp), n rays -- and handles ray k in one lane:
 *   1. Scene::trace, closest hit; d_hits[k], if given, is that record.
 *   2. A miss: L = Scene::getEnvironmentMap(ray) of mr_scene_set_environment with environment == 1 -- bg_color, or the lookup of
 *      the FULL-RESOLUTION image at the ray's direction (a specular child is never isDiffuse) -- otherwise 0.  A lookup the
 *      reference leaves undefined is 0 and counted.
 *   3. A hit: the per-hit step of mr_hit_surface with the scene's texture table or none (all seven texture kinds, the bumped
 *      normal on stone); rows k of d_color / d_normal, if given, receive it.  A miss leaves its rows untouched.
 *   4. A hit: for every light of mr_scene_set_lights in list order the shadow ray, its closest-hit trace, the light scale and the
 *      point or disc terms, summed into L -- mr_shade_lights_surface's loop.
 *   5. d_ray_rgb[k] = L, if given; weight * L / spp is added to d_rgb[pixel]: one add per ray, hit or miss (float atomics; rays
 *      of one pixel in adjacent lanes are summed in the wave first).  d_rgb may be NULL when d_ray_rgb is given.
 *   6. With children == MR_LEVEL_SPECULAR the reflect / Fresnel / refract children of mr_gen_secondary_rays go to the output
 *      queue: about the normal and with the material that generator uses, not the bumped normal.  Capacity rule, d_out_count
 *      (zeroed by the call, then += children, stored or not) and d_out_octants are mr_trace_level's.
 * d_counts: FIVE words, 8-byte aligned, not zeroed by the call: [0] += rays, [1] += shadow rays (hits x lights), [2] +=
 *   undefined texture lookups, [3] += misses, [4] += undefined environment lookups.
 * flags: MR_MATH_PRODUCT, MR_TRACE_INCOHERENT only.  n == 0 is MR_OK and launches nothing, after zeroing d_out_count on a level
 *   with children.
 * The first call after mr_scene_set_textures or mr_scene_set_environment uploads (mr_render_lights_environment's rule) and must
 *   lie outside a stream capture; after that the call is the zeroing of d_out_count (with children; a one-word kernel, so that a
 *   graph replays it as written) plus one kernel and can be captured.
 *
 * The contract.  Per ray, the outputs are those of the batched
 *   mr_trace -> mr_hit_surface -> mr_shade_lights_surface(d_ray_rgb) || mr_shade_environment(flags 0, d_ray_rgb)
 *   -> mr_gen_secondary_rays
 * on the same queue, bit for bit: hit records, colour, normal, L (the light chain's row where the ray hit, the environment
 * chain's where it missed), the counters; the children are the same set in another order; d_rgb differs by the order of the
 * float atomics.
 * Errors.  MR_ERR_INVALID from the arguments alone, before the scene's state is read and before any device call: NULL scene /
 *   level / d_rays; d_rgb and d_ray_rgb both NULL; spp == 0; other flags; children == MR_LEVEL_PATH (the path-traced generators
 *   stay batched: mr_gen_path_rays[_surface]); non-zero reserved words; children without an output queue or capacity;
 *   misalignment (rays and out rays 16 bytes, counters 8, float and index buffers 4).  MR_ERR_STATE: a scene that is unbuilt,
 *   built host_only, or has no lights.  Square lights and the thin lens are not part of this call. */
typedef struct mr_level_lights_desc {
    uint32_t spp, flags, children;       /* children: MR_LEVEL_LAST or MR_LEVEL_SPECULAR */
    uint32_t environment;                /* 0: a miss is worth 0.  1: Scene::getEnvironmentMap of mr_scene_set_environment */
    uint32_t out_capacity_lo, out_capacity_hi;
    uint32_t reserved[6];                /* must be 0 */
    uint8_t *d_out_octants;              /* may be NULL, as in mr_level_desc */
} mr_level_lights_desc;
mr_status mr_trace_level_lights(mr_scene *scene, const mr_level_lights_desc *level, const mr_ray *d_rays,
                                const float *d_weights, const uint32_t *d_pixels, uint64_t n, float *d_rgb,
                                mr_hit *d_hits, float *d_ray_rgb, float *d_color, float *d_normal,
                                mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                                uint64_t *d_out_count, uint64_t *d_counts, void *stream);

/* ---- ... of a PATH_TRACING build: the same level with the path tracer's children and the low-res environment image ----------
 * mr_trace_level_lights stops at the specular children.  This call takes its queue plus what the path tracer's queues carry --
 * d_ids, stable ray ids (NULL: the ray's index, as in mr_gen_path_rays), and one byte per ray that says whether Ray::random made
 * it (level->d_lowres, optional) -- and handles ray k in one lane:
 *   1. Scene::trace, closest hit; d_hits[k], if given, is that record.
 *   2. A miss: L = Scene::getEnvironmentMap(ray) with environment == 1 -- bg_color, or LoadedTexture::lookup of the image at the
 *      ray's direction: the FULL-RESOLUTION image, or lowresLookup2D of its low-res copy for a ray that is isDiffuse
 *      (Scene.cpp:678-681): d_lowres[k] != 0, or every ray of the queue with MR_ENV_LOWRES -- otherwise 0.  A lookup the
 *      reference leaves undefined is 0 and counted, in either image.
 *   3. - 5. as in mr_trace_level_lights: the surface step (rows k of d_color / d_normal, if given), the loop over the light list,
 *      d_ray_rgb[k] = L, weight * L / spp added to d_rgb[pixel].
 *   6. With children == MR_LEVEL_PATH the children of mr_gen_path_rays_surface go to the output queue: of the kinds in path_kinds
 *      (MR_PATH_MIRROR | MR_PATH_REFRACT | MR_PATH_DIFFUSE) that the hit's MATERIAL has, lobe-sampled with the random numbers of
 *      (seed, ray id, bounce, kind), every one about the normal of step 3 -- the bumped one on stone -- and the diffuse child with
 *      weight x the looked-up colour of step 3.  d_out_ids (optional) receives the child ids mr_gen_path_rays derives;
 *      d_out_lowres (optional), one byte per STORED child, is 1 for the child of Ray::random and 0 otherwise: the next level's
 *      d_lowres.  Capacity rule (a child whose slot lies beyond out_capacity is counted, not stored: none of its outputs is
 *      written), d_out_count (zeroed by the call, then += children, stored or not) and d_out_octants are mr_trace_level's.
 * d_counts: FIVE words as in mr_trace_level_lights: [0] += rays, [1] += shadow rays, [2] += undefined texture lookups,
 *   [3] += misses, [4] += undefined environment lookups.
 * flags: MR_MATH_PRODUCT, MR_TRACE_INCOHERENT, MR_ENV_LOWRES only.  n == 0 is MR_OK and launches nothing, after zeroing
 *   d_out_count on a level with children.
 * Uploads and graph capture: mr_trace_level_lights' rule -- after the first call the call is the zeroing of d_out_count (with
 *   children; a one-word kernel) plus one kernel.
 *
 * The contract.  Per ray, on the same queue, seed, bounce and kinds, the outputs are those of the batched
 *   mr_trace -> mr_hit_surface -> mr_shade_lights_surface(d_ray_rgb) || mr_shade_environment(d_ray_rgb, the same flags and
 *   d_lowres) -> mr_gen_path_rays_surface(that chain's colour and normal)
 * bit for bit: hit records, colour, normal, L (the light chain's row where the ray hit, the environment chain's where it
 * missed), the five counters; the children are the same set -- ray, weight, pixel, id and octant of every child id -- in another
 * order, d_out_count is equal; d_rgb differs by the order of the float atomics.  On a scene without a texture table and with
 * path_kinds = MR_PATH_MIRROR | MR_PATH_REFRACT the children are mr_gen_path_rays' set.
 * Errors.  MR_ERR_INVALID from the arguments alone, before the scene's state is read and before any device call: NULL scene /
 *   level / d_rays; d_rgb and d_ray_rgb both NULL; spp == 0; other flags; children == MR_LEVEL_SPECULAR (those are
 *   mr_trace_level_lights') or unknown; environment > 1; with children, path_kinds 0 or with unknown bits; non-zero reserved
 *   words; children without an output queue or capacity; misalignment (rays and out rays 16 bytes, counters 8, float, index and
 *   id buffers 4; the byte masks and octants may lie anywhere).  MR_ERR_STATE: a scene that is unbuilt, built host_only, or has
 *   no lights.  Square lights and the thin lens are not part of this call. */
typedef struct mr_level_lights_path_desc {
    uint32_t spp, flags, children;       /* children: MR_LEVEL_LAST or MR_LEVEL_PATH */
    uint32_t environment;                /* 0: a miss is worth 0.  1: Scene::getEnvironmentMap of mr_scene_set_environment */
    uint32_t path_kinds, seed, bounce;   /* as in mr_gen_path_rays; read with children == MR_LEVEL_PATH */
    uint32_t out_capacity_lo, out_capacity_hi;
    uint32_t reserved[5];                /* must be 0 */
    uint8_t *d_out_octants;              /* may be NULL, as in mr_level_desc */
    const uint8_t *d_lowres;             /* may be NULL: per ray, non-zero = the ray is isDiffuse */
    uint8_t *d_out_lowres;               /* may be NULL: per stored child, 1 = made by Ray::random */
} mr_level_lights_path_desc;
mr_status mr_trace_level_lights_path(mr_scene *scene, const mr_level_lights_path_desc *level, const mr_ray *d_rays,
                                     const float *d_weights, const uint32_t *d_pixels, const uint32_t *d_ids, uint64_t n,
                                     float *d_rgb, mr_hit *d_hits, float *d_ray_rgb, float *d_color, float *d_normal,
                                     mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids,
                                     uint64_t *d_out_count, uint64_t *d_counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRO_HIP_FRAME_H */
