/* miro_hip_surface.h -- entry points of the miro_hip C ABI declared outside miro_hip.h.  miro_hip.h includes this file, so a
 * caller includes miro_hip.h alone.  Why a file of its own: tests/test_solid_textures.py holds the list of functions that
 * miro_hip.h itself declares at 69 names, and tests/test_abi.py holds miro_amd's EXPORTED_SYMBOLS to exactly that list; an
 * entry point added since is declared here and listed in miro_amd.binding.SURFACE_SYMBOLS, which load_library() requires of
 * the library in the same way.  Each call is documented in miro_hip.h next to the call it extends. */
#ifndef MIRO_HIP_SURFACE_H
#define MIRO_HIP_SURFACE_H
#ifdef __cplusplus
extern "C" {
#endif

/* mr_trace_photons on the walk that looks textures up: see "mr_trace_photons_surface" in miro_hip.h */
mr_status mr_trace_photons_surface(mr_scene *scene, mr_photon_map *map, const mr_photon_trace_desc *desc,
                                   mr_photon_trace_result *result, mr_photon_record *d_records, uint64_t records_capacity,
                                   void *stream);

/* the photon-map term of mr_final_gather for any queue of the recursion: see "mr_gather_level" in miro_hip.h.  d_scratch holds
 * 12 n floats and its layout is part of the contract: [0, 3n) the query positions, [3n, 6n) the query normals (NaN = no query),
 * [6n, 9n) the global map's estimate, [9n, 12n) the caustic map's; ray k's triple sits at 3k of each part (not compacted). */
mr_status mr_gather_level(mr_scene *scene, mr_photon_map *global_map, mr_photon_map *caustic_map, const mr_ray *d_rays,
                          const mr_hit *d_hits, const float *d_normal, const float *d_weights, const uint32_t *d_pixels, uint64_t n,
                          float max_dist, uint32_t nphotons, uint32_t spp, float *d_scratch, float *d_rgb, float *d_ray_rgb,
                          uint64_t *d_counts, void *stream);

/* The photon map built on the device: see "mr_photon_map_build_device" in miro_hip.h.  store(n records) +
 * scale_photon_power(scale) + balance() for an EMPTY, unbalanced map, from a device array of records (pos, dir and power are
 * read, the other fields ignored), in the order given.  On return the map is balanced and resident, and answers every call as
 * the map that the same records took through mr_photon_map_store / _scale / _balance; mr_photon_map_export reads the device
 * arrays back.  The host reads O(1) data (counts, the box) and the list of deferred photons: those whose scaled angle
 * acos(dz) * 256 / pi or atan2(dy, dx) * 256 / (2 pi) is not finite or lies within 2^-20 of a whole number get their two
 * direction bytes from the host's own expression.  n is at most 2^24 (larger maps: the host path).
 * Errors: NULL map, NULL records with n > 0, records not 4-byte aligned, n > 2^24, a non-finite position (found on the device;
 * the map stays empty and usable): MR_ERR_INVALID.  A map that holds photons or is balanced: MR_ERR_STATE. */
typedef struct mr_photon_build_result {
    uint64_t stored;     /* photons in the map */
    uint64_t dropped;    /* records beyond max_photons (PhotonMap.cpp:260-261) */
    uint64_t deferred;   /* photons whose direction bytes the host decided */
    double store_ms, balance_ms, pack_ms;   /* wall time of the three stages, stream synchronised between them */
} mr_photon_build_result;
mr_status mr_photon_map_build_device(mr_photon_map *map, const mr_photon_record *d_records, uint64_t n, float scale,
                                     mr_photon_build_result *result, void *stream);

/* mr_trace_photons (surface == 0) or mr_trace_photons_surface (surface == 1) whose records never leave the device: see
 * "mr_trace_photons_resident" in miro_hip.h.  Rounds, termination, result, d_records and errors are those calls'; the records
 * are appended to a library-owned device buffer and the call ends with mr_photon_map_build_device(map, records, stored,
 * 1 / emitted) into `build` (may be NULL): the map is balanced and resident on return.  ONE map per call: the map must be
 * empty (MR_ERR_STATE otherwise); several lights traced into one map stay with mr_trace_photons + mr_photon_map_balance. */
mr_status mr_trace_photons_resident(mr_scene *scene, mr_photon_map *map, const mr_photon_trace_desc *desc, uint32_t surface,
                                    mr_photon_trace_result *result, mr_photon_build_result *build,
                                    mr_photon_record *d_records, uint64_t records_capacity, void *stream);

/* mr_shade_square_lights with the hit's diffuse colour and normal read from mr_hit_surface's buffers, for a scene with a texture
 * table (any scene will do): see "mr_shade_square_lights_surface" in miro_hip.h.  d_color / d_normal: 3 n floats each, 4-byte
 * aligned, read for rays with a hit only. */
mr_status mr_shade_square_lights_surface(mr_scene *scene, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t samples,
                                         uint32_t seed, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                         const float *d_normal, const float *d_weights, const uint32_t *d_pixels,
                                         const float *d_uv_in, uint64_t n, uint32_t spp, uint32_t flags, float *d_rgb,
                                         float *d_ray_rgb, uint64_t *d_counts, void *stream);

/* mr_gen_path_rays with every hit's normal and the diffuse child's colour read from mr_hit_surface's buffers, for a scene with a
 * texture table (any scene will do): see "mr_gen_path_rays_surface" in miro_hip.h.  d_color / d_normal: 3 n floats each, 4-byte
 * aligned, read for rays with a hit only. */
mr_status mr_gen_path_rays_surface(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                   const float *d_normal, const float *d_weights, const uint32_t *d_pixels, const uint32_t *d_ids,
                                   uint64_t n, uint32_t spp, uint32_t seed, uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays,
                                   float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids, uint64_t *d_count,
                                   uint64_t out_capacity, uint8_t *d_out_octants, void *stream);

/* Where the calling thread's last mr_bvh_build spent its wall time, in milliseconds (thread-local; any pointer may be NULL): see
 * mr_build_opts.builder in miro_hip.h.  builder_used: the builder that really produced the tree -- MR_BUILD_REFERENCE for a
 * scene that MR_BUILD_REFERENCE_DEVICE handed to the host because of a non-finite coordinate.
 *   prims_ms   device builder: upload of the raw mesh arrays and the object-table kernel (0 for the host builder)
 *   levels_ms  device builder: the launches of the tree's depths with their read-backs; host builder: the whole recursion
 *   finish_ms  device builder: subtree sizes, pre-order numbering and the download of the tree (0 for the host builder)
 *   upload_ms  either: flattening the tree into the device layout and uploading it (0 with host_only) */
mr_status mr_bvh_build_timing(uint32_t *builder_used, double *prims_ms, double *levels_ms, double *finish_ms, double *upload_ms);

/* ---- the whole direct-light frame step over the scene's LIGHT LIST in ONE launch ----------------------------------------
 * mr_render_direct's frame with Phong::shade's loop over Scene::lights() (Phong.cpp:59-63) in the place of its one point
 * light: for every sample Camera::eyeRay -> Scene::trace -> for every light of mr_scene_set_lights, in list order, the shadow
 * ray, Scene::trace, the occluder's light scale and the light's terms added to L (from 0; a miss contributes 0) -> the pixel's
 * mean.  The same hit records, per-sample L and pixels, bit for bit, as the batched
 *   mr_gen_eye_rays[_tiled] -> mr_trace -> mr_shade_lights(d_ray_rgb) [-> pairwise mean over each pixel's samples]
 * on the same scene, camera, seed and sample order, without the ray, hit and per-ray colour buffers (60 bytes per sample).
 * Window: mr_render_direct's in every respect -- rows [y0,y1) or one rank's interleaved bands, spp a power of two <= 64,
 *   jitter, seed, tiled.  frame->light and frame->diffuse are NOT read.
 * Lights: the scene's list (point and disc lights, at most MR_MAX_LIGHTS).  Materials: the table of mr_scene_set_materials,
 *   or the white Lambert without one -- what mr_shade_lights uses.
 * d_rgb: rows*W*3 floats, window rows in band order, image order inside a row.  Optional device outputs (NULL to skip):
 *   d_hits        rows*W*spp records in sample order (the tiled order with frame->tiled), 16-byte aligned
 *   d_sample_rgb  3 floats per sample in d_hits' order: the sample's un-weighted L (0 for a miss)
 *   d_counts      [0] += samples, [1] += shadow rays = samples with a hit x lights (8-byte aligned, not zeroed by the call)
 * flags: MR_MATH_PRODUCT, MR_TRACE_INCOHERENT (both kinds of ray), MR_TRACE_ANY (shadow rays only).
 * Launches: with device buffers the call enqueues ONE kernel on `stream` and can be captured into a graph; it allocates
 *   nothing and uses none of the scene's hand-out counters or eye-relative tables, so calls on one scene may overlap freely.
 * Errors, in this order.  MR_ERR_INVALID, before any device call and before the scene's state is read: NULL scene / frame /
 *   d_rgb; W or H of 0; spp not a power of two <= 64; a bad band description; rows outside the image; window too large; any
 *   other flag, MR_FRAME_NO_SHADOWS included; d_hits not 16-byte aligned (d_counts 8, the float buffers 4).  MR_ERR_STATE: a
 *   scene that is not built or was built host_only; a scene without lights; a scene with a texture table (use mr_trace ->
 *   mr_shade_lights, or mr_hit_surface -> mr_shade_lights_surface); MR_TRACE_ANY with a refractive material.  An empty window
 *   (y0 == y1, or a rank without bands) is MR_OK with no launch. */
mr_status mr_render_lights(mr_scene *scene, const mr_frame_desc *frame, float *d_rgb, mr_hit *d_hits, float *d_sample_rgb,
                           uint64_t *d_counts, void *stream);

/* ---- ... on ANY scene, textured ones included -------------------------------------------------------------------------
 * mr_render_lights with the surface pass's step between the primary trace and the light loop: with a texture table
 * (mr_scene_set_textures) every hit's diffuseColor (Phong.cpp:51-56, all seven kinds in any mixture) and the normal Scene::trace
 * hands on (bump-mapped on a STONE material, normalised; Scene.cpp:234-263) are what mr_hit_surface computes for that ray and
 * hit; the colour goes where the material's diffuse went, the normal everywhere N goes; the occluder's light scale still reads
 * the occluder's own geometric normal.  The same hit records, per-sample colour, normal and L and pixels, bit for bit, as the batched
 *   mr_gen_eye_rays[_tiled] -> mr_trace -> mr_hit_surface -> mr_shade_lights_surface(d_ray_rgb) [-> pairwise mean over each
 *   pixel's samples]
 * on the same scene, camera, seed and sample order, without its ray, hit, colour, normal and per-ray L buffers (84 bytes per
 * sample).  Without a texture table the call renders what mr_render_lights renders, bit for bit.
 * Window, lights, materials, flags, d_rgb, d_hits, d_sample_rgb: mr_render_lights' in every respect.  Besides (NULL to skip):
 *   d_sample_color   3 floats per sample in d_hits' order, 4-byte aligned: what mr_hit_surface writes to d_color for that ray
 *   d_sample_normal  likewise, its d_normal.  A sample that missed leaves its row of both untouched, as there.
 *   d_counts         THREE words: [0] += samples, [1] += shadow rays, [2] += hits whose lookup the reference leaves undefined
 *                    (mr_hit_surface's d_counts[0] on the same batch); 8-byte aligned, not zeroed by the call
 * A sample that misses contributes 0, as in mr_render_lights: the environment of mr_scene_set_environment is NOT applied
 *   (mr_render_lights_environment, declared in miro_hip_frame.h, is this call with it applied).
 * Launches: with a texture table that is already on the device the call enqueues ONE kernel on `stream` and can be captured
 *   into a graph.  The first call after mr_scene_set_textures uploads the table on `stream` -- an allocation and a copy -- and
 *   must lie outside a capture (every other call that reads the table uploads it too).
 * Errors: mr_render_lights', in its order, without the refusal of a texture table; d_sample_color / d_sample_normal not 4-byte
 *   aligned is MR_ERR_INVALID with the other alignments.  MR_TRACE_ANY with a refractive material and a scene without lights
 *   stay MR_ERR_STATE. */
mr_status mr_render_lights_surface(mr_scene *scene, const mr_frame_desc *frame, float *d_rgb, mr_hit *d_hits, float *d_sample_rgb,
                                   float *d_sample_color, float *d_sample_normal, uint64_t *d_counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRO_HIP_SURFACE_H */
