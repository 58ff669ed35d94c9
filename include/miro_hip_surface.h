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

#ifdef __cplusplus
}
#endif
#endif /* MIRO_HIP_SURFACE_H */
