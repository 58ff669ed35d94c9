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

#ifdef __cplusplus
}
#endif
#endif /* MIRO_HIP_SURFACE_H */
