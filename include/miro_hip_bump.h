/* miro_hip_bump.h -- reflective bump-mapped materials in the miro_hip C ABI: the reflect / Fresnel / refract generators about the
 * normal Scene::trace hands on.
 * miro_hip_passes.h includes this file below its declarations, so a caller includes miro_hip.h alone.
 * Why a ninth file: tests hold the lists of functions that the eight others declare at 69, 9, 3, 1, 2, 2, 3 and 4 names; the entry
 * point here is listed in miro_amd.binding.BUMP_SYMBOLS, which load_library() requires of the library in the same way.
 *
 * Scene::trace bumps the normal of every hit on a material with a UV texture (Scene.cpp:234-263; only StoneTexture's bumpHeight2D
 * is not 0) and everything after it reads that normal: Phong::shade, Ray::reflect (Ray.h:156: d - 2 dot(N, d) N), the Fresnel
 * term, Ray::refract, the photon walk.  mr_scene_set_textures accepts a material that names a MR_TEX_STONE texture and has a
 * non-zero ks (a polished stone floor) where that texture's descriptor says MR_TEX_REFLECTIVE in reserved[0], the one word of
 * mr_texture_desc.reserved that may be non-zero, and for a STONE texture only.  Without the flag such a table is MR_ERR_INVALID
 * as it always was: the flag is the caller's word that it renders the scene through the calls below, so a caller written
 * against the old rule is still told at set-up, not by a refusal in the middle of a frame.  A non-zero kt on such a material
 * stays MR_ERR_INVALID with or without it, because the light through a refractive occluder reads the occluder's N
 * (Phong.cpp:99-113) and no shadow loop bumps it.  A scene with such a material is
 * "bumped_specular"; on it, and on it alone,
 *   mr_gen_secondary_rays                        returns MR_ERR_STATE and names mr_gen_secondary_rays_surface,
 *   mr_gen_path_rays with MR_PATH_MIRROR         returns MR_ERR_STATE and names mr_gen_path_rays_surface,
 *   mr_trace_level_lights and the specular levels of mr_render_recursion[_lens | _photons | _passes]
 *                                                launch kernels whose children bounce about the bumped normal,
 * and every call that already took the normal of its own surface step (mr_render_level_lights and its lens and pass forms,
 * mr_trace_level_lights_path, mr_gen_path_rays_surface, mr_trace_photons_surface) is what it was.
 *
 * mr_gen_secondary_rays_surface is mr_gen_secondary_rays (miro_hip.h) with d_normal after d_hits: the buffer mr_hit_surface
 * writes, 3 n floats, 4-byte aligned, read for rays that have a child only (a listed ray has a hit; mr_hit_surface leaves the
 * rows of a miss untouched).  Every child -- Ray::reflect, the Fresnel term, Ray::refract -- takes hit.N from it; P is still
 * rebuilt from ray and hit, and WHICH children a hit has stays the material's.  Every other argument, the order of the children,
 * d_count and the capacity rule are mr_gen_secondary_rays'.  It looks nothing up and refuses no scene; on a scene without a
 * reflective STONE material, fed mr_hit_surface's buffer, the children are mr_gen_secondary_rays' bit for bit.
 * Errors: mr_gen_secondary_rays' own list in its order, then NULL or misaligned d_normal: MR_ERR_INVALID. */
#ifndef MIRO_HIP_BUMP_H
#define MIRO_HIP_BUMP_H
#ifdef __cplusplus
extern "C" {
#endif

#define MR_TEX_REFLECTIVE 1u   /* mr_texture_desc.reserved[0] of a MR_TEX_STONE texture: a material that names it may have ks != 0 */

mr_status mr_gen_secondary_rays_surface(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                                        const float *d_weights, const uint32_t *d_pixels, uint64_t n, uint32_t spp,
                                        mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels, uint64_t *d_count,
                                        uint64_t out_capacity, uint8_t *d_out_octants, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRO_HIP_BUMP_H */
