/*
 * miro_hip.h -- C ABI of the MI355X-native intersection path for the Miro ray tracer
 * (hallgeirl/cse168-raytracer).  Plain C, plain pointers and sizes; no C++ or torch types.
 *
 * The reference has no FFI layer: its hot path is the C++ surface
 *     bool Scene::trace(HitInfo&, const Ray&, float tMin, float tMax) const   Scene.h:38-39, Scene.cpp:214-268
 *     void BVH::build(Objects*, int depth)                                    BVH.h:33,      BVH.cpp:60-339
 *     bool BVH::intersect(HitInfo&, const Ray&, float tMin, float tMax) const BVH.h:35-36,   BVH.cpp:438-469
 * called from Scene.cpp:72 (build), :217/:278/:539 and Phong.cpp:97 (trace).  The entry points
 * below are what a binding for that surface binds: scene assembly (Scene::addObject,
 * TriangleMesh::load), BVH::build, and a *batched* Scene::trace (a single-ray call is a
 * batch of one).  cse168-raytracer_amd/host/miro_shim.hpp re-creates the C++ signatures on top
 * of these functions; INTEGRATION.md shows the reference-side glue.
 *
 * All functions return MR_OK (0) or a negative mr_status; mr_last_error() gives a
 * thread-local message.  No exception crosses this boundary.  There is NO CPU fallback:
 * without a HIP device every device-touching call fails with MR_ERR_HIP.
 */
#ifndef MIRO_HIP_H
#define MIRO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t mr_status;
enum {
    MR_OK          =  0,
    MR_ERR_INVALID = -1,   /* bad argument */
    MR_ERR_IO      = -2,   /* file could not be opened (TriangleMesh::load returns false, TriangleMeshLoad.cpp:66-71) */
    MR_ERR_NOMEM   = -3,
    MR_ERR_HIP     = -4,   /* HIP runtime error or no device */
    MR_ERR_STATE   = -5    /* call out of order (trace before build, add after build) */
};

/* Ray (Ray.h:40-84): origin, direction and the [tMin,tMax] interval that Scene::trace
 * takes as separate arguments.  32 bytes, two float4 loads per lane on the device. */
typedef struct mr_ray { float ox, oy, oz, tmin, dx, dy, dz, tmax; } mr_ray;

/* HitInfo (Ray.h:21-38) in its minimal device form.  prim indexes triangles in
 * Scene::addObject order (= concatenated mesh order); beta/gamma are the locals of
 * Triangle.cpp:155-156.  On a miss prim == MR_MISS, t == tmax (BVH.cpp:444), beta=gamma=0.
 * P, N, material, object are rebuilt by the shim (Triangle.cpp:160-166). 16 bytes. */
typedef struct mr_hit { float t; uint32_t prim; float beta, gamma; } mr_hit;
#define MR_MISS 0xFFFFFFFFu
/* A hit on an unbounded object (a Plane, kept in Scene::m_unboundedObjects, Scene.h:22-23) reports
 * prim = MR_PLANE_BIT | its index in that list; spheres are bounded objects and use ordinary indices.
 * beta = gamma = 0 for both; P = o + t*d (Sphere.cpp:61, Plane.cpp:42). */
#define MR_PLANE_BIT 0x80000000u

/* Indexed triangle mesh as TriangleMesh stores it (TriangleMesh.h:27-67). */
typedef struct mr_mesh_desc {
    const float    *vertices;  uint32_t n_vertices;   /* xyz triples */
    const float    *normals;   uint32_t n_normals;    /* xyz triples */
    const uint32_t *vidx;                             /* 3 per triangle */
    const uint32_t *nidx;                             /* 3 per triangle */
    uint32_t        n_triangles;
} mr_mesh_desc;

typedef struct mr_build_opts {
    uint32_t leaf_size;     /* OBJECTS_PER_LEAF (BVH.h:59,61): 4 = scalar reference build (default when 0) */
    uint32_t builder;       /* MR_BUILD_REFERENCE (0): the reference's binary-search split, identical tree, built on the host.
                               MR_BUILD_REFERENCE_DEVICE (1): the identical tree -- nodes, padded corners, child links, depths and
                               leaf order bit for bit -- built by kernels (csrc/mr_bvh_build.hip), one launch per depth.  It needs a
                               device: with host_only = 1 the call fails with MR_ERR_INVALID (before any device call; the message
                               names host_only).  A scene with a non-finite coordinate is built on the host instead (MR_OK);
                               "mr_bvh_build_timing" (declared in miro_hip_surface.h) tells which builder produced the tree and
                               where the calling thread's last mr_bvh_build spent its wall time.  Any other value: MR_ERR_INVALID,
                               "unknown builder" */
    uint32_t host_only;     /* 1: build the tree on the host and skip the device upload (tree inspection,
                               CPU-only tooling); mr_trace on such a scene fails with MR_ERR_STATE */
    uint32_t layout;        /* storage order of the device records (MR_LAYOUT_*): a permutation of where the same nodes and
                               triangles live in HBM -- references, visiting order and hit records are unaffected */
    uint32_t reserved[4];
} mr_build_opts;
enum { MR_BUILD_REFERENCE = 0, MR_BUILD_REFERENCE_DEVICE = 1 };
enum {
    MR_LAYOUT_DFS      = 0,   /* inner nodes in depth-first pre-order (a node's first inner child is its neighbour) */
    MR_LAYOUT_PAIRS    = 1,   /* pre-order, padded so that a node and its first inner child always share one 128-byte line */
    MR_LAYOUT_TREELETS = 2,   /* the top 12 levels breadth-first, below them treelets of three levels stored contiguously */
    MR_LAYOUT_ALIGN_LEAVES = 16 /* OR-ed in: dummy triangle records in front of a leaf whenever that lets its triangles touch
                                   fewer 128-byte lines */
};

typedef struct mr_scene_info {
    uint32_t n_vertices, n_normals, n_triangles;
    uint32_t n_nodes, n_leaves, max_depth;            /* Stats::BVH_Nodes / BVH_LeafNodes (BVH.cpp:64,88) */
    uint32_t leaf_size, built;
    uint64_t device_bytes;                            /* node + triangle + index arrays resident in HBM */
    int32_t  device;
    uint32_t reserved[3];
} mr_scene_info;

typedef struct mr_camera {                            /* Camera.h:53-60 */
    float eye[3], lookat[3], up[3], fov_deg;
} mr_camera;

/* mr_trace flags */
enum {
    MR_TRACE_CLOSEST  = 0u,        /* Scene::trace semantics (closest hit, strict-less replacement) */
    MR_TRACE_ANY      = 1u << 0,   /* stop at the first accepted hit; legal for shadow batches only when the
                                      scene has no refractive material (Phong.cpp:99-113) */
    MR_RAYS_ON_DEVICE = 1u << 1,   /* rays is a device pointer */
    MR_HITS_ON_DEVICE = 1u << 2,   /* hits is a device pointer */
    MR_MATH_FAST      = 1u << 3,   /* fused multiply-add + v_rcp_f32: same primitive, t within 1e-5 relative of the
                                      reference, beta/gamma only within the formula's own rounding sensitivity
                                      (~|o-A|/|edge| ulps).  The default is the bit-exact IEEE expression tree
                                      of Triangle.cpp:150-156 and is what parity and the bench are quoted on */
    MR_COUNT_STATS    = 1u << 4,   /* accumulate -DSTATS counters (BVH.cpp:461,496,632,643) */
    MR_TRACE_PERSISTENT = 1u << 5, /* incoherent batches: resident waves pull rays from a counter and re-arm idle
                                      lanes by wave64 ballot + prefix sum.  Same arithmetic and hit records as the
                                      one-shot kernel (exact quotients, or products with MR_MATH_PRODUCT); on par with
                                      it on random rays, slower on coherent camera rays -- off by default;
                                      triangle scenes only: ignored, i.e. the default kernel runs, when the scene holds
                                      spheres or planes, and under MR_COUNT_STATS / MR_MATH_FAST) */
    MR_TRACE_INCOHERENT = 1u << 7, /* batch hint: the 64 rays of a wave do not share their path through the tree (secondary,
                                      random or 1-sample-per-pixel batches).  Selects the voting control flow: every
                                      iteration a wave runs the step (node test / triangle test) most of its lanes need,
                                      instead of running node tests until its slowest lane has found a leaf.  Same per-ray
                                      steps in the same order: identical hit records.  Combines with MR_TRACE_PERSISTENT.
                                      Without the hint the default kernel decides per wave: a wave whose rays point into
                                      several octants votes, one whose rays share an octant does not */
    MR_FRAME_NO_SHADOWS = 1u << 8, /* mr_render_direct only: the reference's -DDISABLE_SHADOWS build (Phong.cpp:91) -- no shadow ray
                                      is built or traced, every light reaches every hit (BASELINE config 2, "primary rays
                                      only"); default traversal only */
    MR_MATH_PRODUCT   = 1u << 6    /* slab distances as products (corner - o) * RN(1/d) instead of the reference's
                                      quotients (corner - o) / d (BVH.cpp:601-602), whose decisions the default reproduces
                                      exactly (products where the visit's comparisons are more than 16 ulp from a tie --
                                      provably the quotients' outcome --, one fma correction step per product otherwise:
                                      exactly the correctly rounded quotient for operands in the normal range; literal
                                      divisions for the rest).  A product differs
                                      from the quotient by <= 3 ulp, which can flip a box comparison only on a
                                      near-tie (observed: 0 of 3e8 rays in normal use, 2 of 1.3e8 when tMax is set one ulp
                                      above a known hit); t / beta / gamma of a hit are the same bits either way.
                                      About 25 % faster */
};

typedef struct mr_scene mr_scene;

/* ---- scene assembly: Scene::addObject / TriangleMesh::load / createSingleTriangle -------------- */
/* A scene lives on one device; every call that touches it makes that device the calling thread's current HIP
 * device (hipSetDevice) and leaves it so -- the intended deployment is one process (or thread) per GPU. */
mr_status mr_scene_create(int32_t device, mr_scene **out);
mr_status mr_scene_destroy(mr_scene *scene);
/* copies the arrays; triangles are appended in order (assignment2.cpp:449-461) */
mr_status mr_scene_add_mesh(mr_scene *scene, const mr_mesh_desc *mesh);
/* TriangleMesh::load(file, ctm) (TriangleMeshLoad.cpp:63-311); ctm = 16 floats row-major or NULL.  `vt` records and the
 * texture indices of v/t and v/t/n face corners are kept (see mr_scene_set_texcoords). */
mr_status mr_scene_add_obj(mr_scene *scene, const char *path, const float *ctm16, uint32_t *n_triangles_out);
/* TriangleMesh::createSingleTriangle + setV1..3/setN1..3 (TriangleMeshLoad.cpp:15-56) */
mr_status mr_scene_add_triangle(mr_scene *scene, const float v[9], const float n[9]);
/* Sphere + setCenter/setRadius + Scene::addObject (Sphere.h:13-21, Sphere.cpp:28-69): the next bounded object;
 * *prim_out (may be NULL) receives its object index, which mr_hit.prim and prim_material use. */
mr_status mr_scene_add_sphere(mr_scene *scene, const float center[3], float radius, uint32_t *prim_out);
/* Plane + setNormal/setOrigin + Scene::addObject (Plane.h:22-27, Plane.cpp:33-48): the next unbounded object,
 * scanned after the BVH by every trace (Scene.cpp:220-230).  `material` indexes mr_scene_set_materials' table;
 * *index_out (may be NULL) receives the plane's index. */
mr_status mr_scene_add_plane(mr_scene *scene, const float normal[3], const float origin[3], uint32_t material,
                             uint32_t *index_out);

/* ---- BVH::build (BVH.cpp:60-339) via Scene::preCalc (Scene.cpp:50-84); uploads the scene ------- */
mr_status mr_bvh_build(mr_scene *scene, const mr_build_opts *opts);

mr_status mr_scene_get_info(const mr_scene *scene, mr_scene_info *info);
/* host copies of the merged mesh (for the shim's P/N/material reconstruction) */
mr_status mr_scene_get_mesh(const mr_scene *scene, mr_mesh_desc *out);
/* tree in DFS pre-order: corners6[n_nodes*6], meta3[n_nodes*3] = (is_leaf, child0|first, child1|count),
 * leaf_prims[n_triangles].  Any pointer may be NULL. */
mr_status mr_scene_export_tree(const mr_scene *scene, float *corners6, int32_t *meta3, uint32_t *leaf_prims);

/* ---- Scene::trace, batched (Scene.cpp:214-268 -> BVH.cpp:438-658 -> Triangle.cpp:136-169) ------- */
/* stream: a hipStream_t (NULL = default stream).  Host buffers are staged and the call returns when the hits are
 * in `hits`; batches above 2^20 rays are cut into chunks whose upload, trace and download overlap (fully so when the
 * buffers are pinned, see mr_host_alloc; pageable memory is staged by the HIP runtime on the calling thread).
 * With both buffers on the device the call only enqueues work on `stream`.
 * Threads: a built scene is immutable and mr_trace / mr_trace_indirect may be called on it from several host
 * threads at once, like the reference's const Scene::trace from its OpenMP workers (Scene.cpp:112-115); calls
 * with host buffers take turns on the scene's staging buffers.  mr_shade_direct and mr_shade_accumulate keep
 * per-scene scratch (occlusion flags, light scale): one such call in flight per scene. */
mr_status mr_trace(mr_scene *scene, const mr_ray *rays, uint64_t n_rays, mr_hit *hits,
                   uint32_t flags, void *stream);
/* Page-locked host memory for ray / hit buffers handed to mr_trace (the reference's callers keep Ray and HitInfo in
 * ordinary `new`-ed memory, Scene.cpp:117-140; pinned buffers let the copies run at PCIe speed and overlap the trace).
 * Usable from any device; free with mr_host_free (NULL is a no-op). */
mr_status mr_host_alloc(void **ptr, uint64_t bytes);
mr_status mr_host_free(void *ptr);
/* Same, for a batch whose size was produced on the device (the compacted shadow batch of
 * mr_gen_shadow_rays): traces min(*d_count, max_rays) rays without a host round trip.  All pointers are
 * device pointers; MR_RAYS_ON_DEVICE / MR_HITS_ON_DEVICE are implied. */
mr_status mr_trace_indirect(mr_scene *scene, const mr_ray *d_rays, const uint64_t *d_count, uint64_t max_rays,
                            mr_hit *d_hits, uint32_t flags, void *stream);
/* The same trace for a BOUNCE QUEUE (device buffers): a generator writes children in the order of their parents, so the
 * rays of a wave start at neighbouring surface points but point into all eight octants.  This call first writes into
 * d_order (n uint32) the ray indices grouped by direction octant inside consecutive chunks of 2^chunk_log2 rays (8 ... 14;
 * 0 = 14; a stable counting sort -- no ray is moved), then traces ray d_order[k] in lane k and stores its hit at
 * d_hits[d_order[k]]: the hit buffer is byte for byte that of mr_trace on the same rays; whole waves share a direction
 * sign (the octant-specialised loops apply) and rays that leave the scene at once stop holding waves.  Measured on the
 * stand-in atrium's diffuse-bounce queue: 5.2 -> 6.0 Grays/s; on the bunny's: 22 -> 31 (profiles/r03_octant_order.log).
 * flags: MR_TRACE_ANY, MR_MATH_PRODUCT, MR_TRACE_INCOHERENT.
 * d_octants (may be NULL): one byte per ray holding the sign bits of its direction (x<0 | y<0 << 1 | z<0 << 2), as the
 * generators write them (d_out_octants of mr_gen_secondary_rays / mr_gen_path_rays / mr_level_desc); the order is then made
 * from 1 byte per ray instead of the 32-byte rays -- the order kernel is bandwidth-bound, this is what it costs.  The bytes are
 * trusted to be the rays' octants: other values change the grouping, never the hit buffer.
 * chunk_log2 | MR_ORDER_GIVEN: d_order is an INPUT -- a permutation of 0 ... n-1 the caller made (mr_order_by_octant, or the
 * one an earlier call on the same rays left there); it is not checked, an index >= n reads and writes out of bounds.
 * mr_order_by_octant is the first half alone (d_rays may be NULL when d_octants is given): for mr_level_desc.d_order. */
#define MR_ORDER_GIVEN 0x80000000u
mr_status mr_order_by_octant(mr_scene *scene, const mr_ray *d_rays, const uint8_t *d_octants, uint64_t n, uint32_t chunk_log2,
                             uint32_t *d_order, void *stream);
mr_status mr_trace_grouped(mr_scene *scene, const mr_ray *d_rays, const uint8_t *d_octants, uint64_t n, mr_hit *d_hits,
                           uint32_t *d_order, uint32_t chunk_log2, uint32_t flags, void *stream);
/* -DSTATS counters accumulated by MR_COUNT_STATS traces (synchronises the device) */
mr_status mr_trace_get_stats(mr_scene *scene, uint64_t *box_tests, uint64_t *tri_tests, int32_t reset);

/* ---- callers of the path, on the device ("next" rows: Camera::eyeRay, Phong shadow ray) ---------- */
/* Camera::eyeRay (Camera.cpp:104-161) for rows [y0,y1), spp samples per pixel, ray index
 * ((y-y0)*W+x)*spp+s.  jitter=0: pixel centres (randomize=false).  d_rays: device pointer. */
mr_status mr_gen_eye_rays(mr_scene *scene, const mr_camera *cam, uint32_t W, uint32_t H,
                          uint32_t y0, uint32_t y1, uint32_t spp, uint32_t jitter, uint32_t seed,
                          mr_ray *d_rays, void *stream);
/* The same rays in TILED order, for frames with fewer than 64 samples per pixel: the reference traces pixel by pixel
 * (Scene.cpp:112-140) and has no batch order to keep, and a wave whose 64 rays cover a square of pixels shares far more
 * of its BVH path than one on a 64 x 1 strip.  A pixel's spp rays stay consecutive (slot p = rays p*spp .. p*spp+spp-1);
 * the window's rows are taken in groups of th, each group in blocks of tw pixels, each block row by row, with
 * th x tw = 8x8, 8x4, 4x4, 4x2, 2x2, 2x1 for spp = 1, 2, 4, 8, 16, 32 (image order for any other spp).
 * mr_tile_pixel_map writes, for the same window, pixel_of_slot[p] = (y - y0) * W + x into a HOST array of W * rows
 * entries: everything downstream that works per ray (trace, shadow rays, shade) is order-agnostic, and a frame
 * buffer shaded in slot order is scattered to image order with this map. */
mr_status mr_gen_eye_rays_tiled(mr_scene *scene, const mr_camera *cam, uint32_t W, uint32_t H,
                                uint32_t y0, uint32_t y1, uint32_t spp, uint32_t jitter, uint32_t seed,
                                mr_ray *d_rays, void *stream);
mr_status mr_tile_pixel_map(uint32_t W, uint32_t rows, uint32_t spp, uint32_t *pixel_of_slot);
/* The scatter itself, on the device: d_image[((y - y0) * W + x) * channels + c] = d_slots[p * channels + c] for every
 * pixel slot p of the window (channels = 3 for the float framebuffer of mr_shade_direct).  Not in place. */
mr_status mr_untile_pixels(mr_scene *scene, const float *d_slots, float *d_image, uint32_t W, uint32_t rows,
                           uint32_t spp, uint32_t channels, void *stream);
/* Phong::shade shadow ray (Phong.cpp:80-97) for every hit, compacted with a wave64 ballot /
 * prefix sum.  d_out needs room for n rays; d_src[k] = index of the originating ray (may be NULL);
 * d_count: device uint64 receiving the number of shadow rays (zeroed by the call).
 * The compacted order is wave-granular, not ray order; use d_src to match. */
mr_status mr_gen_shadow_rays(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n,
                             const float light[3], mr_ray *d_out, uint32_t *d_src, uint64_t *d_count,
                             void *stream);
/* HitInfo::P and ::N as the object's intersect() leaves them (Triangle.cpp:160,162; Sphere.cpp:61-63;
 * Plane.cpp:42-44), device buffers of 3 floats per ray (either may be NULL).  d_rays (the rays the hits belong
 * to) may be NULL for scenes of triangles only.  On a scene with a STONE texture this stays the un-bumped, un-normalised
 * normal; mr_hit_surface gives the normal Scene::trace hands on (Scene.cpp:234-263). */
mr_status mr_hit_attrs(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n, float *d_P, float *d_N,
                       void *stream);

/* ---- Phong::shade for one point light over a traced frame ("next" row: the consumer of the shadow batch) --- */
typedef struct mr_light {                             /* PointLight.h:8-59 */
    float position[3], color[3], wattage;
} mr_light;
/* For n primary rays (spp consecutive rays per pixel) with their hits, and the traced shadow batch of
 * mr_gen_shadow_rays (hits + source indices + device count): direct lighting of a uniform material with
 * diffuse colour `diffuse` as Phong::shade computes it (Phong.cpp:44-160; opaque occluders only: MR_ERR_STATE when the
 * scene's material table holds a refractive material -- mr_shade_accumulate handles those), normals
 * normalised as Scene::trace does (Scene.cpp:262), misses = background 0 (Scene.cpp:340,685), averaged over
 * the spp samples of each pixel (Scene.cpp:126-139) into d_rgb[(n/spp)*3] -- the linear float framebuffer
 * (tempImage, Scene.cpp:106).  All pointers are device pointers. */
mr_status mr_shade_direct(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n,
                          const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src, const uint64_t *d_shadow_count,
                          const mr_light *light, const float diffuse[3], uint32_t spp, float *d_rgb, void *stream);
/* ---- the whole direct-light frame step in ONE launch ------------------------------------------------------------
 * Scene::raytraceImage's loop for a window of rows (Scene.cpp:112-141): for every sample Camera::eyeRay ->
 * Scene::trace -> the shadow ray of Phong::shade (Phong.cpp:80-97) -> Scene::trace -> Phong::shade -> the pixel's
 * mean.  The same rays, hit records and pixels, bit for bit, as
 *   mr_gen_eye_rays[_tiled] -> mr_trace -> mr_gen_shadow_rays -> mr_trace_indirect -> mr_shade_direct [-> mr_untile_pixels]
 * without any ray buffer: rays live in registers, the shadow ray is built from the hit the lane still holds.
 * Rows of the window: [y0,y1) when band_world == 1; otherwise the interleaved bands of one rank of a multi-GPU frame
 * (bands of band_rows rows dealt round-robin: rank r owns bands r, r + band_world, ...; y0/y1 ignored).
 * spp: a power of two <= 64 (other counts: use the batched calls).  tiled: sample order of mr_gen_eye_rays_tiled over
 * the window's rows (sample k of d_hits / d_shadow_hits follows that order); d_rgb is always in image order.
 * flags: MR_MATH_PRODUCT, MR_TRACE_INCOHERENT (both rays), MR_TRACE_ANY (shadow ray only), MR_FRAME_NO_SHADOWS.
 * Material: without mr_scene_set_materials the uniform Phong material of `diffuse` (what mr_shade_direct shades, and the
 * batched equivalence above holds bit for bit); once the scene has a material table, Phong::shade uses the material of the
 * object that was hit (Phong.cpp:116-156) and lets light through refractive occluders scaled by dot(N, l) of the occluder
 * (Phong.cpp:99-113) -- `diffuse` is ignored, the frame equals mr_trace_level(MR_LEVEL_LAST) over the eye rays, and
 * MR_TRACE_ANY is refused when a material is refractive (MR_ERR_STATE); default traversal only. */
typedef struct mr_frame_desc {
    mr_camera camera;
    uint32_t  W, H, y0, y1;
    uint32_t  band_rows, band_rank, band_world;   /* band_world <= 1: the contiguous window [y0,y1) */
    uint32_t  spp, jitter, seed, tiled, flags;
    mr_light  light;
    float     diffuse[3];
    uint32_t  reserved[4];
} mr_frame_desc;
/* d_rgb: rows*W*3 floats (window rows in band order).  Optional device outputs (NULL to skip): d_hits / d_shadow_hits,
 * rows*W*spp records each -- the shadow record of a sample whose primary ray missed is {t = 0, prim = MR_MISS};
 * d_counts[2]: += primary rays, += shadow rays traced (not zeroed by the call).
 * Streams: a frame of 60 000 chunks of 256 samples or more hands the last 6 % of its chunks out through one of 64 per-scene
 * device counters (taken round-robin per call, re-armed by the launch itself, so a captured HIP graph replays): calls on one
 * scene may overlap on different streams, up to 64 at a time; a captured graph keeps its counter -- do not replay it while
 * other frames of the same scene are in flight on other streams.
 * Memory: the default traversal of a triangle-only scene traces primary rays on tables relative to the camera eye, built on
 * `stream` by a launch in front of the frame when no earlier call left them for this eye; a scene keeps up to 64 such sets
 * (the least recently used one is rebuilt), each allocated on first use: 64 bytes per inner node + 48 per triangle record
 * (about the size of the scene's own node and triangle arrays), freed with the scene.  A captured graph rebuilds its set at
 * every replay. */
mr_status mr_render_direct(mr_scene *scene, const mr_frame_desc *frame, float *d_rgb, mr_hit *d_hits, mr_hit *d_shadow_hits,
                           uint64_t *d_counts, void *stream);
/* "mr_render_lights" (declared, with its whole contract, in miro_hip_surface.h): this frame over the scene's light list
 * (mr_scene_set_lights: point and disc lights) and its material table instead of `light` / `diffuse`, bit for bit
 * mr_gen_eye_rays[_tiled] -> mr_trace -> mr_shade_lights; one launch, no counters, no eye-relative tables.
 * "mr_render_lights_surface" (miro_hip_surface.h) is that frame on any scene, textured ones included, and
 * "mr_render_lights_environment" (declared, with its whole contract, in miro_hip_frame.h) the frame that gives a ray that
 * misses the environment of mr_scene_set_environment: the level-0 image of Scene::raytraceImage, background included. */

/* ---- multi-GPU frames: image rows dealt to the devices in interleaved bands -------------------
 * Bands of band_rows rows are dealt round-robin: band b (rows [b*band_rows, ...)) belongs to rank b % world and is that
 * rank's band number b / world; a rank keeps its rows in band order.  mr_band_locate answers, for image row y, which
 * rank owns it and where it sits in that rank's shard; mr_band_rows_of counts a rank's rows (host arithmetic, no device).
 * The reference hands rows to OpenMP workers two at a time (`schedule(dynamic, 2)`, Scene.cpp:113). */
mr_status mr_band_locate(uint32_t H, uint32_t band_rows, uint32_t world, uint32_t y, uint32_t *rank, uint32_t *local_row);
mr_status mr_band_rows_of(uint32_t H, uint32_t band_rows, uint32_t rank, uint32_t world, uint32_t *rows);
/* The de-interleave after the frame's single gather, on the device: d_recv holds `world` shards of shard_rows rows each
 * (shard_rows >= the largest rank's row count; rows of W pixels, floats_per_pixel floats per pixel: 3 for the float
 * framebuffer, 4 * spp for mr_hit records); row y of d_full (H rows) is copied from its owner's shard. */
mr_status mr_deinterleave_bands(mr_scene *scene, const float *d_recv, float *d_full, uint32_t W, uint32_t H, uint32_t band_rows,
                                uint32_t world, uint32_t shard_rows, uint32_t floats_per_pixel, void *stream);

/* ---- specular materials and secondary rays ("next" row: Scene::traceScene's recursion, Scene.cpp:302-336) -------- */
typedef struct mr_material {                          /* Phong(kd, ks, kt, shininess, refractIndex), Phong.h:10-14 */
    float diffuse[3], specular[3], transmission[3], shininess, refract_index;
} mr_material;
/* Materials of the scene (the Phong constructor's energy clamps are applied, Phong.cpp:12-33) and the material id
 * of every triangle in addObject order (NULL: material 0 everywhere).  Without this call every triangle is the white
 * Lambert of the BASELINE scenes.  May be called before or after mr_bvh_build. */
mr_status mr_scene_set_materials(mr_scene *scene, const mr_material *materials, uint32_t n_materials,
                                 const uint32_t *prim_material);
/* Phong::shade with per-triangle materials for a batch of rays of any bounce: d_weights (rgb per ray, NULL = 1) is the
 * product of reflection / transmission factors along the path, d_pixels (NULL = ray index / spp) the pixel the ray
 * contributes to; light through refractive occluders is attenuated as Phong.cpp:99-113 does (needs the shadow rays
 * themselves besides their hits).  Adds weight * L / spp to d_rgb[pixel] with float atomics. */
mr_status mr_shade_accumulate(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                              const uint32_t *d_pixels, uint64_t n, const mr_ray *d_shadow_rays, const mr_hit *d_shadow_hits,
                              const uint32_t *d_shadow_src, const uint64_t *d_shadow_count, const mr_light *light, uint32_t spp,
                              float *d_rgb, void *stream);
/* Ray::reflect / getReflectionCoefficient / refract (Ray.h:143-243) for every hit on a reflective or refractive
 * material: up to three children per ray (room for 3n), compacted by wave64 ballot + prefix sum, each with its path
 * weight and pixel.  d_count: device uint64 receiving the number of children (zeroed by the call).
 * out_capacity: rays the output arrays have room for.  Children beyond it are counted but not stored: *d_count >
 * out_capacity afterwards means the queue was too small (3n always suffices) -- nothing is written out of bounds.
 * d_out_octants (may be NULL): one byte per child, the sign bits of its direction -- mr_trace_grouped's d_octants. */
mr_status mr_gen_secondary_rays(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                const uint32_t *d_pixels, uint64_t n, uint32_t spp, mr_ray *d_out_rays, float *d_out_weights,
                                uint32_t *d_out_pixels, uint64_t *d_count, uint64_t out_capacity, uint8_t *d_out_octants,
                                void *stream);

/* The PATH_TRACING build of those generators (Ray.h:149-158,235-239) plus Ray::random (Ray.h:124-140): every child is
 * drawn from a lobe (alignHemisphereToVector, Utility.h:34-50) around the mirror / refracted direction with
 * phi = acos(pow(u1, 1/(1+shininess))), or -- the diffuse bounce -- around the normal with phi = asin(sqrt(u1));
 * theta = 2 pi u2.  u1, u2 replace the reference's rand() by the counter-based generator of the eye-ray jitter, keyed by
 * (seed, ray id, bounce, child kind).  kinds selects the children: MR_PATH_MIRROR | MR_PATH_REFRACT (Scene.cpp:302-336)
 * | MR_PATH_DIFFUSE (an extension: traceScene at HEAD never calls Ray::random); up to four children per ray (room for
 * 4n).  d_ids (NULL = ray index) are stable ray ids, d_out_ids (may be NULL) receives the children's.  out_capacity as
 * in mr_gen_secondary_rays (4n always suffices; n when kinds == MR_PATH_DIFFUSE).
 * mr_gen_path_rays_surface (declared in miro_hip_surface.h; csrc/mr_path_surface.hip) is the same call with d_color / d_normal
 * after d_hits, the two buffers of mr_hit_surface (3 n floats each, 4-byte aligned, read for rays with a hit only): every child
 * -- Ray::reflect, the Fresnel term, Ray::refract, Ray::random -- takes hit.N from d_normal, the normal as Scene::trace hands
 * it on (Scene.cpp:234-263, bumped on a STONE material), and the diffuse child carries weight * d_color, the diffuseColor of
 * Phong.cpp:51-56 that Scene::tracePhoton carries on (Scene.cpp:545-553, :608), instead of weight * m_diffuse.  WHICH children
 * a hit has stays the material's (isDiffuse / isReflective / isRefractive): a diffuse child whose colour is 0 is emitted with
 * weight 0.  Every other argument, check, key, child id and capacity rule is mr_gen_path_rays'; NULL or misaligned d_color /
 * d_normal: MR_ERR_INVALID.  It looks nothing up and refuses no texture table; on a scene without one the children are
 * mr_gen_path_rays' bit for bit. */
enum { MR_PATH_MIRROR = 1u, MR_PATH_REFRACT = 2u, MR_PATH_DIFFUSE = 4u };
mr_status mr_gen_path_rays(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                           const uint32_t *d_pixels, const uint32_t *d_ids, uint64_t n, uint32_t spp, uint32_t seed,
                           uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                           uint32_t *d_out_ids, uint64_t *d_count, uint64_t out_capacity, uint8_t *d_out_octants, void *stream);

/* ---- one level of Scene::traceScene's recursion (Scene.cpp:270-346) in ONE launch -------------------------------
 * For every ray of the queue: Scene::trace -> Phong::shade (shadow ray, Scene::trace, the occluder's light scale,
 * diffuse term + highlight, Phong.cpp:80-156) times the ray's weight, added to its pixel -> the children of the next
 * level.  The same hit records, shadow rays and children, bit for bit, as
 *   mr_trace -> mr_gen_shadow_rays -> mr_trace_indirect -> mr_shade_accumulate -> mr_gen_secondary_rays | mr_gen_path_rays
 * without the buffers between them: the hit stays in the lane's registers, the shadow ray is built from it and traced
 * by the same lane.  The children arrive in another ORDER than the batched generators' (compare the queues as sets,
 * by ray id under path tracing); the pixel sums differ by the order of the float atomics, as two runs of
 * mr_shade_accumulate do.
 * children: MR_LEVEL_LAST (none: the queue's rays are shaded only; the d_out_* may be NULL), MR_LEVEL_SPECULAR (the
 * generators of mr_gen_secondary_rays, room for 3n) or MR_LEVEL_PATH (those of mr_gen_path_rays with path_kinds, seed
 * and bounce as there, room for 4n).  flags: MR_MATH_PRODUCT, MR_TRACE_INCOHERENT.  d_weights / d_pixels / d_ids /
 * d_out_ids may be NULL as in mr_gen_path_rays.  d_out_count: zeroed by the call, receives the number of children.
 * out_capacity_lo / _hi (a 64-bit count in two words): rays the output queue has room for, required (> 0) for a level with
 * children; children beyond it are counted, not stored (*d_out_count > capacity: queue too small, nothing out of bounds).
 * d_counts (may be NULL): [0] += rays traced, [1] += shadow rays traced. */
enum { MR_LEVEL_LAST = 0u, MR_LEVEL_SPECULAR = 1u, MR_LEVEL_PATH = 2u };
typedef struct mr_level_desc {
    mr_light light;
    uint32_t spp, flags, children;
    uint32_t path_kinds, seed, bounce;
    uint32_t out_capacity_lo, out_capacity_hi;
    uint32_t reserved;
    uint8_t *d_out_octants;       /* may be NULL: per child, the sign bits of its direction (mr_order_by_octant's input) */
    const uint32_t *d_order;      /* may be NULL: lane k works on ray d_order[k] of the queue (a permutation of 0 ... n-1) */
} mr_level_desc;
mr_status mr_trace_level(mr_scene *scene, const mr_level_desc *level, const mr_ray *d_rays, const float *d_weights,
                         const uint32_t *d_pixels, const uint32_t *d_ids, uint64_t n, float *d_rgb, mr_ray *d_out_rays,
                         float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids, uint64_t *d_out_count,
                         uint64_t *d_counts, void *stream);

/* ---- Phong::shade over the scene's LIGHT LIST (Phong.cpp:59-63), point and disc lights, in ONE launch ---------------------
 * mr_scene_set_lights is Scene::addLight (Scene.h:29-30, assignment3.cpp:77-84,141-152) for the whole list: it replaces an
 * earlier list, n_lights == 0 clears it; before or after mr_bvh_build (the list lives on the host and travels in the kernel
 * arguments).  Only mr_shade_lights reads it: every other shading entry keeps its single mr_light argument.
 *   MR_LIGHT_POINT  PointLight (PointLight.h:8-59): position, color, wattage; normal and radius are ignored.
 *   MR_LIGHT_DISC   DirectionalAreaLight (DirectionalAreaLight.h:7-38 on SquareLight.h): the light mr_trace_photons emits from.
 * mr_shade_lights is Phong::shade (Phong.cpp:44-160) for n traced rays: per ray with a hit (a miss keeps L = 0: its product
 * weight * 0 is a zero, which is not added, unless the weight is not finite -- then it is the NaN that Scene.cpp:309-342 adds for
 * a child that leaves the scene, and that mr_trace_level_lights adds; mr_shade_accumulate skips every miss), L = 0;
 * for every light IN LIST ORDER the shadow ray is built (Phong.cpp:80-92) and traced (Scene::trace, closest hit: the occluder's
 * material matters), the occluder's light scale applied (Phong.cpp:97-113: opaque -> the light is skipped, refractive ->
 * dot(N, l), skipped if negative or < epsilon), and the light's diffuse term times the scale plus its highlight
 * (Phong.cpp:116-156) added to L; then weight * L / spp is added to d_rgb[pixel] exactly as mr_shade_accumulate does it
 * (d_weights NULL = 1, d_pixels NULL = ray index / spp, float atomics).  Materials: the table of mr_scene_set_materials, or the
 * white Lambert without one.  With ONE point light the result is, bit for bit where every pixel receives one addition, that of
 *   mr_gen_shadow_rays -> mr_trace_indirect -> mr_shade_accumulate
 * with that light, without the shadow-ray, shadow-hit, source-index and light-scale buffers (csrc/mr_lights.hip: the lane
 * keeps its hit point and builds and traces every shadow ray itself).
 * The disc light, as the reference treats it -- quirks reproduced, not repaired:
 *   - DirectionalAreaLight::getLightDirection ignores the origin Phong::shade samples (Phong.cpp:80-81): shading by a disc
 *     light uses NO random number.
 *   - l = -normal (as given); falloff = |l|^2; l /= sqrt(falloff).  Shadow ray: origin P + l * epsilon, direction l, tMin = 0,
 *     tMax = sqrt(falloff) = |normal| (Phong.cpp:85-97): with a unit normal an occluder is looked for only ONE UNIT towards
 *     the light, whatever the distance to the disc.
 *   - after the shadow test (the shadow ray is traced and counted either way): nDotL = dot(N, -normal) with the normal as
 *     given (not normalised), t = dot(normal, position - P) / -1.0f, and the light is skipped when
 *     |(P - t * normal) - position|^2 > radius^2 (the hit lies outside the disc's cylinder, Phong.cpp:128-133); falloff = 1 / PI
 *     instead of the point light's 1 / (4 PI^2 r^2) (Phong.cpp:135,140).
 *   - diffuse term and highlight are the point light's expressions with that nDotL / falloff and the normalised l
 *     (Phong.cpp:146-156).
 * d_ray_rgb (may be NULL): 3n floats, the un-weighted L of every ray (0 for a miss).  The sum over the lights happens in one
 *   lane in list order, so this output is deterministic; d_rgb carries the float-atomic order caveat of mr_shade_accumulate.
 *   d_rgb may be NULL when d_ray_rgb is given.
 * d_counts (may be NULL): [0] += shadow rays traced (= rays with a hit x lights); not zeroed by the call.
 * flags: MR_MATH_PRODUCT, MR_TRACE_INCOHERENT, and MR_TRACE_ANY for the shadow rays (refused with MR_ERR_STATE when the
 *   material table holds a refractive material, Phong.cpp:99-113).
 * With device buffers only, the call only enqueues one kernel on `stream` (it can be captured into a HIP graph).
 * Errors: NULL scene, n_lights > MR_MAX_LIGHTS, NULL list with n_lights > 0, unknown kind, non-zero reserved, a non-finite
 *   field, a disc with radius <= 0 or a zero normal: MR_ERR_INVALID (before any device call); mr_shade_lights on a scene
 *   that is not built, was built host_only or has no lights: MR_ERR_STATE. */
enum { MR_LIGHT_POINT = 0, MR_LIGHT_DISC = 1 };
#define MR_MAX_LIGHTS 8
typedef struct mr_light_desc {                        /* PointLight.h:8-59 / DirectionalAreaLight.h:7-38 */
    uint32_t kind;
    float position[3], normal[3], color[3], wattage, radius;   /* normal, radius: MR_LIGHT_DISC only */
    uint32_t reserved[4];                             /* must be 0 */
} mr_light_desc;
mr_status mr_scene_set_lights(mr_scene *scene, const mr_light_desc *lights, uint32_t n_lights);
mr_status mr_shade_lights(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                          const uint32_t *d_pixels, uint64_t n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb,
                          uint64_t *d_counts, void *stream);

/* ---- distribution effects: the thin-lens camera and the square area light (csrc/mr_distribution.hip) -----------------------
 * Both draw random numbers per sample from the counter-based generator of the eye-ray jitter, H(x) = pcg32(x),
 * u(h) = (h >> 8) / 2^24, and both accept the caller's own numbers instead.  No time has been measured for either.
 *
 * mr_gen_eye_rays_lens is Camera::eyeRay under -DDOF (Camera.cpp:135-160) with DOF_APERTURE / DOF_FOCUS_PLANE (Miro.h:18-19)
 * as arguments; raytraceImage averages TRACE_SAMPLES such rays per pixel (Scene.cpp:126-139): that is spp.  Its first eleven
 * arguments are mr_gen_eye_rays' (same window, same ray order ((y-y0)*W+x)*spp+s; there is no tiled form).  Per sample, every
 * operation in fp32 and in the reference's order:
 *   (lx, ly)    = sampleDisc(aperture) (Utility.h:82-95)
 *   new_eye     = eye + (lx * uDir + ly * vDir)                                        (Camera.cpp:140)
 *   new_viewDir = (eye + viewDir * focus_plane) - new_eye,  viewDir the unit view vector (Camera.cpp:142)
 *   localw      = normalize(-new_viewDir)                                              (Camera.cpp:145)
 *   dir         = normalize(uPos * uDir + vPos * vDir - localw)                        (Camera.cpp:157-160)
 *   ray         = (new_eye, tMin 0, dir, MIRO_TMAX)
 * uDir and vDir are those of the UNMOVED eye (Camera.cpp:146-147 are commented out in the reference): the quirk is
 * reproduced, not repaired.  With aperture == 0 the origin is the eye, but localw is rebuilt from eye + viewDir * focus_plane
 * and may differ from mr_gen_eye_rays' wDir in the last bit.
 * Samples, d_samples_in == NULL: with h = H(H(H(seed) ^ pixel) + s) the per-sample hash of mr_gen_eye_rays (pixel = y*W+x),
 *   dx = u(H(h)), dy = u(H(h ^ 0x68bc21eb)) exactly as there (0.5, 0.5 when jitter == 0), so the
 *   pixel jitter of a seed is unchanged; the lens pair of rejection round r = 0 ... 31 is
 *     x = (2 u(H(h ^ (0x4c454e53 + 2r))) - 1) * aperture,  y = (2 u(H(h ^ (0x4c454e53 + 2r + 1))) - 1) * aperture,
 *   accepted unless x*x + y*y > aperture*aperture (Utility.h:86-89).  The reference's loop is unbounded; here a sample that
 *   is rejected 32 times (probability (1 - PI/4)^32 = 4e-22) is (0, 0) and counted in d_counts[1].
 * d_samples_in (may be NULL): 4 floats per ray, dx, dy, lx, ly, used as they are (jitter and seed are then not read): for
 *   callers with their own stratified sampler.  d_samples_out (may be NULL): 4 floats per ray, the values used.
 * d_counts (may be NULL): [0] += rays written, [1] += samples that exhausted the 32 rounds; not zeroed by the call.
 * The call only enqueues one kernel on `stream`.
 * Errors (MR_ERR_INVALID, before any device call): NULL scene / cam / d_rays / lens, a non-zero reserved word, a non-finite or
 *   negative aperture, a non-finite or non-positive focus_plane, a bad window, d_rays or a sample buffer not 16-byte aligned.
 *
 * mr_shade_square_lights is Phong::shade (Phong.cpp:66-157) for n traced rays over a list of SquareLights (SquareLight.h:6-58
 * on PointLight.h:8-59) with `samples` shadow rays per hit and light (Phong.cpp:71-78; the reference ships samples = 1 and
 * keeps 49 in a comment).  Per ray with a hit, L = 0; for every light in list order and i = 0 ... samples-1:
 *   origin = samplePhotonOrigin(i, samples) (SquareLight.h:23-39): sideLength = sqrt((float)samples), du = dimensions[0] /
 *     sideLength, dv likewise, sx = i % int(sideLength), sy = i / int(sideLength),
 *     u = du*r0 + sx*du - dimensions[0]/2.0f, v = dv*r1 + sy*dv - dimensions[1]/2.0f, origin = position + u*t1 + v*t2 with
 *     (t1, t2) = getTangents(normal) (Utility.h:25-31; SquareLight::preCalc), computed on the host: mr_square_light_tangents
 *     returns them.  The normal only orients the rectangle: a SquareLight shades like a point light at `origin`.
 *   l = origin - P (PointLight::getLightDirection); then the point light's arm of Phong.cpp:85-156: shadow ray from
 *     P + l*epsilon along l/|l| with tMax = |l|, closest hit, the occluder rule of :99-113 (opaque: the sample is skipped,
 *     refractive: scaled by dot(N, l), skipped if negative or < epsilon), falloff = 1/(4 PI^2 |l|^2), and
 *     L += color * (max(0, nDotL*falloff*wattage / (float)samples) * diffuse * diffuse) * scale, then
 *     L += max(0, eDotr^500 * falloff*wattage / (float)samples) -- two additions per sample, as Phong.cpp:146,155 make them.
 *   (mr_shade_lights adds a light's two terms to each other first; for the first sample of a ray the two orders give the same
 *   bits, so dimensions = (0, 0), samples = 1 and one light is mr_shade_lights with one MR_LIGHT_POINT, bit for bit.)
 * Then weight * L / spp is added to d_rgb[pixel] exactly as mr_shade_lights adds it; d_ray_rgb is the deterministic per-ray L.
 * A sum over mixed light kinds takes one call per kind (mr_shade_lights for point and disc lights, this call for square
 * lights), each adding into d_rgb: the float addition order then differs from that of the reference's single list.
 * samples: a perfect square in {1, 4, 9, ..., 64}: for any other value int(sideLength)^2 != samples and the reference's cells
 *   leave the rectangle (MR_ERR_INVALID).
 * Random pairs (r0, r1), d_uv_in == NULL: h = H(H(H(seed ^ 0x73717561) ^ ray index) + 64*light + i), r0 = u(H(h)),
 *   r1 = u(H(h ^ 0x68bc21eb)).  d_uv_in (may be NULL): 2 * n * n_lights * samples floats in [0, 1), the pair of ray k, light j,
 *   sample i at 2 * ((k * n_lights + j) * samples + i); read for rays with a hit only.
 * d_counts (may be NULL): [0] += shadow rays traced (= rays with a hit x lights x samples); not zeroed by the call.
 * flags: those of mr_shade_lights; MR_TRACE_ANY is refused with MR_ERR_STATE when a material is refractive.
 * Materials: the table of mr_scene_set_materials.  A scene with a texture table (mr_scene_set_textures) is REFUSED with
 *   MR_ERR_STATE: this call shades without the texture lookup.  "mr_shade_square_lights_surface" (declared in
 *   miro_hip_surface.h) is the call for such a scene: the same arguments with d_color / d_normal, the two buffers of
 *   mr_hit_surface, after d_hits.  The hit's diffuseColor (the first factor of Phong.cpp:146; the second stays the material's
 *   m_diffuse) and its N (Phong.cpp:139,151) are read from them, for rays with a hit only; P is rebuilt from ray and hit, the
 *   occluder rule of :99-113 keeps the occluder's own normal.  Every other argument, check, random pair (the same seed, ray,
 *   light and sample give the same pair), output and error is this call's, but: NULL or not 4-byte aligned d_color / d_normal
 *   are MR_ERR_INVALID, and no texture table is refused -- it looks nothing up and runs on any built scene
 *   (csrc/mr_square_surface.hip).
 * The call only enqueues one kernel on `stream`.
 * Errors: NULL scene, n_lights == 0 or > MR_MAX_LIGHTS, NULL list, non-zero reserved, a non-finite field, a zero normal,
 *   a negative dimension, samples not such a square, NULL rays / hits, both outputs NULL, spp == 0, n >= 2^32, other flags,
 *   misaligned buffers (rays / hits 16 bytes, counters / d_uv_in 8): MR_ERR_INVALID (before any device call, and before the
 *   scene's state is looked at); a scene that is not built or was built host_only: MR_ERR_STATE. */
typedef struct mr_lens_desc {                         /* Miro.h:18-19 */
    float aperture, focus_plane;                      /* DOF_APERTURE (radius of the lens disc), DOF_FOCUS_PLANE */
    uint32_t reserved[6];                             /* must be 0 */
} mr_lens_desc;
mr_status mr_gen_eye_rays_lens(mr_scene *scene, const mr_camera *cam, uint32_t W, uint32_t H,
                               uint32_t y0, uint32_t y1, uint32_t spp, uint32_t jitter, uint32_t seed,
                               mr_ray *d_rays, void *stream, const mr_lens_desc *lens, const float *d_samples_in,
                               float *d_samples_out, uint64_t *d_counts);
typedef struct mr_square_light_desc {                 /* SquareLight.h:6-58 on PointLight.h:8-59 */
    float position[3], normal[3], color[3], wattage, dimensions[2];
    uint32_t reserved[4];                             /* must be 0 */
} mr_square_light_desc;
mr_status mr_square_light_tangents(const float normal[3], float t1[3], float t2[3]);   /* getTangents (Utility.h:25-31) */
mr_status mr_shade_square_lights(mr_scene *scene, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t samples,
                                 uint32_t seed, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                 const uint32_t *d_pixels, const float *d_uv_in, uint64_t n, uint32_t spp, uint32_t flags,
                                 float *d_rgb, float *d_ray_rgb, uint64_t *d_counts, void *stream);

/* ---- the environment of rays that MISS: Scene::getEnvironmentMap (Scene.cpp:338-342,657-688) ------------------------------
 * Scene::traceScene ends a ray that leaves the scene with shadeResult = getEnvironmentMap(ray), which its parent multiplies by
 * the reflection / refraction factor like any child result.  getEnvironmentMap returns m_bgColor (Scene::setBgColor, default 0)
 * or, with an image (Scene::setEnvironment(new LoadedTexture(...)), setEnvironmentRotation, assignment3.cpp:50-52), a bilinear
 * lookup into the lat-long image: the full image for ordinary rays, the 24-texel-wide blurred copy the LoadedTexture
 * constructor builds (Texture.cpp:52-91) for rays made by Ray::random (ray.isDiffuse).  Without mr_scene_set_environment
 * (m_environment = 0, m_bgColor = 0) a miss is worth 0, which is what every other entry point assumes: only
 * mr_shade_environment reads the environment.
 *
 * mr_scene_set_environment -- host only (works on a host_only scene and without a device), before or after mr_bvh_build;
 * copies the image; env == NULL restores the default.  The device copy is made by the first mr_shade_environment after a
 * change, on that call's stream.  pixels: a float RGB image (FreeImage's FIT_RGBF; 8-bit FIT_BITMAP images are not
 * supported), W * H * 3 floats, row y = FreeImage scanline y (row 0 is the BOTTOM row of the picture).  The call reproduces
 * LoadedTexture::LoadedTexture (Texture.cpp:30-92) as written:
 *   - m_maxIntensity = the maximum over all channels of all pixels, starting from -1e15.
 *   - the low-res image: width 24, height lrh = (int)(24.0f * ((float)H / (float)W)); texel (j, i) is the UN-NORMALISED
 *     Gaussian-weighted sum over its block of (W / 24) x (H / lrh) pixels (integer divisions), sigma = 1, centred on the
 *     block's middle pixel: weight 1.0 / (2.0 * PI * sigma) * exp(float), accumulated in long double (it is no average: the
 *     weights of a block sum to about 1 only because sigma = 1).
 *   - the texel is stored through setPixel's FIT_RGBF arm (Texture.cpp:118-124), which EXCHANGES GREEN AND BLUE: the
 *     low-res image holds (r, b, g).
 * Errors (MR_ERR_INVALID, the earlier environment stays): NULL scene, a non-zero reserved word, a non-finite bg_color /
 * rotation / pixel, pixels with W < 24, with a low-res height of 0 or with H > 4 W (the low-res image is kept in LDS),
 * rotation[0] outside [0, 2 pi] or rotation[1] outside [0, pi / 2] (beyond them the reference's lookup leaves its bitmap).
 *
 * mr_scene_get_environment -- which = 0: the image as given, 1: the low-res image as stored (green and blue exchanged).
 * *W, *H, *max_intensity (any may be NULL) and, when pixels != NULL, W * H * 3 floats.  Without an image: W = H = 0,
 * max_intensity = 0.
 *
 * mr_shade_environment -- for n traced rays: every ray whose hit record is a MISS takes value = getEnvironmentMap(ray) and
 * adds weight * value / spp to d_rgb[pixel] exactly as mr_shade_accumulate does (d_weights NULL = 1, d_pixels NULL = ray
 * index / spp, float atomics); rays with a hit contribute nothing.  The lookup (Scene.cpp:664-681, Texture.cpp:161-185), every
 * operation in fp32 in the reference's order, with atan2 / asin from miro_math.h (the same bits in a host checker):
 *     phi = atan2(d.x, d.z) + rot[0] + PI;   theta = asin(d.y) + rot[1];
 *     if (theta > PI / 2) { phi += PI; theta -= 2 * (theta - PI / 2); }      if (phi > 2 PI) phi -= 2 PI;   (once)
 *     u = phi / (2 PI);   v = theta / PI + 0.5;
 *     px = (float)w * u;   x1 = (int)px;  x2 = x1 + 1;  x1 %= w;  x2 %= w;   x1_error = px - (float)x1;    (the same in y)
 *     f = (p(x1,y1) * (1 - x1_error) + p(x2,y1) * x1_error) * (1 - y1_error) + (p(x1,y2) * (1 - x1_error) + p(x2,y2) * x1_error) * y1_error
 *     value = min(powf(f / max_intensity, 0.5f) * 1.5f, 1.0f) per channel   (std::min: a NaN stays a NaN)
 *   x1_error is taken from the WRAPPED x1: at u == 1 (or v == 1) the index wraps to 0, the error term is w (or h) and the
 *   blend extrapolates -- reproduced.  Where the reference's arithmetic leaves the image -- u or v not finite (a direction
 *   whose |y| exceeds 1 by an ulp: asin gives NaN), an index beyond int, a negative index -- its behaviour is undefined;
 *   here such a lookup is DEFINED as 0 and counted.
 * The low-res image is used for ray i when flags & MR_ENV_LOWRES or d_lowres && d_lowres[i] (the reference's ray.isDiffuse).
 * Without an image every miss yields bg_color; without any environment the call is valid and adds nothing.
 * d_ray_rgb (may be NULL): 3n floats, the un-weighted value of every ray, 0 for a hit; deterministic.  d_rgb may be NULL when
 *   d_ray_rgb is given.
 * d_counts (may be NULL): [0] += misses shaded, [1] += undefined lookups; not zeroed by the call.
 * flags: MR_ENV_LOWRES only.
 * With device buffers the call only enqueues on `stream`; once the device copy of the image exists (after one call) it can be
 * captured into a HIP graph.  One mr_scene_set_environment at a time, and none while a shade call is in flight.
 * Errors: NULL scene / rays / hits, both outputs NULL, spp == 0, other flags, misaligned buffers: MR_ERR_INVALID; a scene that
 *   is not built or was built host_only: MR_ERR_STATE. */
typedef struct mr_environment_desc {
    float bg_color[3];            /* Scene::setBgColor; used when pixels == NULL */
    const float *pixels;          /* host, W*H*3 floats, row y = FreeImage scanline y (row 0 = bottom), or NULL */
    uint32_t W, H;
    float rotation[2];            /* setEnvironmentRotation(phi, theta) */
    uint32_t reserved[6];         /* must be 0 */
} mr_environment_desc;
enum { MR_ENV_LOWRES = 1u << 16 };
mr_status mr_scene_set_environment(mr_scene *scene, const mr_environment_desc *env);
mr_status mr_scene_get_environment(const mr_scene *scene, uint32_t which, uint32_t *W, uint32_t *H, float *max_intensity,
                                   float *pixels);
mr_status mr_shade_environment(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                               const uint32_t *d_pixels, const uint8_t *d_lowres, uint64_t n, uint32_t spp, uint32_t flags,
                               float *d_rgb, float *d_ray_rgb, uint64_t *d_counts, void *stream);

/* ---- textured Phong materials: TexturedPhong (Texture.cpp:509-527), UV mapping, checker and image textures ------------------
 * Phong::shade takes its diffuse colour from the material: diffuseColor = diffuse2D(hit.object->toUVCoordinates(hit.P))
 * (Phong.cpp:51-56).  For a plain Phong that is m_diffuse; for a TexturedPhong it is Texture::lookup2D at the object's UV
 * coordinates, and the light's diffuse term is max(0, nDotL * falloff * wattage) * diffuseColor * m_diffuse (Phong.cpp:146); the
 * highlight does not see the texture.  A scene may carry up to MR_MAX_TEXTURES 2-D textures and a material may name one;
 * mr_shade_lights and mr_shade_accumulate then run their textured kernels (csrc/mr_textures.hip).  A scene without a texture
 * table is untouched: the same kernels, the same bits.
 *
 * UV coordinates of a hit (csrc/mr_uv.h), every operation fp32 in the reference's order:
 *   plane     (P.x, P.z)  (Plane.cpp:50-60; also Object's default, Object.h:37)
 *   sphere    dir = normalize(P - centre); u = atan2(dir.x, dir.z) / (2 PI) + 0.5; v = max(-1, min(1, asin(dir.y))) / PI + 0.5
 *             (Sphere.cpp:83-95).  The clamp is on the ANGLE, to +-1 radian: v stays inside about [0.18, 0.82] -- reproduced, not
 *             repaired.  atan2 / asin are those of miro_math.h; `+ 0.5` is a double addition rounded to float.
 *   triangle  (0, 0) when its mesh has no texture coordinates; otherwise Triangle.cpp:172-222: one axis is dropped by the rule
 *             normal.x > normal.z -> (i, j) = (2, 1), else normal.y > normal.z -> (0, 2), else (0, 1) on the signed,
 *             un-normalised cross(B-A, C-A); beta = max(detPC / detBC, 0), gamma = max(detBP / detBC, 0),
 *             alpha = max(1 - (beta + gamma), 0) with std::max(a, b) = a < b ? b : a (a NaN quotient stays: a degenerate
 *             projection, detBC == 0, propagates); uv = alpha * tA + beta * tB + gamma * tC, summed left to right.
 *
 * mr_scene_set_texcoords -- TriangleMesh::m_texCoords / m_texCoordIndices for the whole scene: n_texcoords uv pairs and three
 * indices per object in addObject order (spheres included; their entries are ignored), MR_NO_TEXCOORD in all three = this
 * triangle's mesh has none.  Replaces an earlier table (also the one mr_scene_add_obj made from `vt` records and v/t, v/t/n
 * face corners, which needs no call); n_texcoords == 0 clears it.  Before or after mr_bvh_build, like mr_scene_set_materials;
 * objects added afterwards have none.  Errors (MR_ERR_INVALID, the earlier table stays): NULL scene, NULL arrays, a non-finite
 * coordinate, an index >= n_texcoords, MR_NO_TEXCOORD in some but not all of an object's three.
 * mr_scene_get_texcoords -- the table back: *n_texcoords, 2 * n_texcoords floats and 3 indices per object (any may be NULL).
 *
 * mr_scene_set_textures -- host only (works on a host_only scene), copies its inputs, replaces an earlier table;
 * n_textures == 0 clears it.  The device copy is made by the first shading call after a change, on that call's stream.
 * material_texture: one texture id per material of mr_scene_set_materials' table (MR_NO_TEXTURE = plain Phong), or NULL (no
 * material names a texture).  A material that names a texture is a TexturedPhong: its m_diffuse becomes what the Phong
 * constructor's clamps make of kd = 1 (Texture.cpp:513-514, Phong.cpp:24-31), clamp(1 - ks - kt, 0, 1) per channel -- the call
 * writes that into the stored material record WHATEVER `diffuse` the caller put in mr_material, and clearing the table does not
 * bring the old value back (set the materials again).  While a table exists mr_scene_set_materials is refused (MR_ERR_STATE:
 * the table names materials by index): clear, set materials, set textures.
 *   MR_TEX_CHECKER  CheckerBoardTexture (Texture.h:112-133): u' = |scale * u|, plus scale when u < 0, the same for v;
 *                   ((int)u' + (int)v') % 2 == 0 ? color1 : color2.  Coordinates that are not finite, or whose scaled magnitude
 *                   reaches 2^30, are undefined in the reference; here they are DEFINED as color1 and counted.
 *   MR_TEX_IMAGE    LoadedTexture (Texture.cpp:23-28,131-185): W * H * 3 floats, row 0 = the bottom scanline (the environment's
 *                   convention).  hdr = 1 is FIT_RGBF: m_maxIntensity is computed as the constructor does and
 *                   tonemapValue = min(powf(f / max, 0.5f) * 1.5f, 1); hdr = 0 is FIT_BITMAP: pass channel / 255, tonemapValue
 *                   is the identity.  Phong::shade calls lookup2D, the full-resolution image: no low-res copy is built (no
 *                   24-texel minimum).  The bilinear lookup is mr_shade_environment's (wrapped indices, the error term taken
 *                   from the wrapped index: u == 1 extrapolates).  A lookup that leaves the image in the reference (negative or
 *                   non-finite u / v, an index beyond int) is DEFINED as 0 and counted -- for every negative coordinate,
 *                   the sliver -1 / W < u < 0 included, where the reference's truncation happens to stay on texel 0.
 *   MR_TEX_STONE    StoneTexture(scale) (Texture.h:101-110, Texture.cpp:358-440): flagstones from WorleyNoise::noise2D of order 3
 *                   with Perlin turbulence, and the one texture whose bumpHeight2D is not 0 -- Scene::trace bump-maps the normal
 *                   of a hit on it (Scene.cpp:234-263).  Only `scale` is read.  A material that names one must have ks = kt = 0,
 *                   as the reference's own uses have (assignment1.cpp:232,313): no reflected or refracted ray and no light
 *                   through a refractive occluder (Phong.cpp:99-113 reads the occluder's N) ever needs a bumped normal.
 *   MR_TEX_STEM     StemTexture(scale) (Texture.h:184-213): green from the same two noises; bump height 0.  Only `scale` is read.
 *                   The two noises are pure functions over two fixed tables (csrc/mr_noise.h), pinned to values recorded from
 *                   the reference's own lib/src/Perlin.cpp and lib/src/Worley.cpp (tests/golden/noise_kat.npz).  A coordinate
 *                   that is NaN or reaches 2^30 after scaling fails int(floor()) there: DEFINED as noise 0 here and counted.
 *                   powf / exp are the series of miro_math.h, where the reference calls libm; pow(f1f0, 2) (Texture.cpp:424)
 *                   is the float product of the C++03 std::pow(float, int).
 *   The three UVW kinds are the reference's Texture3D classes.  Phong::shade looks them up at the hit point itself,
 *   diffuse3D(tex_coord3d_t(hit.P.x, hit.P.y, hit.P.z)) (Phong.cpp:53-56): no object mapping and no texture coordinates are
 *   involved, and Scene::trace bump-maps UV materials only (Scene.cpp:238), so the normal stays the geometric one, normalised,
 *   and ks / kt are not restricted.  They reuse the struct's fields: color1 = the pivot, color2[0] = the radius.
 *   MR_TEX_PETAL    PetalTexture(pivot, radius, scale) (Texture.h:171-181, Texture.cpp:442-505): p = normalize(P - pivot), dist =
 *                   |P - pivot| / radius, v = acos(-p.y) / PI, u = acos(p.x) / (2 PI), mirrored to 1 - u unless p.z < 0; two Perlin
 *                   turbulences at (u, v / 4) (10 octaves) and (u, v) (25 octaves) blend a base and a tip colour with a highlight
 *                   and a depression.  `scale` is not read (lookup3D never reads m_scale).
 *   MR_TEX_LEAF     LeafTexture(pivot, direction, scale) (Texture.h:216-251): StemTexture::lookup2D's body at (P.x * scale,
 *                   P.y * scale).  Only `scale` is read: pivot and direction are constructor arguments the lookup never uses.
 *   MR_TEX_FLOWER_CENTER  FlowerCenterTexture(pivot, radius, scale) (Texture.h:253-277): fraction = clamp(powf(|P - pivot| /
 *                   radius, 30), 0, 1) blends (0.31, 0.18) into (0.92, 0.71), blue 0.1f.  `scale` is not read.
 *                   What counts as undefined in a PETAL lookup: its 25-octave turbulence reaches the frequency 4 * 3^24, about
 *                   1.1e12, far beyond int(floor()).  An evaluation ALL of whose coordinates are whole numbers (every float from
 *                   2^23 on is one, and z is 0) is +-0 in the reference whatever the conversion yields -- the fractions are 0, so
 *                   every grad is +-0 and every lerp weight 0: it contributes 0 and is NOT counted.  An evaluation with a coordinate
 *                   that is NaN or reaches 2^30 and another that is not whole is undefined there: noise 0 here, and counted (about
 *                   0.4 % of the lookups at uniform (u, v)).  P == pivot gives NaN coordinates, an acos argument a rounding above 1
 *                   gives NaN: both propagate as the reference's arithmetic has them and are counted by the same rule.  acos and
 *                   powf are the series of miro_math.h.  CloudTexture is not a kind: it overloads lookup2D(const tex_coord3d_t &)
 *                   instead of overriding lookup3D (Texture.h:152), so as a material it is the base class's black.
 * Errors (MR_ERR_INVALID, the earlier table stays): NULL scene, n_textures > MR_MAX_TEXTURES, NULL list, unknown kind, non-zero
 *   reserved word, non-finite field (also one the kind does not read) or pixel, W or H of 0 (or above 65536), NULL pixels,
 *   hdr > 1, a texture id >= n_textures, a material_texture given without a material table, a STONE texture named by a material
 *   with a non-zero kt, or with a non-zero ks unless the texture says MR_TEX_REFLECTIVE (miro_hip_bump.h says what such a scene
 *   changes), a PETAL or FLOWER_CENTER texture whose radius is not finite and greater than 0.
 *
 * mr_hit_uv -- toUVCoordinates(hit.P) of n traced rays: d_uv receives 2n floats, (0, 0) for a miss.  d_rays may be NULL for
 *   scenes of triangles only.  mr_texture_lookup -- lookup2D of texture `texture` at n coordinates (d_uv: 2n floats): d_rgb
 *   receives 3n floats; d_counts (may be NULL): [0] += undefined lookups, not zeroed.  Both only enqueue on `stream`.
 *
 *   mr_texture_lookup serves the four UV kinds; on a UVW kind it returns MR_ERR_INVALID naming mr_texture_lookup3 (lookup2D of a
 *   Texture3D is the base class's black, Texture.h:66).
 * mr_texture_lookup3 -- Texture::lookup3D of the UVW texture `texture` at n points (d_p: 3n floats): d_rgb receives 3n floats.
 *   d_coords (may be NULL): for a PETAL, (u, v, dist) of Texture.cpp:465-492 per point, 3n floats -- the coordinates the noise
 *   is evaluated at and the blend factor; not written for the other two kinds.  d_counts (may be NULL): [0] += the lookups the
 *   reference leaves undefined (above), not zeroed.  MR_ERR_INVALID naming mr_texture_lookup on a UV kind.  Only enqueues on
 *   `stream`.
 *
 * Entry points that shade without the lookup refuse a scene with a texture table (MR_ERR_STATE, naming the batched calls):
 * mr_render_direct, mr_shade_direct, mr_trace_level, and mr_trace_photons (its roulette reads diffuse2D, Scene.cpp:545-551;
 * mr_trace_photons_surface is the walk with the lookup).
 *
 * ---- procedural textures and bump-mapped normals: a per-hit surface pass (csrc/mr_procedural.hip) ----
 * A STONE or STEM lookup is too heavy to sit inside a kernel that also traverses (five Worley searches and up to 33 Perlin
 * evaluations per stone hit), so a scene whose table holds one is shaded in two steps: mr_hit_surface, then a _surface call.
 * mr_hit_surface -- for every ray of a traced batch that hit: d_color[3k..] = diffuseColor of Phong.cpp:51-56 (m_diffuse of a
 *   plain Phong, Texture::lookup2D at Object::toUVCoordinates(hit.P) of a TexturedPhong with a UV texture, Texture::lookup3D at
 *   hit.P itself with a UVW texture; all seven kinds in any mixture) and d_normal[3k..] =
 *   HitInfo::N as Scene::trace leaves it (Scene.cpp:234-263): on a STONE material four bumpHeight2D samples at (u -+ delta, v),
 *   (u, v -+ delta) with delta = (float)0.0001, dx and dy by central differences, randomVec by the largest component of N, t1 =
 *   cross(N, randomVec), N += dx * cross(N, t1) - dy * cross(N, cross(N, t1)), then normalize(); on every other material the
 *   normalisation alone (the zero perturbation is skipped; a UVW material gets neither toUVCoordinates nor the bump).  One
 *   kernel serves every scene (csrc/mr_procedural.hip).  A ray that missed leaves its six floats untouched.  Works on any
 *   scene, with or without a texture table.  d_counts (may be NULL): [0] += hits whose lookup the reference leaves undefined,
 *   not zeroed.  d_rays may be NULL for scenes of triangles only.
 * mr_shade_lights_surface, mr_shade_accumulate_surface -- mr_shade_lights (Phong.cpp:44-150 over the light list) and
 *   mr_shade_accumulate with the hit's diffuseColor and N read from d_color / d_normal (24 bytes per ray) instead of computed;
 *   every other argument, check and output is the plain call's.  They look nothing up, so they run on any scene.
 * mr_shade_square_lights_surface (declared in miro_hip_surface.h; csrc/mr_square_surface.hip) -- mr_shade_square_lights the same
 *   way: d_color / d_normal follow d_hits, soft shadows on a stone floor or on the flower.  Documented with
 *   mr_shade_square_lights above.
 * mr_texture_bump_height -- Texture::bumpHeight2D (Texture.h:63; StoneTexture's: Texture.cpp:358-393) of texture `texture` at n
 *   coordinates (d_uv: 2n floats) into d_height (n floats): 0 for every kind but STONE, the UVW kinds included.
 * mr_noise_probe -- the noise functions themselves, needs no scene: MR_NOISE_PERLIN reads xyz triples (3n floats) and writes
 *   PerlinNoise::noise (Perlin.h:16-51), n floats; MR_NOISE_WORLEY2 reads xy pairs (2n floats) and writes, per point, F[3] as
 *   floats then ID[3] as uint32 of WorleyNoise::noise2D(at, 3, ...) (Worley.cpp:95-173), 6n words.  Runs on the current device.
 * All six only enqueue on `stream`.
 *
 * On a scene whose table holds a STONE, STEM or UVW texture the calls that would compute the colour or the normal themselves
 * return MR_ERR_STATE with a message naming their _surface form: mr_shade_lights, mr_shade_accumulate, mr_shade_square_lights
 * (which refuses every texture table, checker and image included: mr_shade_square_lights_surface is its form for all of them),
 * and mr_gen_path_rays with MR_PATH_DIFFUSE (Ray::random bounces about N; mr_gen_path_rays_surface is its form).  The first
 * three have no lookup3D; the last would bounce about the right normal on a UVW scene, whose normals nothing bumps, but would
 * still carry m_diffuse instead of the looked-up colour.  A scene without them runs the kernels it ran before.  Still without a
 * surface form: mr_trace_level, which refuses every texture table.  mr_gen_secondary_rays emits no diffuse child and needs its
 * surface form, mr_gen_secondary_rays_surface (miro_hip_bump.h), only where a STONE material has ks != 0: on such a scene it
 * and mr_gen_path_rays with MR_PATH_MIRROR return MR_ERR_STATE and name their _surface form; a STONE material has kt = 0. */
enum { MR_TEX_CHECKER = 0, MR_TEX_IMAGE = 1, MR_TEX_STONE = 2, MR_TEX_STEM = 3, MR_TEX_PETAL = 4, MR_TEX_LEAF = 5, MR_TEX_FLOWER_CENTER = 6 };
#define MR_MAX_TEXTURES 16
#define MR_NO_TEXTURE  0xFFFFFFFFu
#define MR_NO_TEXCOORD 0xFFFFFFFFu
typedef struct mr_texture_desc {
    uint32_t kind;
    float color1[3], color2[3], scale;                /* MR_TEX_CHECKER; MR_TEX_STONE, MR_TEX_STEM and MR_TEX_LEAF read scale alone;
                                                         MR_TEX_PETAL and MR_TEX_FLOWER_CENTER: color1 = pivot, color2[0] = radius */
    const float *pixels;                              /* MR_TEX_IMAGE: host, W*H*3 floats, row 0 = bottom */
    uint32_t W, H, hdr;
    uint32_t reserved[5];                             /* must be 0; [0] of a MR_TEX_STONE may be MR_TEX_REFLECTIVE (miro_hip_bump.h) */
} mr_texture_desc;
mr_status mr_scene_set_texcoords(mr_scene *scene, const float *texcoords, uint32_t n_texcoords, const uint32_t *tidx);
mr_status mr_scene_get_texcoords(const mr_scene *scene, uint32_t *n_texcoords, float *texcoords, uint32_t *tidx);
mr_status mr_scene_set_textures(mr_scene *scene, const mr_texture_desc *textures, uint32_t n_textures,
                                const uint32_t *material_texture);
mr_status mr_hit_uv(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n, float *d_uv, void *stream);
mr_status mr_texture_lookup(mr_scene *scene, uint32_t texture, const float *d_uv, uint64_t n, float *d_rgb, uint64_t *d_counts,
                            void *stream);
mr_status mr_texture_lookup3(mr_scene *scene, uint32_t texture, const float *d_p, uint64_t n, float *d_rgb, float *d_coords,
                             uint64_t *d_counts, void *stream);
enum { MR_NOISE_PERLIN = 0, MR_NOISE_WORLEY2 = 1 };
mr_status mr_hit_surface(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n, float *d_color, float *d_normal,
                         uint64_t *d_counts, void *stream);
mr_status mr_shade_lights_surface(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                  const float *d_normal, const float *d_weights, const uint32_t *d_pixels, uint64_t n, uint32_t spp,
                                  uint32_t flags, float *d_rgb, float *d_ray_rgb, uint64_t *d_counts, void *stream);
mr_status mr_shade_accumulate_surface(mr_scene *scene, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                      const float *d_normal, const float *d_weights, const uint32_t *d_pixels, uint64_t n,
                                      const mr_ray *d_shadow_rays, const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src,
                                      const uint64_t *d_shadow_count, const mr_light *light, uint32_t spp, float *d_rgb, void *stream);
mr_status mr_texture_bump_height(mr_scene *scene, uint32_t texture, const float *d_uv, uint64_t n, float *d_height, void *stream);
mr_status mr_noise_probe(uint32_t which, const float *d_in, uint64_t n, float *d_out, void *stream);

/* sigmoid(6v-3) tone map + 8-bit quantisation (Scene.cpp:87-91,177-202; Image.cpp:44-50) */
mr_status mr_tonemap(mr_scene *scene, const float *d_rgb, uint64_t n_values, uint8_t *d_out, void *stream);

/* ---- photon map (BASELINE config 5): Photon_map of PhotonMap.h:42-105 ---------------------------------------- */
typedef struct mr_photon_map mr_photon_map;
mr_status mr_photon_map_create(int32_t device, uint32_t max_photons, mr_photon_map **out);     /* Photon_map(max_phot) */
mr_status mr_photon_map_destroy(mr_photon_map *map);
/* Photon_map::store (PhotonMap.cpp:255-289) for n photons: power, position, incoming direction (xyz triples);
 * photons beyond max_photons are dropped silently, as in the reference */
mr_status mr_photon_map_store(mr_photon_map *map, uint32_t n, const float *power, const float *pos, const float *dir);
mr_status mr_photon_map_scale(mr_photon_map *map, float scale);        /* scale_photon_power (:298-306) */
/* Photon_map::balance (:314-359): left-balanced kd-tree in heap order; uploads unless host_only */
mr_status mr_photon_map_balance(mr_photon_map *map, uint32_t host_only);
/* "mr_photon_map_build_device" (declared in miro_hip_surface.h): store(n records) + scale_photon_power(scale) + balance() of an
 * EMPTY map in one call, on the device, from a device array of mr_photon_record: hand-written kernels (csrc/mr_photon_build.hip)
 * store the photons, sort three lists by (coordinate, storage index), build the left-balanced tree one heap level per step,
 * and pack the planes and block boxes.  The map is then balanced and resident exactly as the three calls above would have left
 * it -- same photon at every node, same split axes, direction bytes and powers, same boxes -- and mr_photon_map_store /
 * _scale are refused as after mr_photon_map_balance (which itself is then a no-op).  mr_photon_map_export reads the device
 * arrays back.  Opt-in: the three host calls are unchanged and remain the yardstick. */
mr_status mr_photon_map_count(const mr_photon_map *map, uint32_t *stored);
/* balanced tree in heap order (any pointer may be NULL): pos[3n], plane[n], theta_phi[2n] (quantised direction), power[3n] */
mr_status mr_photon_map_export(const mr_photon_map *map, float *pos, int32_t *plane, uint8_t *theta_phi, float *power);
/* Photon_map::irradiance_estimate (:81-145), batched: for each query (surface position + normal, xyz triples on the
 * device) the nphotons (<= 512) nearest photons within max_dist whose incoming direction faces the normal;
 * d_irrad[3q..] = sum of their powers * (1/pi)/r^2.  d_found / d_r2 (optional) receive np.found and np.dist2[0]. */
mr_status mr_irradiance_estimate(mr_photon_map *map, const float *d_pos, const float *d_normal, uint64_t n_queries,
                                 float max_dist, uint32_t nphotons, float *d_irrad, int32_t *d_found, float *d_r2,
                                 void *stream);
/* Work counters of the estimates on this map, like MR_COUNT_STATS for the traversal (the reference has no counterpart:
 * Stats.h counts nothing in PhotonMap.cpp).  While enabled, every mr_irradiance_estimate / mr_final_gather on the map runs
 * the counting build of the kernel and adds to: [0] queries answered, [1] blocks of 63 kd-tree nodes examined, [2] photon
 * records (position + direction, 32 bytes) examined by the search, [3] radius tightenings (k-th-nearest selections),
 * [4] photon records examined by the reference-order pre-pass that finds the first overflow's victim
 * (PhotonMap.cpp:195-240), [5] searches repeated because a guessed radius did not hold the k nearest, [6] child-block boxes
 * measured (64 bytes each), [7] candidates buffered, [8] blocks expanded (64 child boxes each), [10] queries searched from
 * the pre-pass's safe radius (no guess available); [9], [11] unused. */
mr_status mr_photon_map_count_stats(mr_photon_map *map, int32_t enable);
mr_status mr_photon_map_get_stats(mr_photon_map *map, uint64_t counters[12], int32_t reset);

/* The photon-map term of Scene::traceScene (Scene.cpp:285-299) for a traced batch: for every ray whose hit has a
 * diffuse material (Phong::isDiffuse), irradiance_estimate on the global and on the caustic map (either may be NULL)
 * at the hit point with the normalised normal, and (irradiance + caustic) averaged over the pixel's spp samples
 * added to d_rgb[ray / spp].  d_scratch: 12 * n floats on the device (query positions, normals, two results). */
mr_status mr_final_gather(mr_scene *scene, mr_photon_map *global_map, mr_photon_map *caustic_map, const mr_ray *d_rays,
                          const mr_hit *d_hits, uint64_t n, float max_dist, uint32_t nphotons, uint32_t spp,
                          float *d_scratch, float *d_rgb, void *stream);

/* "mr_gather_level" (declared in miro_hip_surface.h): the same term for ANY queue of the recursion -- the eye rays, or the
 * reflect / Fresnel / refract children of a later level (mr_gen_secondary_rays) -- so that the maps are read at every hit of
 * Scene::traceScene, not at depth 0 only.  Per ray k of the n rays:
 *   query      iff the ray hit and the hit's material is diffuse (Phong::isDiffuse, Phong.cpp:39-42: the clamped m_diffuse of
 *              the material table, also for a TexturedPhong, as the reference tests it)
 *   position   HitInfo::P
 *   normal     d_normal == NULL: the object's normal, normalised (the bits mr_final_gather uses).  d_normal != NULL: three
 *              floats per ray, the normal as Scene::trace hands it on -- the buffer mr_hit_surface writes, bumped on STONE --
 *              read as it is for query rays and never for the others.  On a scene whose texture table holds a procedural
 *              kind (STONE, STEM or a UVW kind) d_normal == NULL is refused: MR_ERR_STATE, call mr_hit_surface first.
 *   value      E = irradiance + caustic, one float add per channel (Scene.cpp:298); with one map that map's estimate; with
 *              none the call is valid and adds nothing.  0 for a ray that is no query.
 * d_weights (rgb per ray, NULL = 1) and d_pixels (pixel per ray, NULL = k / spp) are the queue's, as in mr_shade_lights.
 * Outputs: d_ray_rgb (may be NULL) receives E per ray, un-weighted; d_rgb (may be NULL when d_ray_rgb is given) has
 * E[c] * weight[c] / spp ADDED to the ray's pixel with float atomics, runs of equal pixels summed inside the wave first: the
 * order of the additions is not reproducible, as documented at mr_shade_lights.  d_counts (may be NULL, two uint64, not
 * zeroed by the call): [0] += queries made, [1] += rays seen.
 * d_scratch: 12 * n floats on the device; the layout is part of the contract (miro_hip_surface.h): positions, normals (NaN =
 * no query), the global estimate, the caustic estimate, 3 n floats each, ray k at 3 k -- queries are not compacted.
 * n need not be a multiple of spp; n == 0 is MR_OK and launches nothing.  nphotons in [1, 512].  With device buffers the call
 * only enqueues on `stream` (the query kernel, one estimate per map, the accumulate kernel) and can be captured into a graph.
 * Errors: a NULL scene / rays / hits / scratch or both outputs NULL, spp == 0 (or n / spp beyond 32 bits), nphotons out of range, misaligned buffers
 * (rays / hits 16 bytes, counters 8, floats 4), a map on another device: MR_ERR_INVALID.  A scene that is not built or was
 * built host_only, a map that is not balanced or not resident: MR_ERR_STATE. */

/* ---- photon tracing: Scene::tracePhotons / traceCausticPhotons (Scene.cpp:351-472) for ONE DirectionalAreaLight ----------
 * Emits photons from the disc light and walks each with Scene::tracePhoton (Scene.cpp:529-655), as the serial (non-OpenMP)
 * build does, on the device: one lane per photon, emission -> Scene::trace -> roulette -> store / next segment, in one kernel
 * (csrc/mr_photon_walk.hip).  There is no CPU path.
 *   Emission: power = color * wattage * PI * radius^2 (/ 10 when caustic), direction = normal (as given, not normalised),
 *   origin = position + x * t1 + y * t2, (x, y) from sampleDisc (Utility.h:82-95), t1 / t2 from getTangents (Utility.h:25-31).
 *   Walk: Ray(position + epsilon * direction, direction), Scene::trace(0, MIRO_TMAX); at a hit the cumulative probabilities
 *   prob[0..2] from the averages of the material's kd, ks, kt (the table of mr_scene_set_materials; the white Lambert
 *   without one), one draw rnd: rnd > prob[2] absorbs; rnd < prob[0] is the diffuse event -- the photon is stored from its
 *   second hit on (power, hit.P, incoming direction), a caustic photon whose FIRST hit is diffuse dies, and the walk goes on
 *   along Ray::random with power kd * power / prob[0]; rnd < prob[1] mirrors, rnd < prob[2] transmits (one more draw against
 *   the Fresnel coefficient: reflect or refract); a global (non-caustic) photon whose first event is specular dies.
 *   Directions: the mirror and refraction directions are those of the reference's default build (no -DPATH_TRACING), i.e. of
 *   mr_gen_secondary_rays; the diffuse direction is that of mr_gen_path_rays(kinds = MR_PATH_DIFFUSE) with id = emission
 *   index and bounce = depth.  The Fresnel coefficient, which here DECIDES a branch, is computed on the shared functions of
 *   miro_math.h as mr_gen_path_rays computes it (not on libm's sinf / acosf as mr_gen_secondary_rays does), so that the
 *   decision is the same bits on the device and in a host restatement.
 *   depth counts the photon's hits from 1 (tracePhoton's depth after its increment); a photon walks at most max_depth + 1
 *   segments and stores at most max_depth records (depths 2 ... max_depth + 1).
 * Random numbers: the reference's rand() cannot be reproduced; every draw is the counter-based generator of the eye-ray
 * jitter, H(x) = pcg32(x), u(h) = (h >> 8) / 2^24, keyed by integers (e = emission index, counted from 0 per call):
 *   diffuse direction at depth d   hray = H(H(seed) ^ e) + 4 d;   hk = H(hray + 3);   u1 = u(H(hk)), u2 = u(H(hk ^ 0x68bc21eb))
 *                                  (exactly mr_gen_path_rays' diffuse child for id = e, bounce = d)
 *   roulette draw at depth d       hev = H(H(seed ^ 0x70686f74) ^ e) + 2 d;   rnd = u(H(H(hev)))
 *   Fresnel draw at depth d        u(H(H(hev + 1)))
 *   disc sample, attempt a         hd = H(H(seed ^ 0x64697363) ^ e);   hk = H(hd + a);   x = (2 u(H(hk)) - 1) radius,
 *                                  y = (2 u(H(hk ^ 0x68bc21eb)) - 1) radius; accepted unless x^2 + y^2 > radius^2; after 64
 *                                  rejected attempts (probability 1e-43) the disc's centre is taken
 *   The three seed domains (seed, seed ^ 0x70686f74, seed ^ 0x64697363) keep the event and disc keys apart from the
 *   direction keys of the same bounce.
 * Termination: let s(i) be the number of photons emission i stores.  emitted = the smallest E <= max_emissions with
 *   s(0) + ... + s(E-1) >= target, or max_emissions if there is none (0 when target == 0).  The map receives, through
 *   mr_photon_map_store (photons beyond max_photons are dropped silently), exactly the records of emissions 0 ... E-1,
 *   ordered by emission index and by depth within an emission -- the last emission's records all count, so stored may exceed
 *   target.  The result does not depend on round_emissions or on how the device schedules the photons; only `rounds` does.
 *   Then scale_photon_power(1 / emitted) (Scene.cpp:402).  The call does NOT balance: several lights can be traced into one
 *   map before mr_photon_map_balance.  stored == 0 is MR_OK.
 * d_records (may be NULL): the same records in the same order as a device array, at most records_capacity of them (the rest
 *   are counted in result->stored, never written); powers as stored, before the scaling.
 * The call synchronises `stream` (it copies the records into the map's host store) and returns when the map is filled.
 * Errors: NULL scene / map / desc, max_emissions == 0, radius <= 0, zero or non-finite normal, max_depth > 32, scene and map
 *   on different devices: MR_ERR_INVALID (before any device call); scene not built or host_only, map already balanced:
 *   MR_ERR_STATE.
 *
 * mr_trace_photons_surface -- the same call on the walk of csrc/mr_photon_walk_surface.hip, which looks textures up: emission,
 *   the keys of every draw, termination, records, independence from round_emissions and the errors are exactly those above.
 *   At every hit the colour and the normal are what mr_hit_surface writes for that ray and hit (one device function serves
 *   both): the colour is diffuseColor of Scene.cpp:545-549 for all seven texture kinds and for plain Phong, the normal is
 *   HitInfo::N as Scene::trace leaves it -- bumped on a STONE material, only normalised everywhere else.
 *     roulette       prob[0] = average(colour); prob[1], prob[2] add the averages of the material's ks and kt as above; the
 *                    comparisons are the reference's, literally: rnd > prob[2], rnd < prob[0], rnd < prob[1], rnd < prob[2], so
 *                    a zero, negative or NaN colour falls where those put it
 *     diffuse event  Ray::random about that normal with the keys above; power = (colour * power) * (1 / prob[0])
 *     specular       mirror, Fresnel and refraction use the same normal (a STONE material has ks = kt = 0, so a bumped normal
 *                    only ever reaches Ray::random)
 *     stored         hit.P, the incoming direction, the power before the bounce, as above
 *   Lookups the reference leaves undefined (a petal's large octaves, texels outside an image) take the value the surface pass
 *   defines and are not counted: a count over walked emissions would depend on the round size.
 *   Works on any built, device-resident scene, with or without a texture table; without one, map, records and result are
 *   byte-identical to mr_trace_photons'.  It uploads the table if it changed, as the shading calls do.
 *   mr_trace_photons itself keeps refusing a scene with a texture table (MR_ERR_STATE, naming this call).
 *   mr_trace_photons_timing serves both calls. */
typedef struct mr_disc_light {                        /* DirectionalAreaLight.h:7-38 on SquareLight.h / PointLight.h */
    float position[3], normal[3], color[3], wattage, radius;
} mr_disc_light;
typedef struct mr_photon_trace_desc {
    mr_disc_light light;
    uint32_t target;          /* PhotonsPerLightSource: emit until at least this many photons have been stored */
    uint32_t max_emissions;   /* required > 0: hard stop (the reference loops forever when nothing is ever stored) */
    uint32_t caustic;         /* 0: Scene::tracePhotons; 1: traceCausticPhotons (Scene.cpp:413-472), power / 10 */
    uint32_t seed;
    uint32_t max_depth;       /* 0 = TRACE_DEPTH_PHOTONS (Miro.h:14) = 5; at most 32 */
    uint32_t round_emissions; /* emissions per device round, 0 = chosen by the library (from the yield of the first round);
                                 any value gives the same map and the same emitted / stored / segments */
    uint32_t reserved[6];     /* must be 0 */
} mr_photon_trace_desc;
typedef struct mr_photon_trace_result {
    uint64_t emitted, stored, segments, rounds;   /* segments: Scene::trace calls of emissions 0 ... emitted-1 */
} mr_photon_trace_result;
typedef struct mr_photon_record {                     /* 48 bytes */
    float pos[3], dir[3], power[3];
    uint32_t emission, depth, flags;                  /* flags bit 0: the photon's first bounce was specular */
} mr_photon_record;
mr_status mr_trace_photons(mr_scene *scene, mr_photon_map *map, const mr_photon_trace_desc *desc,
                           mr_photon_trace_result *result, mr_photon_record *d_records, uint64_t records_capacity,
                           void *stream);
/* (the prototype of mr_trace_photons_surface -- the signature above -- is in miro_hip_surface.h, included below) */
/* "mr_trace_photons_resident" (declared in miro_hip_surface.h): either walk with the records kept on the device -- appended
 * round by round to a library-owned buffer instead of copied to the host -- and mr_photon_map_build_device(map, records,
 * stored, 1 / emitted) at the end: the map comes back balanced and resident, byte-identical to mr_trace_photons (or _surface)
 * + mr_photon_map_balance on the same desc.  One EMPTY map per call; several lights into one map stay with the host path.
 * mr_trace_photons_timing reports readback_ms = store_ms = 0 for it. */
/* Where the calling thread's last mr_trace_photons / mr_trace_photons_surface spent its wall time, in milliseconds (any pointer may be NULL): the
 * device rounds (walk + bookkeeping kernels, including the wait for them), the copies of the records, the host store. */
mr_status mr_trace_photons_timing(double *kernel_ms, double *readback_ms, double *store_ms);

const char *mr_last_error(void);
const char *mr_version(void);

#ifdef __cplusplus
}
#endif
#include "miro_hip_surface.h"
#include "miro_hip_frame.h"
#include "miro_hip_render.h"
#endif /* MIRO_HIP_H */
