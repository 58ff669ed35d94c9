// mr_internal.h -- shared declarations of the miro_hip library (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <cstdint>
#include <string>
#include <vector>

#include "miro_hip.h"

namespace mr {

// ---------------------------------------------------------------------------------------
// error plumbing: integer status + thread-local message (no exceptions across the ABI)
// ---------------------------------------------------------------------------------------
mr_status fail(mr_status code, const char *fmt, ...);
#define MR_HIP_CHECK(expr)                                                              \
    do {                                                                                \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess)                                                          \
            return mr::fail(MR_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                 \
                            hipGetErrorString(e__), __FILE__, __LINE__);                \
    } while (0)
// what every call does before its first device work: the two refusals below, then hipSetDevice
//   MR_ERR_HIP      "no HIP device available (...); this library has no CPU fallback"
//   MR_ERR_INVALID  "device %d out of range [0,%d)"
mr_status select_device(int32_t device);

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---------------------------------------------------------------------------------------
// small arithmetic that host and device code share, each written once so that every user gets the same bits
// ---------------------------------------------------------------------------------------
// the counter-based random numbers of the eye-ray jitter, the path and photon lobes, the lens and the square light:
// H(x) = pcg32(x), u(h) = unit01(h) = (h >> 8) / 2^24
__host__ __device__ __forceinline__ uint32_t pcg32(uint32_t x) {
    const uint32_t state = x * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}
__host__ __device__ __forceinline__ float unit01(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

__host__ __device__ __forceinline__ void cross3(const float a[3], const float b[3], float o[3]) {      // Vector3.h cross()
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// getTangents (Utility.h:25-31): alignHemisphereToVector, DirectionalAreaLight and SquareLight::preCalc all call it.  The
// result is built in locals and copied out: inlined into align_to_vector this is the code that function had of its own.
__host__ __device__ __forceinline__ void tangents_of(const float v[3], float t1[3], float t2[3]) {
    const float ez[3] = {0.f, 0.f, 1.f}, ey[3] = {0.f, 1.f, 0.f};
    float a[3], b[3];
    cross3(ez, v, a);
    if ((double)((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) < 1e-6) cross3(ey, v, a);     // float < double literal
    cross3(a, v, b);
    for (int c = 0; c < 3; c++) { t1[c] = a[c]; t2[c] = b[c]; }
}

// ---------------------------------------------------------------------------------------
// host tree, DFS pre-order (what BVH::build produces, BVH.h:29-63)
// ---------------------------------------------------------------------------------------
struct HostNode {
    float lo[3], hi[3];   // padded corners (m_corners[0], m_corners[1])
    int32_t is_leaf;
    int32_t a, b;         // inner: child node indices; leaf: [first, count) into leaf_prims
    int32_t depth;
};

struct HostTree {
    std::vector<HostNode> nodes;
    std::vector<uint32_t> leaf_prims;   // object indices in leaf order
    uint32_t n_leaves = 0, max_depth = 0, leaf_size = 4;
};

// Bounded objects in Scene::addObject order (Scene.h:20-25).  Object i is a triangle with indices vi/ni[3i..3i+2]
// or, when vi[3i] == kSphereSlot, the sphere number vi[3i+1] (a Sphere takes the next object index like any
// triangle would).  Planes are unbounded (Plane.h:27): they never enter the BVH and are scanned after it
// (Scene.cpp:220-230); a hit on plane k reports prim = kPlaneBit | k.
constexpr uint32_t kSphereSlot = 0xFFFFFFFFu;
constexpr uint32_t kPlaneBit = 0x80000000u;
constexpr uint32_t kNoTexcoord = 0xFFFFFFFFu;   // a texture-coordinate index: the triangle's mesh has none (numTextCoords() == 0)
constexpr uint32_t kNoTexture = 0xFFFFFFFFu;    // a material's texture id: plain Phong
constexpr uint32_t kSphereTag = 0x7fc00168u;   // bits of q2.w of a sphere's 48-byte leaf record (a NaN no product yields)

struct HostMesh {
    std::vector<float> v, n;        // xyz triples
    std::vector<uint32_t> vi, ni;   // 3 per object
    std::vector<float> spheres;     // cx, cy, cz, radius
    std::vector<float> planes;      // normal xyz, origin xyz
    std::vector<float> t;           // texture coordinates, uv pairs (TriangleMesh::m_texCoords); empty: no object has any
    std::vector<uint32_t> ti;       // 3 per object, kNoTexcoord in all three = the object's mesh has none; may be shorter than
                                    // vi (objects added without texture coordinates behind the last one that had some)
    std::vector<uint32_t> plane_material;
    uint32_t n_vertices() const { return (uint32_t)(v.size() / 3); }
    uint32_t n_normals() const { return (uint32_t)(n.size() / 3); }
    uint32_t n_triangles() const { return (uint32_t)(vi.size() / 3); }      // objects: triangles + spheres
    uint32_t n_spheres() const { return (uint32_t)(spheres.size() / 4); }
    uint32_t n_planes() const { return (uint32_t)(planes.size() / 6); }
    bool is_sphere(uint32_t obj) const { return !spheres.empty() && vi[3 * (size_t)obj] == kSphereSlot; }
};

// TriangleMesh::load semantics (TriangleMeshLoad.cpp:63-311): appends to `mesh`
mr_status load_obj(const char *path, const float *ctm16, HostMesh &mesh, uint32_t *n_tris);
// BVH::build semantics (BVH.cpp:60-339): identical tree to the reference's
mr_status build_reference_tree(const HostMesh &mesh, uint32_t leaf_size, HostTree &tree);
// the same tree built by kernels (mr_bvh_build.hip; MR_BUILD_REFERENCE_DEVICE), on the current device.  The temporaries are
// freed before it returns.  nonfinite: some coordinate is not finite, found by the object-table kernel -- the tree is not built
// (MR_OK) and the caller builds it on the host.  phases: wall time of the object table (uploads of the raw mesh included), of
// the launches of the 33 depths, and of the numbering and the download.
struct BvhBuildPhases { double prims_ms = 0.0, levels_ms = 0.0, finish_ms = 0.0; };
mr_status build_reference_tree_device(const HostMesh &mesh, uint32_t leaf_size, HostTree &tree, BvhBuildPhases &phases, bool &nonfinite);

// ---------------------------------------------------------------------------------------
// device layout (see DESIGN.md "Data layout in HBM")
// ---------------------------------------------------------------------------------------
// Inner node i = 4 consecutive float4 (one 64-byte record, one cache-line half):
//   q0 = (c0.lo.x, c0.hi.x, c0.lo.y, c0.hi.y)
//   q1 = (c1.lo.x, c1.hi.x, c1.lo.y, c1.hi.y)
//   q2 = (c0.lo.z, c0.hi.z, c1.lo.z, c1.hi.z)
//   q3 = (ref0, ref1, -, -) as int bits
// ref >= 0: inner node index.  ref < 0: leaf, ~ref = (first << 4) | min(count, 15);
// count == 15 means "read leaf_cnt_ext[first]" (only leaves cut off at depth 32 get there).
// Triangle k (leaf order) = 3 consecutive float4 (48 bytes):
//   (A.x, A.y, A.z, BmA.x) (BmA.y, BmA.z, CmA.x, CmA.y) (CmA.z, n.x, n.y, n.z),  n = BmA x CmA
// A sphere's record in the same array: (c.x, c.y, c.z, radius) (0, 0, 0, 0) (0, 0, 0, kSphereTag bits).
// Plane k = 2 float4: (normal.xyz, material id bits) (origin.xyz, 0).
constexpr int kLeafCountBits = 4;
constexpr int kLeafCountMask = 15;
constexpr uint32_t kWorkCounters = 64;   // launches in flight on different streams each get their own counter
constexpr uint64_t kStageChunk = 1ull << 20;   // rays per chunk of a pipelined host-pointer trace (32 MiB up, 16 MiB down)

struct DeviceScene {
    float4   *nodes = nullptr;         // 4 * n_inner
    float4   *tris = nullptr;          // 3 * n_triangles (leaf order)
    uint32_t *tri_prim = nullptr;      // leaf order -> prim id
    uint32_t *leaf_cnt_ext = nullptr;  // leaf order position -> count (for count >= 15)
    // original indexed mesh, for HitInfo reconstruction and shadow-ray origins
    float    *v = nullptr, *n = nullptr;
    uint32_t *vi = nullptr, *ni = nullptr;
    // materials (11 floats each: diffuse, specular, transmission, shininess, refraction index) and the material of
    // every triangle; prim_material == nullptr means material 0 everywhere
    float    *materials = nullptr;
    uint32_t *prim_material = nullptr;
    uint32_t user_materials = 0;       // mr_scene_set_materials was called (otherwise `materials` is the one white Lambert)
    uint32_t refractive = 0;           // some material has a positive transmission component (Phong::isRefractive)
    float4   *spheres = nullptr;       // (c.xyz, radius) per sphere; nullptr when the scene has none
    float4   *planes = nullptr;        // 2 per plane; nullptr when the scene has none
    uint32_t n_spheres = 0, n_planes = 0;
    // texture coordinates (mr_uv.h): uv pairs and three indices per object; both nullptr when no object has any
    float    *texcoords = nullptr;
    uint32_t *ti = nullptr;
    float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};
    int32_t root_ref = 0;
    uint32_t n_inner = 0, n_tris = 0, stack_depth = 1;
    uint64_t bytes = 0;
};

struct TraceParams {
    const float4   *nodes;
    const float4   *tris;
    const uint32_t *tri_prim;
    const uint32_t *leaf_cnt_ext;
    float root_lo[3], root_hi[3];
    int32_t root_ref;
    int32_t stack_depth;
    const mr_ray *rays;
    mr_hit *hits;
    unsigned long long n;                 // number of rays (upper bound when n_dev is set)
    const unsigned long long *n_dev;      // optional device-resident ray count (mr_trace_indirect)
    unsigned long long *stats;   // [0] box tests, [1] triangle tests (MR_COUNT_STATS)
    const float4 *planes;                 // unbounded objects, scanned after the BVH (Scene.cpp:220-230)
    uint32_t n_planes, n_spheres;
    unsigned long long *work_counter;     // zeroed per launch: ray hand-out counter of the persistent kernel
    const uint32_t *order;                // optional: lane k traces ray order[k] (and writes hits[order[k]]): mr_trace_grouped
};

mr_status launch_trace(const TraceParams &p, uint32_t flags, hipStream_t stream);
// order[] = the batch's ray indices, grouped by direction octant inside consecutive chunks of 2^chunk_log2 rays (mr_kernels.hip)
mr_status launch_octant_order(const mr_ray *d_rays, const uint8_t *d_octants, unsigned long long n, uint32_t chunk_log2, uint32_t *d_order, hipStream_t stream);
mr_status launch_eye_rays(const mr_camera &cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1,
                          uint32_t spp, uint32_t jitter, uint32_t seed, bool tiled, mr_ray *d_rays, hipStream_t stream);
mr_status launch_shadow_rays(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits,
                             unsigned long long n, const float light[3], mr_ray *d_out, uint32_t *d_src,
                             unsigned long long *d_count, hipStream_t stream);
mr_status launch_hit_attrs(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, unsigned long long n,
                           float *d_P, float *d_N, hipStream_t stream);

mr_status launch_shade(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, unsigned long long n,
                       const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src, const unsigned long long *d_shadow_count,
                       uint8_t *d_occluded, const mr_light &light, const float diffuse[3], uint32_t spp, float *d_rgb,
                       hipStream_t stream);
// The photon-map term (Scene.cpp:285-299).  One query kernel (mr_gather_level.hip) serves mr_final_gather and mr_gather_level:
// hit point and normal of the diffuse hits, a NaN normal elsewhere; d_normal NULL or the surface pass's normals; d_counts NULL
// or [0] += queries, [1] += rays.  Two accumulate kernels, because their sums round differently: mr_final_gather's
// (mr_shade.hip) adds a pixel's samples in sample order and then one float to the pixel; mr_gather_level's takes per-ray
// weights and pixels and adds wave runs with float atomics.
mr_status launch_gather_accumulate(const float *d_irr_a, const float *d_irr_b, unsigned long long n, uint32_t spp,
                                   float *d_rgb, hipStream_t stream);
mr_status launch_gather_level_queries(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                                      unsigned long long n, float *d_pos, float *d_nrm, unsigned long long *d_counts,
                                      hipStream_t stream);
mr_status launch_gather_level_accumulate(const float *d_irr_a, const float *d_irr_b, const float *d_weights, const uint32_t *d_pixels,
                                         unsigned long long n, uint32_t spp, float *d_rgb, float *d_ray_rgb, hipStream_t stream);
mr_status launch_tonemap(const float *d_rgb, unsigned long long n_values, uint8_t *d_out, hipStream_t stream);
// mr_finish_image (mr_finish_image.hip): two kernels on `stream`.  d_state: three words owned by the scene -- the order-preserving
// integer images of the running maximum and minimum and a ticket --, which hold finish_state_identity() between calls: the second
// kernel's last workgroup puts that back.  d_minmax: optional, (max, min) for the caller
constexpr uint32_t kFinishMaxIdentity = 0x007FFFFFu, kFinishMinIdentity = 0xFF800000u;   // the images of -inf and +inf
mr_status launch_finish_image(const float *d_rgb, unsigned long long n_values, uint8_t *d_out, float *d_minmax, uint32_t *d_state,
                              hipStream_t stream);
mr_status launch_deinterleave(const float *d_recv, float *d_full, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t world,
                              uint32_t shard_rows, uint32_t fpp, hipStream_t stream);
mr_status launch_untile(const float *d_slots, float *d_image, uint32_t W, uint32_t rows, uint32_t spp, uint32_t channels,
                        hipStream_t stream);

// the fused direct-light frame (mr_frame.hip)
// The eye-relative tables of the fused frame (mr_frame.hip: eye_tables), per scene: up to kWorkCounters sets, each built for
// one eye.  A call whose eye a set already holds uses it as it is; otherwise it rebuilds the least recently used set -- whose
// last user is at least kWorkCounters calls back, so finished by the contract of mr_render_direct (miro_hip.h).  A set built
// inside a graph capture is rebuilt by every replay of the graph, whenever that is: from then on it is never taken as holding
// any eye (every call that picks it rebuilds it).
struct EyeTables {
    float4 *d = nullptr;          // n_inner node records of 64 bytes, then n_tris triangle records of 48 (eye_table_bytes)
    float eye[3] = {0.f, 0.f, 0.f};
    bool reusable = false;        // holds the tables of `eye` (built outside a capture)
    bool captured = false;        // a captured graph rebuilds it
    uint64_t last_use = 0;        // pool call number of its last user, 0 = never used
    void *ready = nullptr;        // hipEvent_t recorded after its build, on the stream it was built on
    void *stream = nullptr;
};
struct EyeTablePool {
    std::mutex mu;
    EyeTables set[kWorkCounters];
    uint64_t calls = 0;
};
inline size_t eye_table_bytes(const DeviceScene &ds) {
    const size_t b = (size_t)ds.n_inner * 64 + (size_t)ds.n_tris * 48;
    return b ? b : 64;
}
mr_status launch_frame_b256(const DeviceScene &ds, const mr_frame_desc &fd, float *d_rgb, mr_hit *d_hits, mr_hit *d_shadow_hits,
                            unsigned long long *d_counts, unsigned long long *work_counter, EyeTablePool &eye_pool, hipStream_t stream);
mr_status launch_frame_b128(const DeviceScene &ds, const mr_frame_desc &fd, float *d_rgb, mr_hit *d_hits, mr_hit *d_shadow_hits,
                            unsigned long long *d_counts, unsigned long long *work_counter, EyeTablePool &eye_pool, hipStream_t stream);
// mr_frame.hip in its two workgroup sizes: frames of up to ~10 M samples (1080p at 4 spp) in 128-thread workgroups
inline mr_status launch_frame(const DeviceScene &ds, const mr_frame_desc &fd, float *d_rgb, mr_hit *d_hits, mr_hit *d_shadow_hits,
                              unsigned long long *d_counts, unsigned long long *work_counter, EyeTablePool &eye_pool, hipStream_t stream) {
    const unsigned long long rows = fd.band_world > 1 ? (fd.H + fd.band_world - 1) / fd.band_world : (fd.y1 > fd.y0 ? fd.y1 - fd.y0 : 0);
    const unsigned long long samples = rows * fd.W * fd.spp;
    return samples <= 10000000ull ? launch_frame_b128(ds, fd, d_rgb, d_hits, d_shadow_hits, d_counts, work_counter, eye_pool, stream)
                                  : launch_frame_b256(ds, fd, d_rgb, d_hits, d_shadow_hits, d_counts, work_counter, eye_pool, stream);
}

// tex: the scene's texture table (below), or NULL for the untextured kernel
struct TexParams;
mr_status launch_shade_accumulate(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                  const uint32_t *d_pixels, unsigned long long n, const mr_ray *d_shadow_rays,
                                  const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src,
                                  const unsigned long long *d_shadow_count, float *d_light_scale, const mr_light &light,
                                  uint32_t spp, float *d_rgb, const TexParams *tex, hipStream_t stream);
mr_status launch_secondary_rays(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                const uint32_t *d_pixels, unsigned long long n, uint32_t spp, mr_ray *d_out_rays,
                                float *d_out_weights, uint32_t *d_out_pixels, unsigned long long *d_count,
                                unsigned long long out_capacity, uint8_t *d_out_octants, hipStream_t stream);

// ... with every hit's N read from the surface pass's normal buffer (mr_bump_surface.hip, mr_gen_secondary_rays_surface)
mr_status launch_secondary_rays_surface(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                                        const float *d_weights, const uint32_t *d_pixels, unsigned long long n, uint32_t spp,
                                        mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels, unsigned long long *d_count,
                                        unsigned long long out_capacity, uint8_t *d_out_octants, hipStream_t stream);

// PATH_TRACING generators (mr_bounce.hip): kinds bit 0 mirror, 1 refraction pair, 2 diffuse bounce
mr_status launch_path_rays(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                           const uint32_t *d_pixels, const uint32_t *d_ids, unsigned long long n, uint32_t spp, uint32_t seed,
                           uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                           uint32_t *d_out_ids, unsigned long long *d_count, unsigned long long out_capacity, uint8_t *d_out_octants, hipStream_t stream);
// ... with every hit's N and the diffuse child's colour read from the surface pass's buffers (mr_path_surface.hip)
mr_status launch_path_rays_surface(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                   const float *d_normal, const float *d_weights, const uint32_t *d_pixels, const uint32_t *d_ids,
                                   unsigned long long n, uint32_t spp, uint32_t seed, uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays,
                                   float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids, unsigned long long *d_count,
                                   unsigned long long out_capacity, uint8_t *d_out_octants, hipStream_t stream);

mr_status launch_level(const DeviceScene &ds, const mr_level_desc &ld, const mr_ray *d_rays, const float *d_weights,
                       const uint32_t *d_pixels, const uint32_t *d_ids, unsigned long long n, float *d_rgb, mr_ray *d_out_rays,
                       float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids, unsigned long long *d_out_count,
                       unsigned long long *d_counts, hipStream_t stream);

// Phong::shade over the scene's light list (mr_lights.hip): a light of mr_scene_set_lights as the kernel takes it (the
// list travels in the kernel arguments).  normal / radius: MR_LIGHT_DISC only.
struct ShadeLight {
    uint32_t kind;
    float position[3], normal[3], color[3], wattage, radius;
};
mr_status launch_shade_lights(const DeviceScene &ds, const ShadeLight *lights, uint32_t n_lights, const mr_ray *d_rays,
                              const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels, unsigned long long n,
                              uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts,
                              hipStream_t stream);
// the fused frame over the light list (mr_frame_lights.hip, mr_render_lights).  fd: band_world >= 1 (as mr_render_direct hands it
// to launch_frame).  check_frame_lights: what the descriptor alone can get wrong (spp, bands, rows, size, flags), without a
// device call or a look at any scene, `who` the entry point its messages name; launch_frame_lights: one kernel on `stream`,
// none for an empty window
mr_status check_frame_lights(const char *who, const mr_frame_desc &fd);
mr_status launch_frame_lights(const DeviceScene &ds, const ShadeLight *lights, uint32_t n_lights, const mr_frame_desc &fd, float *d_rgb,
                              mr_hit *d_hits, float *d_sample_rgb, unsigned long long *d_counts, hipStream_t stream);
// ... on any scene (mr_frame_lights_surface.hip, mr_render_lights_surface): every hit's diffuse colour and normal from
// hit_color_normal between the primary trace and the light loop.  tex: as mr_hit_surface hands it to launch_hit_surface
// (recs / mat_tex nullptr without a texture table); o (FrameOutputs, below): sample_color / sample_normal optional; counts: three words
struct LightScene;
struct FrameOutputs;
mr_status launch_frame_lights_surface(const LightScene &ls, const mr_frame_desc &fd, const FrameOutputs &o, hipStream_t stream);
// ... with the environment for rays that miss (mr_frame_lights_env.hip, mr_render_lights_environment): a live sample whose
// primary ray misses is worth ls.env.bg, or the lookup of the full image (ls.env.full); o.counts: five words
mr_status launch_frame_lights_env(const LightScene &ls, const mr_frame_desc &fd, const FrameOutputs &o, hipStream_t stream);
// *d_count = 0 on `stream`, as a one-word kernel: the node that zeroes d_out_count in the three launchers below, which a captured
// graph replays as written (mr_level_lights.hip says what a memset node did)
mr_status launch_zero_count(unsigned long long *d_count, hipStream_t stream);
// one level of the recursion over the light list on any scene (mr_level_lights.hip, mr_trace_level_lights): launch_level's queues
// with that frame's texture table, environment (read with ld.environment only) and optional per-ray outputs; d_out_count is
// zeroed on `stream` on a level with children (a one-word kernel), then one kernel (none for n == 0); d_counts: five words
mr_status launch_level_lights(const LightScene &ls, const mr_level_lights_desc &ld, const mr_ray *d_rays, const float *d_weights,
                              const uint32_t *d_pixels, unsigned long long n, float *d_rgb, mr_hit *d_hits, float *d_ray_rgb,
                              float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                              unsigned long long *d_out_count, unsigned long long *d_counts, hipStream_t stream);
// ... with specular children on a scene whose reflective STONE material bump-maps the mirror direction (ls.bumped_specular;
// mr_level_lights_bump.hip): launch_level_lights hands a level with children on such a scene on to this one, which zeroes
// d_out_count and launches level_lights_body's BUMPED form -- the children bounce about the surface step's normal
mr_status launch_level_lights_bumped(const LightScene &ls, const mr_level_lights_desc &ld, const mr_ray *d_rays, const float *d_weights,
                                     const uint32_t *d_pixels, unsigned long long n, float *d_rgb, mr_hit *d_hits, float *d_ray_rgb,
                                     float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                                     unsigned long long *d_out_count, unsigned long long *d_counts, hipStream_t stream);
// ... of a PATH_TRACING build (mr_level_lights_path.hip, mr_trace_level_lights_path): the same level with the children of
// mr_gen_path_rays_surface (ids in and out, ld.path_kinds / seed / bounce), the low-res environment image for the rays that
// ld.d_lowres or MR_ENV_LOWRES names, and ld.d_out_lowres for the next level
mr_status launch_level_lights_path(const LightScene &ls, const mr_level_lights_path_desc &ld, const mr_ray *d_rays, const float *d_weights,
                                   const uint32_t *d_pixels, const uint32_t *d_ids, unsigned long long n, float *d_rgb, mr_hit *d_hits,
                                   float *d_ray_rgb, float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights,
                                   uint32_t *d_out_pixels, uint32_t *d_out_ids, unsigned long long *d_out_count,
                                   unsigned long long *d_counts, hipStream_t stream);
// A queue of rays between two levels, array by array: what a level with children writes and the next level reads.  ids: the path
// tracer's stable ray ids, low: its byte per ray that says whether Ray::random made the ray; nullptr where the queue has none
struct RayQueue {
    mr_ray *rays;
    float *weights;
    uint32_t *pixels, *ids;
    uint8_t *low;
};
// What a light-list frame on any scene writes: the pixels; per sample, each optional, the primary hit record, the un-weighted L,
// the hit's diffuseColor and the normal Scene::trace hands on; the launch's counters (optional)
struct FrameOutputs {
    float *rgb;
    mr_hit *hits;
    float *sample_rgb, *sample_color, *sample_normal;
    unsigned long long *counts;
};
// the capacity of the output queue as a level's descriptor spells it (mr_level_lights_desc, mr_level_lights_path_desc, mr_frame_level_desc)
template <typename DESC>
unsigned long long out_capacity_of(const DESC &ld) { return ((unsigned long long)ld.out_capacity_hi << 32) | ld.out_capacity_lo; }
// the level-0 frame that also emits the rays of level 1 (mr_frame_level_lights.hip, mr_render_level_lights): launch_frame_lights_env's
// frame (env all zero: a miss is worth 0) with the children of launch_level_lights (ld.children == MR_LEVEL_SPECULAR) or
// launch_level_lights_path (MR_LEVEL_PATH; bounce 0, ids = sample indices) for rays that start at the eye with weight 1 and pixel
// row * W + x, written to `out` (out.low takes the place of ld.d_out_lowres, which is not read); d_out_count is zeroed on `stream`
// (a one-word kernel), then one kernel (none for an empty window).
// frame_level_lights_samples: the samples of fd's window, from the descriptor alone (no device call)
mr_status frame_level_lights_samples(const char *who, const mr_frame_desc &fd, unsigned long long &n);
mr_status launch_frame_level_lights(const LightScene &ls, const mr_frame_desc &fd, const mr_frame_level_desc &ld, const FrameOutputs &o,
                                    const RayQueue &out, unsigned long long *d_out_count, hipStream_t stream);
// ... for the thin-lens camera (mr_frame_lens.hip, mr_render_level_lights_lens): the eye ray of a sample is the one
// launch_eye_rays_lens makes for it without caller-supplied samples.  ld.children == MR_LEVEL_LAST launches the frame without
// children and touches neither `out` nor d_out_count.  `who`: the entry point the window's messages name
mr_status launch_frame_lens(const char *who, const LightScene &ls, const mr_frame_desc &fd, const mr_lens_desc &lens, const mr_frame_level_desc &ld,
                            const FrameOutputs &o, const RayQueue &out, unsigned long long *d_out_count, hipStream_t stream);
// One pass of a frame of S samples per pixel (mr_frame_passes.hip, mr_render_recursion_passes): the launch renders samples
// [base, base + fd.spp) of every pixel, numbered as a single launch at spp = S would number them (keys, path hashes, child ids);
// a pixel's value is its lanes' sum / S, stored by the pass with base == 0 and added by every other.  lens: optional.  Otherwise
// launch_frame_lens' contract, MR_LEVEL_LAST included.
struct FramePass { uint32_t S, base; };
mr_status launch_frame_pass(const char *who, const LightScene &ls, const mr_frame_desc &fd, const mr_lens_desc *lens, const mr_frame_level_desc &ld,
                            const FramePass &pass, const FrameOutputs &o, const RayQueue &out, unsigned long long *d_out_count,
                            hipStream_t stream);
// One level of mr_render_recursion, whose queue's length is a device word (mr_level_lights_queued.hip).  What the level is:
// path: the PATH_TRACING build's kernel (children of bounce `bounce` from path_kinds / seed, ids, low-res bytes), else the
// specular one; last: no children; capacity: the rays the output queue holds
struct QueuedLevel {
    uint32_t spp, flags;
    bool last, path;
    uint32_t environment, path_kinds, seed, bounce;
    unsigned long long capacity;
};
// `in` holds min(*d_n, n_cap) rays, read by the kernel; the grid is level_lights_queued_grid(n_cap, n_bound) workgroups, n_bound
// being what the host knows the length cannot exceed, and workgroups beyond the length leave at once.  Per-ray outputs besides
// the pixels: d_hits and d_normal, both optional (the photon-map term of mr_render_recursion_photons reads them).  row: the
// level's eight counters -- [0 .. 5) as launch_level_lights' d_counts, [5] += children into `out`, stored or not, and NOT zeroed
// here (launch_zero_words: d_words[0 .. n) = 0 on `stream`, as a kernel); ONE kernel, also for an empty queue
unsigned level_lights_queued_grid(unsigned long long n_cap, unsigned long long n_bound);
mr_status launch_zero_words(unsigned long long *d_words, unsigned long long n, hipStream_t stream);
mr_status launch_level_lights_queued(const LightScene &ls, const QueuedLevel &lv, const RayQueue &in, const RayQueue &out,
                                     const unsigned long long *d_n, unsigned long long n_cap, unsigned long long n_bound, float *d_rgb,
                                     mr_hit *d_hits, float *d_normal, unsigned long long *row, hipStream_t stream);
// ... its specular level with children on a scene with ls.bumped_specular (mr_level_lights_queued_bump.hip), to which
// launch_level_lights_queued hands such a level on: the BUMPED form of the same kernel, the same grid
mr_status launch_level_lights_queued_bumped(const LightScene &ls, const QueuedLevel &lv, const RayQueue &in, const RayQueue &out,
                                            const unsigned long long *d_n, unsigned long long n_cap, unsigned long long n_bound, float *d_rgb,
                                            mr_hit *d_hits, float *d_normal, unsigned long long *row, hipStream_t stream);

// the thin-lens camera and Phong::shade over SquareLights (mr_distribution.hip).  side: the sample cells along an edge of a
// square light, side * side shadow rays per hit and light
mr_status launch_eye_rays_lens(const mr_camera &cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t spp, uint32_t jitter,
                               uint32_t seed, const mr_lens_desc &lens, const float *d_samples_in, float *d_samples_out,
                               unsigned long long *d_counts, mr_ray *d_rays, hipStream_t stream);
mr_status launch_shade_square_lights(const DeviceScene &ds, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t side,
                                     uint32_t seed, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                     const uint32_t *d_pixels, const float *d_uv_in, unsigned long long n, uint32_t spp, uint32_t flags,
                                     float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts, hipStream_t stream);
// ... with the hit's diffuse colour and normal read from the surface pass's buffers (mr_square_surface.hip)
mr_status launch_shade_square_lights_surface(const DeviceScene &ds, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t side,
                                             uint32_t seed, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                             const float *d_normal, const float *d_weights, const uint32_t *d_pixels, const float *d_uv_in,
                                             unsigned long long n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb,
                                             unsigned long long *d_counts, hipStream_t stream);

// 2-D textures of TexturedPhong materials (mr_textures.hip; Texture.h:112-133, Texture.cpp:23-28,131-185, Phong.cpp:51-56).  The
// host copy is one blob as the device holds it: three float4 per texture (TexParams below), then the texels of the
// image textures as 16-byte records (r, g, b, 0) like the environment's, then one texture id per material.
struct HostTextures {
    uint32_t n_textures = 0, n_materials = 0;
    size_t texel_base = 0, mat_base = 0;       // offsets into blob, in float4
    std::vector<float4> blob;                  // empty: the scene has no texture table
    bool procedural = false;                   // some texture is a STONE, a STEM or a UVW kind: only the _surface calls shade such a scene
    bool bumped_specular = false;              // some material names a STONE texture and has ks != 0: its mirror child bounces about
                                               // the bumped normal, which only the surface pass (or a fused surface step) has
};
struct TexParams {                             // the table as the kernels take it
    const float4 *recs;                        // 3 per texture: (kind, W, H, first texel as bits) (color1 | max_intensity, hdr) (color2)
                                               // STONE / STEM: (kind, 0, 0, 0) (0, 0, 0, scale) (0): scale where a checker's is
                                               // PETAL / LEAF / FLOWER_CENTER: (kind, 0, 0, 0) (pivot, scale) (radius, 0, 0, 0)
    const float4 *texels;
    const uint32_t *mat_tex;                   // per material: texture id or kNoTexture
    const float *texcoords;                    // the scene's texture coordinates (mr_uv.h), nullptr: none
    const uint32_t *ti;
};
// the textured forms of shade_lights_kernel / shade_accumulate_kernel and the two inspection kernels (mr_textures.hip)
mr_status launch_shade_lights_tex(const DeviceScene &ds, const TexParams &tex, const ShadeLight *lights, uint32_t n_lights,
                                  const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels,
                                  unsigned long long n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb,
                                  unsigned long long *d_counts, hipStream_t stream);
mr_status launch_shade_accumulate_tex(const DeviceScene &ds, const TexParams &tex, const mr_ray *d_rays, const mr_hit *d_hits,
                                      const float *d_weights, const uint32_t *d_pixels, unsigned long long n,
                                      const float *d_light_scale, const mr_light &light, uint32_t spp, float *d_rgb,
                                      hipStream_t stream);
mr_status launch_hit_uv(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, unsigned long long n, float *d_uv,
                        hipStream_t stream);
mr_status launch_texture_lookup(const TexParams &tex, uint32_t texture, const float *d_uv, unsigned long long n, float *d_rgb,
                                unsigned long long *d_counts, hipStream_t stream);

// Procedural and UVW textures and bump-mapped normals (mr_procedural.hip): the per-hit surface pass of every scene, the
// light-list and accumulate kernels that read its two buffers, and the inspection kernels (launch_texture_lookup3: lookup3D of
// one UVW texture at d_p).  launch_hit_surface takes a TexParams whose recs / mat_tex are nullptr for a scene without a
// texture table.
mr_status launch_hit_surface(const DeviceScene &ds, const TexParams &tex, const mr_ray *d_rays, const mr_hit *d_hits, unsigned long long n,
                             float *d_color, float *d_normal, unsigned long long *d_counts, hipStream_t stream);
mr_status launch_shade_lights_surf(const DeviceScene &ds, const ShadeLight *lights, uint32_t n_lights, const mr_ray *d_rays,
                                   const mr_hit *d_hits, const float *d_color, const float *d_normal, const float *d_weights,
                                   const uint32_t *d_pixels, unsigned long long n, uint32_t spp, uint32_t flags, float *d_rgb,
                                   float *d_ray_rgb, unsigned long long *d_counts, hipStream_t stream);
mr_status launch_shade_accumulate_surf(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                       const float *d_normal, const float *d_weights, const uint32_t *d_pixels, unsigned long long n,
                                       const float *d_light_scale, const mr_light &light, uint32_t spp, float *d_rgb, hipStream_t stream);
mr_status launch_texture_lookup_proc(const TexParams &tex, uint32_t texture, const float *d_uv, unsigned long long n, float *d_rgb,
                                     unsigned long long *d_counts, hipStream_t stream);
mr_status launch_bump_height(bool stone, float scale, const float *d_uv, unsigned long long n, float *d_height, hipStream_t stream);
mr_status launch_noise_probe(uint32_t which, const float *d_in, unsigned long long n, float *d_out, hipStream_t stream);
mr_status launch_texture_lookup3(const TexParams &tex, uint32_t texture, const float *d_p, unsigned long long n, float *d_rgb,
                                 float *d_coords, unsigned long long *d_counts, hipStream_t stream);
// the first half of launch_shade_accumulate (mr_bounce.hip): Phong.cpp:97-113's light scale per ray from the traced shadow rays
mr_status launch_light_scale(const DeviceScene &ds, const mr_ray *d_shadow_rays, const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src,
                             const unsigned long long *d_shadow_count, unsigned long long n, float *d_light_scale, hipStream_t stream);

// The environment of rays that miss (mr_environment.hip; Scene::getEnvironmentMap, Scene.cpp:657-688).  The host copy is what
// mr_scene_set_environment made of the caller's image (LoadedTexture::LoadedTexture, Texture.cpp:30-92); the device copy holds
// one 16-byte record (r, g, b, 0) per texel, full image then low-res image, so that a texel fetch is one dwordx4.
struct HostEnvironment {
    float bg[3] = {0.f, 0.f, 0.f};
    float rot[2] = {0.f, 0.f};
    uint32_t W = 0, H = 0, lw = 0, lh = 0;     // W == 0: no image (m_environment = 0)
    float max_intensity = 0.f;
    std::vector<float> rec;                    // (r, g, b, 0) per texel: W * H of the image, then lw * lh of the low-res image
                                               // as setPixel stored it (green and blue exchanged); what the device copy holds
};
struct EnvParams {                             // the environment as the kernel takes it
    const float4 *full, *low;                  // nullptr: colour only
    uint32_t W, H, lw, lh;
    float rot[2], max_intensity, bg[3];
};
constexpr uint32_t kEnvLowresWidth = 24;       // LoadedTexture::LOWRES_WIDTH (Texture.h:297)
constexpr uint32_t kEnvMaxLowresHeight = 96;   // H <= 4 W: the low-res image (at most 36 KB) is staged in LDS
mr_status launch_shade_environment(const EnvParams &env, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                   const uint32_t *d_pixels, const uint8_t *d_lowres, unsigned long long n, uint32_t spp,
                                   uint32_t flags, float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts, hipStream_t stream);

// What every light-list launch reads from the scene (lights_scene_params, mr_api.cpp): the device arrays, the texture table or
// none, the environment (all zero where the call has none) and the light list.  Made for ONE API call and not kept: ds and lights
// point into the mr_scene (s->dev, s->lights), which the next mr_scene_set_* call may change
struct LightScene {
    const DeviceScene *ds;
    TexParams tex;
    EnvParams env;
    const ShadeLight *lights;
    uint32_t n_lights;
    bool bumped_specular = false;              // HostTextures::bumped_specular: the specular level kernels take their BUMPED form
};

// photon map on the device: three float4 planes in kd-tree heap order, 1-based (children of i: 2i, 2i+1)
struct PhotonMapDev {
    float4 *rec = nullptr;        // two per photon, one 32-byte record: (x, y, z, split axis as int bits), then the incoming
                                  // direction de-quantised through the reference's tables -- both halves in one cache line for the
                                  // divergent fetches of the reference-order pre-pass
    float4 *power = nullptr;      // (r, g, b, -)
    int32_t n = 0, half = 0;      // stored photons; nodes with index < half descend (PhotonMap.cpp:160,357)
    // Bounding boxes of the tree's BLOCKS (the 63 nodes of six levels below a block root r = 64^L + i, L = 0 .. layers - 1):
    // four float4 per block id = layer_base[L] + i: (lo, hi) of the block's own 63 photons, (lo, hi) of every photon below
    // its root.  The cooperative search finds the blocks that touch the search sphere with these instead of walking planes.
    float4 *boxes = nullptr;
    int32_t layers = 0, layer_base[4] = {0, 0, 0, 0};
    // hand-out counters of the estimate launches (mr_photon.hip): zero between launches, one per launch in flight
    unsigned *work_counters = nullptr;
};
constexpr uint32_t kPhotonWorkCounters = 16;
// n, half, layers and layer_base of a balanced map of n photons; returns the number of its block boxes (the boxes plane holds
// four float4 for each, and for one when there is none)
inline size_t photon_map_layout(PhotonMapDev &dev, uint32_t n) {
    dev.n = (int32_t)n;
    dev.half = (int32_t)n / 2 - 1;                                  // half_stored_photons, PhotonMap.cpp:357
    dev.layers = 0;
    size_t total = 0;
    for (uint64_t first = 1; first <= n && dev.layers < 4; first <<= 6) { dev.layer_base[dev.layers++] = (int32_t)total; total += (size_t)first; }
    return total;
}
constexpr int kKnnMaxK = 512;     // nphotons limit of the wave-cooperative k-NN (PHOTON_SAMPLES = 500)
mr_status launch_irradiance(const PhotonMapDev &pm, unsigned *work_counter, const float *d_pos, const float *d_normal, unsigned long long nq,
                            float max_dist, uint32_t k, float *d_irrad, int32_t *d_found, float *d_r2, unsigned long long *d_stats,
                            hipStream_t stream);
constexpr int kPhotonStats = 12;  // see mr_photon_map_get_stats (miro_hip.h)
// The photon-map term for a queue whose length is a device word (mr_gather_queued.hip, mr_render_recursion_photons): the three
// steps of mr_gather_level as kernels that read n = min(*d_n, bound) themselves.  bound: what the host knows the length cannot
// exceed, at most the queue's capacity -- every grid is sized from it and every buffer holds that many rays; nothing is launched
// where it is 0.  launch_gather_queued_accumulate: spp finds the pixel of a level-0 sample (k / spp, d_pixels NULL), spp_total is the
// divisor -- the same number except in a pass of a longer frame (mr_render_recursion_photons_passes).  d_queries: one word, += the queries made.  launch_gather_eye_queries: level 0 of the one-call frame, whose rays
// exist in registers only -- the eye ray of sample k of fd's window is made again and joined with the hit record (and, given
// d_normal, the normal) the frame wrote.
mr_status launch_gather_eye_queries(const DeviceScene &ds, const char *who, const mr_frame_desc &fd, const mr_hit *d_hits,
                                    const float *d_normal, float *d_pos, float *d_nrm, unsigned long long *d_queries, hipStream_t stream);
// ... of the lens frame (mr_frame_lens.hip): the lens ray of sample k made again
mr_status launch_gather_eye_queries_lens(const DeviceScene &ds, const char *who, const mr_frame_desc &fd, const mr_lens_desc &lens,
                                         const mr_hit *d_hits, const float *d_normal, float *d_pos, float *d_nrm,
                                         unsigned long long *d_queries, hipStream_t stream);
mr_status launch_gather_queued_queries(const DeviceScene &ds, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                                       const unsigned long long *d_n, unsigned long long bound, float *d_pos, float *d_nrm,
                                       unsigned long long *d_queries, hipStream_t stream);
mr_status launch_irradiance_queued(const PhotonMapDev &pm, unsigned *work_counter, const float *d_pos, const float *d_normal,
                                   const unsigned long long *d_n, unsigned long long bound, float max_dist, uint32_t k, float *d_irrad,
                                   unsigned long long *d_stats, hipStream_t stream);
mr_status launch_gather_queued_accumulate(const float *d_irr_a, const float *d_irr_b, const float *d_weights, const uint32_t *d_pixels,
                                          const unsigned long long *d_n, unsigned long long bound, uint32_t spp, uint32_t spp_total,
                                          float *d_rgb, hipStream_t stream);
// ... level 0 of one pass (mr_frame_passes.hip): the ray of sample pass.base + k % fd.spp made again, through `lens` if given
mr_status launch_gather_eye_queries_pass(const DeviceScene &ds, const char *who, const mr_frame_desc &fd, const mr_lens_desc *lens,
                                         const FramePass &pass, const mr_hit *d_hits, const float *d_normal, float *d_pos, float *d_nrm,
                                         unsigned long long *d_queries, hipStream_t stream);
// The scratch of the photon-map term for n rays (mr_gather_level's d_scratch, 12 n floats): positions, normals (NaN = no query),
// then the global map's estimate and the caustic map's; irr[i]: nullptr without map i
struct GatherScratch { float *pos, *nrm, *irr[2]; };
inline GatherScratch gather_scratch(float *d_scratch, unsigned long long n, bool global_map, bool caustic_map) {
    return {d_scratch, d_scratch + 3 * n, {global_map ? d_scratch + 6 * n : nullptr, caustic_map ? d_scratch + 9 * n : nullptr}};
}

// photon tracing (mr_photon_walk.hip): one round = emissions first ... first + count - 1 of one light, walked to their end
struct PhotonWalkLight {
    float position[3], direction[3], t1[3], t2[3];   // getTangents of the normal (Utility.h:25-31), computed on the host
    float power[3], radius;                          // the emitted power (Scene.cpp:380-385 / :442-447)
};
struct PhotonRoundHeader {
    uint32_t emitted;             // emissions of the round that count: up to and including the one that reaches the target
    uint32_t reached;             // the running total reached the target inside this round
    unsigned long long stored, segments;   // over those emissions
};
struct PhotonRoundBuffers {
    float4 *slots = nullptr;      // capacity * max_depth records of three float4 (mr_photon_record), written by the walk
    float4 *compact = nullptr;    // the same size: the round's records in emission order
    uint32_t *words = nullptr;    // per emission: stores | segments << 8
    uint32_t *offsets = nullptr;  // per emission: records of the round in front of its own
    unsigned *next = nullptr;     // the round's emission counter
    PhotonRoundHeader *header = nullptr;
    uint32_t capacity = 0;        // emissions per round the buffers hold
};
constexpr uint32_t kPhotonEventDomain = 0x70686f74u, kPhotonDiscDomain = 0x64697363u;   // seed domains, see mr_trace_photons
constexpr uint32_t kPhotonMaxDepth = 32;
// need: stores still missing to the target (> 0)
mr_status launch_photon_round(const DeviceScene &ds, const PhotonWalkLight &lt, uint32_t seed, uint32_t caustic, uint32_t max_depth,
                              uint32_t first, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b, hipStream_t stream);
// the same round on the kernel of mr_photon_walk_surface.hip: the colour and the normal of every hit are the surface pass's
// (tex: the scene's table, recs / mat_tex nullptr without one)
mr_status launch_photon_round_surface(const DeviceScene &ds, const TexParams &tex, const PhotonWalkLight &lt, uint32_t seed, uint32_t caustic,
                                      uint32_t max_depth, uint32_t first, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b,
                                      hipStream_t stream);
// what follows either walk (mr_photon_walk.hip): photon_scan_kernel and photon_compact_kernel over the round's words and slots
mr_status launch_photon_round_finish(uint32_t max_depth, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b, hipStream_t stream);
// the texture table on the device, uploaded on `stream` by the first call after a change (mr_api.cpp); `p`: as the kernels take it
mr_status texture_params(mr_scene *s, hipStream_t stream, TexParams &p);
// what mr_trace_photons needs to know of a map (the struct lives in mr_photon.cpp)
int32_t photon_map_device(const mr_photon_map *m);
bool photon_map_balanced(const mr_photon_map *m);
uint32_t photon_map_stored(const mr_photon_map *m);
// ... and mr_render_recursion_photons: balanced and resident on a device; one queued k-NN estimate on such a map, which takes the
// next of the map's hand-out counters and the map's statistics as mr_irradiance_estimate's launch does
bool photon_map_resident(const mr_photon_map *m);
mr_status photon_map_estimate_queued(mr_photon_map *m, const float *d_pos, const float *d_normal, const unsigned long long *d_n,
                                     unsigned long long bound, float max_dist, uint32_t nphotons, float *d_irrad, hipStream_t stream);

// the photon map built on the device (mr_photon_build.hip; mr_photon_map_build_device): store + scale + balance of one batch of
// records on an empty map.  The workspace lives from _begin to _end; the stages run in the order declared.
struct PhotonBuildStatus {            // what the store kernel leaves for the host: O(1)
    uint32_t lo[3], hi[3];            // the bounding box as order-preserving keys (decoded by launch_photon_build_store)
    uint32_t nonfinite, deferred;     // some position is not finite; photons whose direction bytes the host decides
};
struct PhotonBuildWork;
// m: photons taken (after the cap); tables1024: the host's DirTables (costheta, sintheta, cosphi, sinphi)
mr_status photon_build_begin(uint32_t m, const float *tables1024, PhotonBuildWork **out, hipStream_t stream);
void photon_build_end(PhotonBuildWork *w);
// the store kernel, then `status` and the box on the host (synchronises `stream`)
mr_status launch_photon_build_store(PhotonBuildWork *w, const mr_photon_record *d_records, float scale, PhotonBuildStatus *status, float lo[3], float hi[3],
                                    hipStream_t stream);
// the deferred list on the device, status.deferred entries of (storage index as bits, dx, dy, dz); the host overwrites .y with
// theta | phi << 8 (as bits) and copies the entries back before launch_photon_build_fix
float4 *photon_build_deferred(PhotonBuildWork *w);
mr_status launch_photon_build_fix(PhotonBuildWork *w, uint32_t count, hipStream_t stream);
mr_status launch_photon_build_tree(PhotonBuildWork *w, hipStream_t stream);
// dev.rec / power / boxes are allocated for photon_map_layout(dev, m); d_dir: 2 m bytes, the quantised directions in heap order
mr_status launch_photon_build_pack(PhotonBuildWork *w, PhotonMapDev &dev, uint8_t *d_dir, hipStream_t stream);

}  // namespace mr

struct mr_scene {
    int32_t device = 0;
    mr::HostMesh mesh;
    mr::HostTree tree;
    bool built = false;       // host tree exists
    bool on_device = false;   // device records uploaded
    mr::DeviceScene dev;
    unsigned long long *d_stats = nullptr;
    unsigned long long *d_work_counters = nullptr;   // ring of kWorkCounters hand-out counters
    std::atomic<uint32_t> next_counter{0};
    // eye-relative tables of mr_render_direct, a set allocated on first use: mr::eye_table_bytes each
    mr::EyeTablePool eye_tables;
    // grow-only staging buffers for host-pointer traces; stage_mutex serialises the calls that use them, so that
    // mr_trace may be called concurrently from several host threads (Scene::trace is const and re-entrant,
    // Scene.cpp:112-115 calls it from every OpenMP worker)
    void *d_stage_rays = nullptr, *d_stage_hits = nullptr;
    uint64_t stage_cap = 0;
    std::mutex stage_mutex;
    // large host-pointer traces are cut into chunks: upload of chunk k+1, kernel of chunk k and download of chunk k-1
    // overlap on these copy streams (events order them against the caller's stream)
    void *copy_in = nullptr, *copy_out = nullptr;   // hipStream_t
    std::vector<void *> stage_events;               // hipEvent_t, grow-only
    // grow-only per-primary-ray occlusion flags for mr_shade_direct
    uint8_t *d_occluded = nullptr;
    uint64_t occluded_cap = 0;
    // grow-only per-ray light attenuation for mr_shade_accumulate
    float *d_light_scale = nullptr;
    uint64_t light_scale_cap = 0;
    // materials (host copy; uploaded by mr_scene_set_materials / mr_bvh_build)
    std::vector<float> materials;          // 11 per material, clamped as the Phong constructor does
    std::vector<uint32_t> prim_material;   // empty: material 0 everywhere
    // Scene::lights() for mr_shade_lights (host only: the list travels in the kernel arguments), at most MR_MAX_LIGHTS
    std::vector<mr::ShadeLight> lights;
    // Scene::m_environment / m_bgColor / m_environmentRotation for mr_shade_environment.  d_env: the texel records on the
    // device (full image, then low-res), uploaded by the first shade call after a change (env_dirty)
    mr::HostEnvironment env;
    float4 *d_env = nullptr;
    bool env_dirty = false;
    // the texture table of mr_scene_set_textures.  d_tex: its device copy, uploaded by the first shading call after a change
    // (tex_dirty), like the environment's
    mr::HostTextures tex;
    float4 *d_tex = nullptr;
    bool tex_dirty = false;
    // mr_finish_image's three words (launch_finish_image), allocated and set to their identities by the first call
    uint32_t *d_finish_state = nullptr;
};
