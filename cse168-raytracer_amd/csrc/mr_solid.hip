// mr_solid.hip -- the surface pass and the inspection kernel of scenes whose texture table holds a UVW texture: the reference's
// Texture3D materials PetalTexture, LeafTexture and FlowerCenterTexture (mr_solid_body.h), which Phong::shade looks up at the hit
// point itself (Phong.cpp:53-56).
//
//   solid_surface_kernel      the whole surface pass of such a scene (mr_hit_surface): procedural_surface_kernel's body
//                             (mr_procedural.hip) plus the UVW arm -- lookup3D at the hit's P, the normal only normalised,
//                             neither uv_of nor the bump applied.  A scene without a UVW kind never runs it.
//   texture_lookup3_kernel    lookup3D of one UVW texture for a batch of points (mr_texture_lookup3)
//
// A unit of its own: mr_procedural.hip stays the 17 kernels it was, at their recorded registers.  The 2-D arms are the shared
// functions of mr_procedural_body.h.  A petal hit costs 35 Perlin evaluations at most, the class of a stone hit; a wave leaves
// them once every lane's coordinates have grown whole (turbulence_whole).
#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_noise.h"
#include "mr_procedural_body.h"
#include "mr_solid_body.h"
#include "mr_texture.h"
#include "mr_traverse.h"
#include "mr_uv.h"

namespace mr {
namespace {

struct SolidSurfaceArgs {
    rec::MeshMat m;
    TexParams t;
    const mr_ray *rays;
    const mr_hit *hits;
    unsigned long long n;
    float *color, *normal;       // three floats per ray each; a ray that missed keeps what the buffers held
    unsigned long long *counts;  // optional: [0] += lookups the reference leaves undefined
};

__global__ __launch_bounds__(kBlock) void solid_surface_kernel(SolidSurfaceArgs a) {
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    unsigned my_undefined = 0;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < a.n; k += stride) {
        const float4 h = reinterpret_cast<const float4 *>(a.hits)[k];
        const uint32_t prim = __float_as_uint(h.y);
        if (prim == MR_MISS) continue;
        float P[3], N[3], col[3];
        surface<true>(a.m.s, a.rays, k, h.x, prim, h.z, h.w, P, N);
        const uint32_t mid = material_id(a.m.s, a.m.prim_mat, prim);
        const uint32_t tex = a.t.mat_tex[mid];
        bool ok = true;
        if (tex == kNoTexture) {
            const float *mt = a.m.mats + 11 * (size_t)mid;
            col[0] = mt[0]; col[1] = mt[1]; col[2] = mt[2];
        } else {
            const uint32_t kind = __float_as_uint(a.t.recs[3 * (size_t)tex].x);
            const bool uvw = kind >= kTexPetal;
            float u = P[0], v = P[1];                                    // LeafTexture reads (P.x, P.y) (Texture.h:232-233)
            if (!uvw) {
                const UvPtrs um = {a.m.s, a.t.texcoords, a.t.ti};
                uv_of(um, prim, P, u, v);
            }
            // the noise is behind this branch: a wave none of whose hits lies on a procedural material skips it whole
            if (uvw || kind == kTexStone || kind == kTexStem) {
                const float4 q1 = a.t.recs[3 * (size_t)tex + 1];
                if (kind == kTexStem || kind == kTexLeaf) {
                    stem_color(nt, q1.w, u, v, col, ok);
                } else if (kind == kTexStone) {
                    stone_color(nt, q1.w, u, v, col, ok);
                    bump_normal(nt, q1.w, u, v, N, ok);
                } else {
                    const float pivot[3] = {q1.x, q1.y, q1.z};
                    const float radius = a.t.recs[3 * (size_t)tex + 2].x;
                    float crd[3];
                    if (kind == kTexPetal) petal_color(nt, pivot, radius, P, col, crd, ok);
                    else flower_center_color(pivot, radius, P, col);
                }
            } else {
                ok = texture_color(a.t, tex, u, v, col);
            }
        }
        normalize3(N);                                                   // Scene.cpp:262
        if (!ok) my_undefined++;
        a.color[3 * k] = col[0]; a.color[3 * k + 1] = col[1]; a.color[3 * k + 2] = col[2];
        a.normal[3 * k] = N[0]; a.normal[3 * k + 1] = N[1]; a.normal[3 * k + 2] = N[2];
    }
    if (a.counts) workgroup_add<kBlock>(my_undefined, &a.counts[0]);
}

// coords: optional, written for a PETAL alone
__global__ __launch_bounds__(kBlock) void texture_lookup3_kernel(TexParams t, uint32_t id, const float *p, unsigned long long n, float *rgb,
                                                                 float *coords, unsigned long long *counts) {
    __shared__ uint32_t s_tab[128];
    const NoiseTables nt = stage_noise_tables(s_tab);
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const uint32_t kind = __float_as_uint(t.recs[3 * (size_t)id].x);
    const float4 q1 = t.recs[3 * (size_t)id + 1], q2 = t.recs[3 * (size_t)id + 2];
    unsigned my_undefined = 0;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        const float P[3] = {p[3 * k], p[3 * k + 1], p[3 * k + 2]};
        float c[3], crd[3];
        bool ok = true;
        solid_color(nt, kind, q1, q2, P, c, crd, ok);
        if (!ok) my_undefined++;
        rgb[3 * k] = c[0]; rgb[3 * k + 1] = c[1]; rgb[3 * k + 2] = c[2];
        if (coords && kind == kTexPetal) { coords[3 * k] = crd[0]; coords[3 * k + 1] = crd[1]; coords[3 * k + 2] = crd[2]; }
    }
    if (counts) workgroup_add<kBlock>(my_undefined, &counts[0]);
}

}  // namespace

mr_status launch_hit_surface_solid(const DeviceScene &ds, const TexParams &tex, const mr_ray *d_rays, const mr_hit *d_hits,
                                   unsigned long long n, float *d_color, float *d_normal, unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    if ((ds.spheres || ds.planes) && !d_rays)
        return fail(MR_ERR_INVALID, "the scene holds spheres / planes: their hit point is o + t*d, d_rays is required");
    SolidSurfaceArgs a;
    a.m = rec::mesh_of(ds); a.t = tex; a.rays = d_rays; a.hits = d_hits; a.n = n; a.color = d_color; a.normal = d_normal; a.counts = d_counts;
    hipLaunchKernelGGL(solid_surface_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_texture_lookup3(const TexParams &tex, uint32_t texture, const float *d_p, unsigned long long n, float *d_rgb,
                                 float *d_coords, unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    hipLaunchKernelGGL(texture_lookup3_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, tex, texture, d_p, n, d_rgb, d_coords, d_counts);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
