// mr_environment.hip -- Scene::getEnvironmentMap (Scene.cpp:657-688) for the rays of a traced batch that MISSED
// (mr_shade_environment): what Scene::traceScene gives a ray that leaves the scene (Scene.cpp:338-342).
//
//   for every ray whose hit record is a miss:  value = m_bgColor, or LoadedTexture::lookup (Texture.cpp:161-185) of the lat-long
//   image at the ray's direction -- the full image, or the 24-texel-wide low-res copy for rays made by Ray::random
//   (ray.isDiffuse);  then weight * value / spp added to the ray's pixel.
//
// A streaming kernel, one lane per ray, whole waves (accumulate_runs shuffles).  A lane loads its 16-byte hit record; only a
// lane that missed goes on to load the second half of its ray (the direction: the origin is never needed) and, with an image,
// its four texels.  A wave without a miss leaves the iteration at once.  Texels are 16-byte records (r, g, b, 0), so a fetch
// is one dwordx4 -- the only irregular traffic of the kernel.  The low-res image (24 x lh <= 96 texels, 9 KB for a 2:1
// image) is copied into LDS by every workgroup at its start: lanes of a wave look into it at unrelated addresses, which LDS
// serves at its bank rate, whereas the scalar / constant path wants one address per wave (a divergent read through it is
// a loop over the lanes).  The grid of the image variants is held to 8 workgroups per CU so that this copy stays small
// beside the batch.
//
// The arithmetic of the lookup is the reference's (mr_environment_body.h, shared with the fused frame of
// mr_frame_lights_env.hip; the bilinear part is mr_texture.h, shared with the material textures),
// operation for operation in fp32 (this unit is compiled with
// -ffp-contract=off like the rest), on mm_atan2f / mm_asinf of miro_math.h: texture coordinates are the same bits as a host
// restatement's.  powf is the device library's (the tolerance of the shaded value, as in mr_lights.hip).
//
// Variants (template arguments) only where a branch would sit in the loop body of every lane: image / colour only, weights,
// pixel map.  The optional outputs and the low-res mask are wave-uniform branches.
#include <hip/hip_runtime.h>

#include "miro_math.h"
#include "mr_environment_body.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_recursion.h"
#include "mr_texture.h"
#include "mr_traverse.h"

namespace mr {
namespace {

struct EnvArgs {
    EnvParams env;
    const float4 *rays;           // two per ray
    const float4 *hits;
    const float *weights;         // rgb per ray (WEIGHTS)
    const uint32_t *pixels;       // pixel per ray (PIXELS), otherwise ray index / spp
    const uint8_t *lowres;        // may be NULL: per ray, non-zero = the low-res image
    uint32_t all_lowres;          // MR_ENV_LOWRES
    uint32_t spp;
    float inv_spp;
    unsigned long long n;
    float *rgb;                   // may be NULL (then ray_rgb is not)
    float *ray_rgb;               // may be NULL: the un-weighted value of every ray
    unsigned long long *counts;   // optional: [0] += misses, [1] += undefined lookups
};

template <bool IMAGE, bool WEIGHTS, bool PIXELS>
__global__ __launch_bounds__(kBlock) void shade_environment_kernel(EnvArgs a) {
    extern __shared__ float4 s_low[];                 // IMAGE: the low-res image, lw * lh records
    const int tid = threadIdx.x;
    __builtin_assume(!PIXELS || a.pixels != nullptr);     // what launch_env_i chose the variant by
    __builtin_assume(!WEIGHTS || a.weights != nullptr);
    const bool any_lowres = IMAGE && (a.all_lowres || a.lowres);
    if (any_lowres) {
        const unsigned n_low = a.env.lw * a.env.lh;
        for (unsigned i = tid; i < n_low; i += kBlock) s_low[i] = a.env.low[i];
        __syncthreads();
    }
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const unsigned long long n_round = (a.n + 63ull) & ~63ull;          // whole waves: accumulate_runs shuffles
    unsigned my_misses = 0, my_undefined = 0;

    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + tid; k < n_round; k += stride) {
        const bool live = k < a.n;
        bool miss = false;
        if (live) miss = __float_as_uint(a.hits[k].y) == MR_MISS;
        if (!__any(miss)) {                                             // wave-uniform: nothing to add
            if (a.ray_rgb && live) { a.ray_rgb[3 * k] = 0.f; a.ray_rgb[3 * k + 1] = 0.f; a.ray_rgb[3 * k + 2] = 0.f; }
            continue;
        }
        float val[3] = {0.f, 0.f, 0.f};
        if (miss) {
            my_misses++;
            if (!IMAGE) {
                val[0] = a.env.bg[0]; val[1] = a.env.bg[1]; val[2] = a.env.bg[2];          // :685
            } else {
                const float4 rb = a.rays[2 * k + 1];
                const bool low = a.all_lowres || (a.lowres && a.lowres[k]);                // ray.isDiffuse (:678-681)
                const int w = low ? (int)a.env.lw : (int)a.env.W, h = low ? (int)a.env.lh : (int)a.env.H;
                float xe = 0.f, ye = 0.f;
                int x1 = 0, x2 = 0, y1 = 0, y2 = 0;
                if (env_texels(a.env.rot, w, h, rb.x, rb.y, rb.z, x1, x2, y1, y2, xe, ye)) {
                    float4 p11, p21, p12, p22;
                    if (low) {
                        p11 = s_low[y1 * w + x1]; p21 = s_low[y1 * w + x2]; p12 = s_low[y2 * w + x1]; p22 = s_low[y2 * w + x2];
                    } else {
                        const float4 *r1 = a.env.full + (size_t)y1 * w, *r2 = a.env.full + (size_t)y2 * w;
                        p11 = r1[x1]; p21 = r1[x2]; p12 = r2[x1]; p22 = r2[x2];
                    }
                    env_blend(p11, p21, p12, p22, xe, ye, a.env.max_intensity, val);
                } else {
                    my_undefined++;
                }
            }
        }
        if (a.ray_rgb && live) { a.ray_rgb[3 * k] = val[0]; a.ray_rgb[3 * k + 1] = val[1]; a.ray_rgb[3 * k + 2] = val[2]; }
        if (a.rgb) {                                                    // wave-uniform
            uint32_t pix = 0xFFFFFFFFu;
            float o[3] = {0.f, 0.f, 0.f};
            if (live) pix = rec::pixel_of(PIXELS ? a.pixels : nullptr, k, a.spp);
            if (miss) {
                float wt[3];
                rec::weight_of(WEIGHTS ? a.weights : nullptr, k, wt);
                for (int c = 0; c < 3; c++) o[c] = val[c] * wt[c] * a.inv_spp;
            }
            rec::accumulate_runs(a.rgb, pix, o[0], o[1], o[2]);
        }
    }

    if (a.counts) {
        const unsigned mine[2] = {my_misses, my_undefined};
        workgroup_add<kBlock>(mine, a.counts);
    }
}

template <bool IMAGE, bool WEIGHTS, bool PIXELS>
mr_status launch_env_t(const EnvArgs &a, hipStream_t stream) {
    unsigned grid = grid_for(a.n);
    size_t lds = 0;
    if (IMAGE) {
        if (grid > 256u * 8u) grid = 256u * 8u;       // every workgroup copies the low-res image: few, long-lived workgroups
        lds = (size_t)a.env.lw * a.env.lh * sizeof(float4);
    }
    hipLaunchKernelGGL((shade_environment_kernel<IMAGE, WEIGHTS, PIXELS>), dim3(grid), dim3(kBlock), lds, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

template <bool IMAGE>
mr_status launch_env_i(const EnvArgs &a, hipStream_t stream) {
    if (a.weights) return a.pixels ? launch_env_t<IMAGE, true, true>(a, stream) : launch_env_t<IMAGE, true, false>(a, stream);
    return a.pixels ? launch_env_t<IMAGE, false, true>(a, stream) : launch_env_t<IMAGE, false, false>(a, stream);
}

}  // namespace

mr_status launch_shade_environment(const EnvParams &env, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                   const uint32_t *d_pixels, const uint8_t *d_lowres, unsigned long long n, uint32_t spp,
                                   uint32_t flags, float *d_rgb, float *d_ray_rgb, unsigned long long *d_counts, hipStream_t stream) {
    if (n == 0) return MR_OK;
    if (env.lw * env.lh > kEnvLowresWidth * kEnvMaxLowresHeight) return fail(MR_ERR_INVALID, "low-res environment image does not fit in LDS");
    EnvArgs a;
    a.env = env;
    a.rays = reinterpret_cast<const float4 *>(d_rays); a.hits = reinterpret_cast<const float4 *>(d_hits);
    a.weights = d_weights; a.pixels = d_pixels; a.lowres = d_lowres;
    a.all_lowres = (flags & MR_ENV_LOWRES) ? 1u : 0u;
    a.spp = spp; a.inv_spp = 1.0f / (float)spp; a.n = n;
    a.rgb = d_rgb; a.ray_rgb = d_ray_rgb; a.counts = d_counts;
    return env.full ? launch_env_i<true>(a, stream) : launch_env_i<false>(a, stream);
}

}  // namespace mr
