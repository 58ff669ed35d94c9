// mr_children_col.h -- the last step of a fused PATH_TRACING level, written once for the kernels that end in it
// (mr_level_lights_path.hip: level_lights_path_kernel; mr_frame_lights_surface_body.h with CHILDREN == 2: frame_level_lights_kernel):
//   env_lookup          Scene::getEnvironmentMap's lookup of the image a ray reads, the full one or its low-res copy
//   write_children_col  rec::write_children<BLOCK, true> with the looked-up colour on the diffuse child and the child's low-res byte
// Device code only; included by the .hip units that call them (everything here is local to its unit).
#pragma once

#include <hip/hip_runtime.h>

#include "mr_environment_body.h"
#include "mr_internal.h"
#include "mr_recursion.h"

namespace mr {
namespace {

// Scene::getEnvironmentMap's lookup of the image a ray reads (Scene.cpp:678-681): the full one, or the low-res copy for a ray
// that is isDiffuse -- shade_environment_kernel's choice of w, h and texel source, the copy read where it lies.  false:
// undefined, val is left as it was.
__device__ __forceinline__ bool env_lookup(const EnvParams &env, bool low, float dx, float dy, float dz, float val[3]) {
    const int w = low ? (int)env.lw : (int)env.W, h = low ? (int)env.lh : (int)env.H;
    float xe = 0.f, ye = 0.f;
    int x1 = 0, x2 = 0, y1 = 0, y2 = 0;
    if (!env_texels(env.rot, w, h, dx, dy, dz, x1, x2, y1, y2, xe, ye)) return false;
    const float4 *img = low ? env.low : env.full;
    const float4 *r1 = img + (size_t)y1 * w, *r2 = img + (size_t)y2 * w;
    env_blend(r1[x1], r1[x2], r2[x1], r2[x2], xe, ye, env.max_intensity, val);
    return true;
}

// rec::write_children<BLOCK, true> whose diffuse child (kind 3) carries w0 * col instead of make()'s w0 * m_diffuse, the rule of
// write_children_col_at (mr_children_body.h), and which writes the child's low-res byte with it.  Called by all threads of the
// workgroup.
template <int BLOCK>
__device__ __forceinline__ void write_children_col(const rec::ChildQueue &q, uint8_t *out_lowres, const rec::ChildGen<true> &g, const float col[3],
                                                   const bool emit[4], uint32_t pix, uint32_t id) {
    const int lane = threadIdx.x & 63;
    unsigned long long mk[4];
    int cn[4], tot = 0;
    for (int j = 0; j < 4; j++) { mk[j] = __ballot(emit[j]); cn[j] = __popcll(mk[j]); tot += cn[j]; }
    const unsigned long long base = rec::workgroup_reserve<BLOCK>((unsigned)tot, q.count);
    const unsigned long long lt = (1ull << lane) - 1ull;
    unsigned long long before = base;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const unsigned long long s = before + __popcll(mk[j] & lt);
        if (emit[j] && s < q.capacity) {
            float org[3], dir[3], wgt[3];
            g.make(j, org, dir, wgt);
            if (j == 3)
                for (int c = 0; c < 3; c++) wgt[c] = g.w0[c] * col[c];
            reinterpret_cast<float4 *>(q.rays)[2 * s] = make_float4(org[0], org[1], org[2], 0.0f);
            reinterpret_cast<float4 *>(q.rays)[2 * s + 1] = make_float4(dir[0], dir[1], dir[2], 1e12f);
            q.weights[3 * s] = wgt[0]; q.weights[3 * s + 1] = wgt[1]; q.weights[3 * s + 2] = wgt[2];
            q.pixels[s] = pix;
            if (q.ids) q.ids[s] = rec::child_id(id, j);
            if (q.octants) q.octants[s] = rec::octant_of(dir);
            if (out_lowres) out_lowres[s] = j == 3 ? (uint8_t)1 : (uint8_t)0;
        }
        before += cn[j];
    }
}

}  // namespace
}  // namespace mr
