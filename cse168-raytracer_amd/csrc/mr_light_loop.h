// mr_light_loop.h -- Phong::shade's loop over Scene::lights() (Phong.cpp:63-156) for ONE hit that a lane holds in registers, as a
// device function: per light the shadow ray, its closest-hit (or any-hit) traversal on the workgroup's LDS stack, the occluder's
// light scale, the point or disc terms, summed into L in list order.  Every fused kernel calls it: the light-list frames
// (mr_frame_lights.hip; mr_frame_lights_surface_body.h: mr_render_lights_surface, mr_render_lights_environment and the frames
// that emit level 1) and the level of the recursion (mr_level_lights_body.h).  The batched light-list kernels (shade_lights_body,
// mr_lights_body.h, which says why) keep the same steps written out, on the same shared pieces -- shadow_ray_for /
// light_scale_of / disc_terms / phong_terms / phong_combine of mr_phong.h -- so a ray's L is the same bits on every route.
//
// Called by ALL lanes of the wave (trace_hit is): a lane without a hit brings hit = false, traces the idle ray and leaves L as it
// was.  The shadow ray is built again after its traversal rather than kept live across it.  n_lights is wave-uniform.
// Included by the .hip units that instantiate it (everything here is local to its unit).
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_phong.h"
#include "mr_surface.h"
#include "mr_traverse.h"

namespace mr {
namespace {

// mt: the hit's material record; col: its diffuseColor; d: the direction of the ray that produced the hit
template <int VAR, bool ANY>
__device__ __forceinline__ void shade_light_list(const TraceParams &tp, const rec::MeshMat &m, const ShadeLight *lights, uint32_t n_lights,
                                                 bool hit, const float P[3], const float N[3], const float *mt, const float col[3],
                                                 const float d[3], int *s_stack, int tid, Stats &st, float L[3]) {
    using namespace rec;
    for (uint32_t li = 0; li < n_lights; li++) {                   // Phong.cpp:63, wave-uniform
        const ShadeLight &lt = lights[li];
        float4 sh;
        {
            float4 sa = make_float4(0.f, 0.f, 0.f, 0.f), sb = make_float4(1.f, 1.f, 1.f, -1.f);
            if (hit) shadow_ray_for(lt, P, sa, sb);
            const mr_hit hs = trace_hit<true, ANY, false, VAR>(tp, sa, sb, sb.w, hit, s_stack, tid, st);
            sh = *reinterpret_cast<const float4 *>(&hs);
        }
        if (hit) {
            float4 sa, sb;
            shadow_ray_for(lt, P, sa, sb);                         // rebuilt rather than kept across the traversal
            const float scale = light_scale_of(m, sa, sb, sh);
            float diffuse[3] = {0.f, 0.f, 0.f}, highlight = 0.0f, out[3] = {0.f, 0.f, 0.f};
            bool lit = scale != 0.0f;                              // Phong.cpp:100-111: the light is skipped
            if (lit) {
                if (lt.kind == MR_LIGHT_DISC) {
                    const float l[3] = {sb.x, sb.y, sb.z};
                    lit = disc_terms(lt, mt, col, P, N, l, d[0], d[1], d[2], diffuse, highlight);
                } else {
                    phong_terms(lt.position, lt.color, lt.wattage, mt, col, P, N, d[0], d[1], d[2], diffuse, highlight);
                }
            }
            if (lit) phong_combine(diffuse, highlight, scale, out);
            L[0] += out[0]; L[1] += out[1]; L[2] += out[2];
        }
    }
}

}  // namespace
}  // namespace mr
