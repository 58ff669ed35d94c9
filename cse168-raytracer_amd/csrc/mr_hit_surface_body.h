// mr_hit_surface_body.h -- diffuseColor (Phong.cpp:51-56; Scene.cpp:545-549 in the photon roulette) and HitInfo::N as
// Scene::trace leaves it (Scene.cpp:234-263) for ONE hit, as a device function.  Two callers: the loop of hit_surface_kernel
// (mr_procedural.hip; mr_hit_surface) and the photon walk of mr_photon_walk_surface.hip.
//
// The caller brings the hit point and the object's own normal (surface_od<true> of mr_surface.h); this function does the
// material -> texture id step, reads the kind, maps the point with uv_of for the UV kinds only, looks the colour up in one of
// the seven arms (or takes the plain material's kd), bump-maps the normal of a STONE hit and normalises.  The arms are the
// shared functions of mr_texture.h, mr_procedural_body.h and mr_solid_body.h, and every unit is compiled with
// -ffp-contract=off: the photon walk's colour and normal are the bits mr_hit_surface writes for the same ray and hit
// (tests/test_photon_walk_surface.py holds the two together).  The noise arms sit behind one branch: a wave none of whose
// hits lies on a STONE / STEM / UVW material skips them whole.
//
// t.mat_tex may be nullptr (a scene without a texture table: every hit is plain Phong).  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_noise.h"
#include "mr_procedural_body.h"
#include "mr_solid_body.h"
#include "mr_surface.h"
#include "mr_texture.h"
#include "mr_uv.h"

namespace mr {
namespace {

// ok: cleared when the reference leaves the lookup undefined (never set)
__device__ __forceinline__ void hit_color_normal(const rec::MeshMat &m, const TexParams &t, const NoiseTables &nt, uint32_t prim,
                                                 const float P[3], float N[3], float col[3], bool &ok) {
    const uint32_t mid = material_id(m.s, m.prim_mat, prim);
    const uint32_t tex = t.mat_tex ? t.mat_tex[mid] : kNoTexture;
    if (tex == kNoTexture) {
        const float *mt = m.mats + 11 * (size_t)mid;
        col[0] = mt[0]; col[1] = mt[1]; col[2] = mt[2];
    } else {
        const uint32_t kind = __float_as_uint(t.recs[3 * (size_t)tex].x);
        const bool uvw = kind >= kTexPetal;
        float u = P[0], v = P[1];                                    // LeafTexture reads (P.x, P.y) (Texture.h:232-233)
        if (!uvw) {
            const UvPtrs um = {m.s, t.texcoords, t.ti};
            uv_of(um, prim, P, u, v);
        }
        // the noise is behind this branch: a wave none of whose hits lies on a procedural material skips it whole
        if (uvw || kind == kTexStone || kind == kTexStem) {
            const float4 q1 = t.recs[3 * (size_t)tex + 1];
            if (kind == kTexStem || kind == kTexLeaf) {
                stem_color(nt, q1.w, u, v, col, ok);
            } else if (kind == kTexStone) {
                stone_color(nt, q1.w, u, v, col, ok);
                bump_normal(nt, q1.w, u, v, N, ok);
            } else {
                const float pivot[3] = {q1.x, q1.y, q1.z};
                const float radius = t.recs[3 * (size_t)tex + 2].x;
                float crd[3];
                if (kind == kTexPetal) petal_color(nt, pivot, radius, P, col, crd, ok);
                else flower_center_color(pivot, radius, P, col);
            }
        } else {
            ok = texture_color(t, tex, u, v, col);
        }
    }
    normalize3(N);                                                   // Scene.cpp:262
}

}  // namespace
}  // namespace mr
