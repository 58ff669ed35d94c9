// mr_procedural_body.h -- the 2-D procedural lookups and the bump mapping as device functions: StemTexture::lookup2D
// (Texture.h:192-212), StoneTexture::lookup2D and ::bumpHeight2D (Texture.cpp:358-440) over the noise of mr_noise.h, and the
// perturbation of Scene::trace (Scene.cpp:235-261).  Called by the inspection kernels of mr_procedural.hip and by
// hit_color_normal (mr_hit_surface_body.h), next to the UVW kinds (mr_solid_body.h).  Device code only; the units that include
// this are compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include "miro_math.h"
#include "mr_noise.h"
#include "mr_uv.h"

namespace mr {
namespace {

enum : uint32_t { kTexStone = 2u, kTexStem = 3u };                      // MR_TEX_STONE, MR_TEX_STEM

// StemTexture::lookup2D (Texture.h:192-212)
__device__ __forceinline__ void stem_color(const NoiseTables &nt, float scale, float cu, float cv, float rgb[3], bool &ok) {
    const float u = cu * scale, v = cv * scale;
    const Worley3 w = worley2(nt, u, v, ok);
    const float noise = turbulence(nt, u, v, 10, 1.5f, 0.8f, 10, ok);
    const float cells = w.F0 - w.F1;
    rgb[0] = 0.0f;
    rgb[1] = (float)(0.5 + 0.5 * (double)(noise + 1.0f) / (double)2.0f - 0.3 * (double)cells);                  // :211
    rgb[2] = 0.0f;
}

// (1 - pow(f[1] - f[0], 0.8f)) * 1.5 (Texture.cpp:370,409)
__device__ __forceinline__ float stone_outline(const Worley3 &w) {
    return (float)((double)(1 - mm_powf(w.F1 - w.F0, 0.8f)) * 1.5);
}

// StoneTexture::bumpHeight2D (Texture.cpp:358-393).  The two branches differ in the parameters of one generateNoise call.
__device__ __forceinline__ float stone_height(const NoiseTables &nt, float scale, float cu, float cv, bool &ok) {
    const float u = cu * scale, v = cv * scale;
    const float height_factor = (float)0.3;
    const Worley3 w = worley2(nt, u, v, ok);
    float f1f0 = stone_outline(w);
    f1f0 *= -1.f;
    // exp of an argument beyond +-700 (only a search that found fewer than two points gets there) gives the same float
    // height as the bound itself: 1 or 0
    double z = -20.0 * ((double)(w.F1 - w.F0) - 0.3);                                                           // :372
    z = z < -700.0 ? -700.0 : (z > 700.0 ? 700.0 : z);
    const float height = (float)(1.0 / (1.0 + mm_exp(z)));
    const bool inside = (double)f1f0 > -1.1;                                                                    // :373
    const float turb = turbulence(nt, u, v, inside ? 0.5f : 1.0f, 2, 0.5f, inside ? (int)(w.I0 % 3u) + 5 : 3, ok);   // :376,381
    const float t = (float)((double)(turb / (inside ? 5.0f : 10.0f)) + 0.5);
    return (inside ? 0.8f : 1.0f) * t + height_factor * height;                                                 // :377,391
}

// StoneTexture::lookup2D (Texture.cpp:396-440)
__device__ __forceinline__ void stone_color(const NoiseTables &nt, float scale, float cu, float cv, float rgb[3], bool &ok) {
    const float u = cu * scale, v = cv * scale;
    const Worley3 w = worley2(nt, u, v, ok);
    const float f1f0 = stone_outline(w);
    float base = uv_min(uv_max(mm_powf((w.F2 - w.F1 + w.F0), 0.1f) - f1f0, 0.f), 0.5f);                         // :412
    const float id10 = (float)(w.I0 % 10u), id5 = (float)(w.I0 % 5u);
    base = (float)((double)base * ((double)(id10 / 20) + 0.5));                                                 // :415
    const float turb = turbulence(nt, u, v, 3, 2, 0.8f, 5, ok);
    base = uv_max(0.0f, base);
    base = (float)((double)base + 0.8 * (double)fabsf(turb));                                                   // :420
    if ((double)f1f0 > 1.1) {
        const float edges = uv_min(f1f0 * f1f0 - 1.f, 0.75f);                                                   // :424
        rgb[0] = rgb[1] = rgb[2] = (float)((double)edges + 0.25 * (double)fabsf(turb));
    } else {
        rgb[0] = base + id10 / 10;                                                                              // :430-432
        rgb[1] = base + (id10 / 10) * 0.5f;
        rgb[2] = base + (id5 / 5) * 0.25f;
    }
}

// the bump mapping of Scene::trace (Scene.cpp:235-261) on the normal N as intersect() left it; the caller normalises (:262)
__device__ __forceinline__ void bump_normal(const NoiseTables &nt, float scale, float u, float v, float N[3], bool &ok) {
    const float delta = (float)0.0001;
    float u1 = 0.f, u2 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll 1
    for (int s = 0; s < 4; s++) {                                        // :243-246
        const float h = stone_height(nt, scale, s == 0 ? u - delta : (s == 1 ? u + delta : u),
                                     s == 2 ? v - delta : (s == 3 ? v + delta : v), ok);
        if (s == 0) u1 = h;
        if (s == 1) u2 = h;
        if (s == 2) v1 = h;
        if (s == 3) v2 = h;
    }
    const float dx = (u2 - u1) / (2 * delta), dy = (v2 - v1) / (2 * delta);                                     // :249-250
    const float n0 = N[0], n1 = N[1], n2 = N[2];
    int m = 0;                                                                                                  // :255-257
    float nm = n0;
    if (n1 > n0) { m = 1; nm = n1; }
    if (n2 > nm) m = 2;
    const float r[3] = {m == 2 ? -n2 : 0.f, m == 0 ? -n0 : 0.f, m == 1 ? -n1 : 0.f};                            // :258
    const float t1[3] = {n1 * r[2] - n2 * r[1], n2 * r[0] - n0 * r[2], n0 * r[1] - n1 * r[0]};                  // :260
    const float c1[3] = {n1 * t1[2] - n2 * t1[1], n2 * t1[0] - n0 * t1[2], n0 * t1[1] - n1 * t1[0]};
    const float c2[3] = {n1 * c1[2] - n2 * c1[1], n2 * c1[0] - n0 * c1[2], n0 * c1[1] - n1 * c1[0]};
    for (int c = 0; c < 3; c++) N[c] = N[c] + (c1[c] * dx - c2[c] * dy);                                        // :261
}

}  // namespace
}  // namespace mr
