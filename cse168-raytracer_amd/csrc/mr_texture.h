// mr_texture.h -- Texture::lookup2D on the device: the bilinear image lookup of LoadedTexture::lookup (Texture.cpp:161-185),
// shared by the environment of rays that miss (mr_environment.hip) and the textures of TexturedPhong materials
// (mr_textures.hip), and CheckerBoardTexture::lookup2D (Texture.h:112-133).  Device code only; every operation in fp32 in the
// reference's order (the units that include this are compiled with -ffp-contract=off).
//
// An image is an array of 16-byte records (r, g, b, 0), row 0 = the bottom scanline, so that a texel fetch is one dwordx4;
// a lookup is four of them at addresses that differ from lane to lane (vector loads: the scalar path wants one address per
// wave).  The texture table (TexParams, mr_internal.h) is read per lane too -- neighbouring hits lie on different
// materials -- as three dwordx4 of a 48-byte record.
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_surface.h"
#include "mr_uv.h"

namespace mr {

// Texture.cpp:170-178 for one axis: the two texel indices and the error term -- taken from the WRAPPED first index (:174).
// false: the reference's arithmetic leaves the image (undefined there, defined as 0 here)
__device__ __forceinline__ bool bilinear_axis(int w, float c, int &i1, int &i2, float &err) {
    const float p = (float)w * c;                                       // :170
    if (!(fabsf(p) < 2147483520.0f)) return false;                      // NaN, or (int)p overflows
    i1 = (int)p; i2 = i1 + 1;                                           // :172
    i1 %= w; i2 %= w;                                                   // :173
    err = p - (float)i1;                                                // :174
    return i1 >= 0 && i2 >= 0;
}

// Texture.cpp:181 for one channel
__device__ __forceinline__ float bilinear_mix(float p11, float p21, float p12, float p22, float xe, float ye) {
    return (p11 * (1 - xe) + p21 * xe) * (1 - ye) + (p12 * (1 - xe) + p22 * xe) * ye;
}
// ... then tonemapValue of a FIT_RGBF image (:27): std::min(a, b) = b < a ? b : a keeps a NaN
__device__ __forceinline__ float bilinear_blend(float p11, float p21, float p12, float p22, float xe, float ye, float max_intensity) {
    const float f = bilinear_mix(p11, p21, p12, p22, xe, ye);
    const float a = powf(f / max_intensity, 0.5f) * 1.5f;
    return 1.0f < a ? 1.0f : a;
}

enum : uint32_t { kTexChecker = 0u, kTexImage = 1u };                   // MR_TEX_CHECKER, MR_TEX_IMAGE

// Texture::lookup2D of texture `id` at (u, v).  false: the lookup is undefined in the reference (rgb is then color1 for a
// checker, 0 for an image).
__device__ __forceinline__ bool texture_color(const TexParams &t, uint32_t id, float u, float v, float rgb[3]) {
    const float4 q0 = t.recs[3 * (size_t)id], q1 = t.recs[3 * (size_t)id + 1];
    if (__float_as_uint(q0.x) == kTexChecker) {                         // Texture.h:125-132
        const float scale = q1.w;
        float a = fabsf(scale * u), b = fabsf(scale * v);
        bool ok = a < 0x1p30f && b < 0x1p30f;                           // finite, and (int) is defined
        if (u < 0) a += scale;
        if (v < 0) b += scale;
        ok = ok && fabsf(a) < 0x1p30f && fabsf(b) < 0x1p30f;
        rgb[0] = q1.x; rgb[1] = q1.y; rgb[2] = q1.z;
        if (ok && ((int)a + (int)b) % 2 != 0) {
            const float4 q2 = t.recs[3 * (size_t)id + 2];
            rgb[0] = q2.x; rgb[1] = q2.y; rgb[2] = q2.z;
        }
        return ok;
    }
    const int w = (int)__float_as_uint(q0.y), h = (int)__float_as_uint(q0.z);
    float xe = 0.f, ye = 0.f;
    int x1 = 0, x2 = 0, y1 = 0, y2 = 0;
    const bool okx = bilinear_axis(w, u, x1, x2, xe), oky = bilinear_axis(h, v, y1, y2, ye);
    rgb[0] = 0.f; rgb[1] = 0.f; rgb[2] = 0.f;
    // a material texture is undefined for EVERY negative coordinate (mr_scene_set_textures, miro_hip.h): also for the sliver
    // -1 / w < u < 0, where (int) truncates to texel 0 and the reference's arithmetic happens to stay inside the image
    if (!(okx && oky) || u < 0 || v < 0) return false;
    const float4 *img = t.texels + __float_as_uint(q0.w);
    const float4 *r1 = img + (size_t)y1 * w, *r2 = img + (size_t)y2 * w;
    const float4 p11 = r1[x1], p21 = r1[x2], p12 = r2[x1], p22 = r2[x2];
    if (__float_as_uint(q1.y)) {                                        // FIT_RGBF: tonemapValue (Texture.cpp:23-28)
        rgb[0] = bilinear_blend(p11.x, p21.x, p12.x, p22.x, xe, ye, q1.x);
        rgb[1] = bilinear_blend(p11.y, p21.y, p12.y, p22.y, xe, ye, q1.x);
        rgb[2] = bilinear_blend(p11.z, p21.z, p12.z, p22.z, xe, ye, q1.x);
    } else {                                                            // FIT_BITMAP: the identity
        rgb[0] = bilinear_mix(p11.x, p21.x, p12.x, p22.x, xe, ye);
        rgb[1] = bilinear_mix(p11.y, p21.y, p12.y, p22.y, xe, ye);
        rgb[2] = bilinear_mix(p11.z, p21.z, p12.z, p22.z, xe, ye);
    }
    return true;
}

// diffuseColor of a hit on material `mid` (Phong.cpp:51-56): Texture::lookup2D at the object's UV coordinates for a
// TexturedPhong, m_diffuse for a plain Phong
__device__ __forceinline__ void diffuse_color_of(const rec::MeshMat &m, const TexParams &t, uint32_t mid, uint32_t prim,
                                                 const float P[3], float col[3]) {
    const uint32_t tex = t.mat_tex[mid];
    if (tex == kNoTexture) {
        const float *mt = m.mats + 11 * (size_t)mid;
        col[0] = mt[0]; col[1] = mt[1]; col[2] = mt[2];
        return;
    }
    const UvPtrs um = {m.s, t.texcoords, t.ti};
    float u, v;
    uv_of(um, prim, P, u, v);
    (void)texture_color(t, tex, u, v, col);
}

// Where a shading body (mr_lights_body.h, mr_accumulate_body.h) takes a hit's diffuseColor from; the last brings the normal too
enum ColorSource : int {
    kColorMaterial,   // the material's own m_diffuse, read where it is used
    kColorTexture,    // diffuse_color_of above, once per hit
    kColorSurface,    // the surface pass's two per-ray buffers (mr_hit_surface): the colour and the bump-mapped normal
};

}  // namespace mr
