// mr_solid_body.h -- Texture::lookup3D of the reference's three Texture3D materials as device functions: PetalTexture
// (Texture.cpp:447-505), LeafTexture (Texture.h:230-250) and FlowerCenterTexture (Texture.h:261-276).  Phong::shade hands them the
// hit point itself, diffuse3D(tex_coord3d_t(hit.P.x, hit.P.y, hit.P.z)) (Phong.cpp:53-56): no object mapping is involved, and
// Scene::trace bump-maps UV materials only (Scene.cpp:238), so the normal of such a hit is the geometric one, normalised.
// Device code only; every operation is a single-rounded fp32 operation in the reference's order (the unit that includes this is
// compiled with -ffp-contract=off), with the reference's own promotions to double where its literals are double.
//
// How the reference's lines read: Texture.cpp:14 has `using namespace std` behind <cmath>, so abs, acos, pow and sin of a float
// are the float overloads -- abs(generateNoise(..)) is fabsf, pow(turb / 0.1f, 0.85f) is powf; PI is the const float of
// Miro.h:10.  position.normalize() (Texture.cpp:476) normalises `position` in place (Vector3.h:205-208; `dir` is never read):
// phi, theta and the side test all read the unit vector.  sinphi is computed, clamped and never used (the division by it is
// commented out, :488): left out.  acos / powf are mm_acosf / the series of miro_math.h, where the reference calls libm.
//
// The whole-number rule.  PetalTexture's second turbulence runs 25 octaves from frequency 4 with factor 3: its last frequency
// is 4 * 3^24, about 1.1e12, and PerlinNoise::noise takes int(floor(x)) (Perlin.h:18-20), undefined from 2^31 on.  mr_noise.h
// defines every coordinate that is NaN or reaches 2^30 as "noise 0, counted", which alone would count nearly every petal hit.
// But when ALL coordinates of an evaluation are whole numbers the result is +-0 whatever the conversion yields: the fractions
// are 0, so every grad is +-0 and every lerp weight is 0 -- and every float from 2^23 on is whole, and z is 0 throughout.  So
//   an evaluation all of whose coordinates are whole (finite) numbers contributes 0 and is NOT counted;
//   an evaluation with a coordinate that is NaN or reaches 2^30 and another that is not whole is undefined in the reference:
//   it contributes 0 and IS counted (perlin_noise of mr_noise.h, as before).
// On uniform (u, v) in [0, 1)^2 about 0.4 % of the lookups meet an octave of the second kind (tests/test_solid_textures.py).
// P == pivot gives NaN coordinates (0 * (1 / 0)), an acos argument a rounding above 1 gives NaN: they run through the
// reference's own arithmetic (std::min / std::max as uv_min / uv_max) and are counted by the same rule, NaN not being whole.
#pragma once

#include <hip/hip_runtime.h>

#include "miro_math.h"
#include "mr_noise.h"
#include "mr_procedural_body.h"
#include "mr_uv.h"

namespace mr {
namespace {

enum : uint32_t { kTexPetal = 4u, kTexLeaf = 5u, kTexFlowerCenter = 6u };          // MR_TEX_PETAL, MR_TEX_LEAF, MR_TEX_FLOWER_CENTER

__device__ __forceinline__ bool noise_coord_whole(float c) { return c == floorf(c) && fabsf(c) < __builtin_inff(); }

// PerlinNoise::noise under the whole-number rule above
__device__ __forceinline__ float perlin_noise_whole(const NoiseTables &t, float x, float y, float z, bool &ok) {
    if (noise_coord_whole(x) && noise_coord_whole(y) && noise_coord_whole(z)) return 0.0f;
    return perlin_noise(t, x, y, z, ok);
}

// generateNoise (Texture.h:20-37) with z = 0 under the whole-number rule, for a wave-uniform `iterations`, frequency_increase >= 1
// and a last frequency whose products with the coordinates stay finite (PetalTexture's two calls: 4 * 2^9 and 4 * 3^24 on
// |u|, |v| <= 1).  An octave both of whose scaled coordinates have reached 2^23 contributes nothing, and neither does any later
// one, the frequency only growing: once that holds in every lane the wave leaves the Perlin evaluations.  max_val sums every
// amplitude all the same.
__device__ __forceinline__ float turbulence_whole(const NoiseTables &t, float x, float y, float initial_frequency, float frequency_increase,
                                                  float amplitude_falloff, int iterations, bool &ok) {
    float amplitude = 1, frequency = initial_frequency, value = 0, max_val = 0;
    int i = 0;
#pragma unroll 1
    for (; i < iterations; i++) {
        const float xf = x * frequency, yf = y * frequency;
        if (__all(fabsf(xf) >= 0x1p23f && fabsf(yf) >= 0x1p23f)) break;
        value += amplitude * perlin_noise_whole(t, xf, yf, 0.0f * frequency, ok);
        max_val += amplitude;
        frequency *= frequency_increase;
        amplitude *= amplitude_falloff;
    }
#pragma unroll 1
    for (; i < iterations; i++) {
        max_val += amplitude;
        amplitude *= amplitude_falloff;
    }
    return value / max_val;
}

// std::min(pow(turb / 0.1f, 0.85f) * 1.5f, 1.0f) (Texture.cpp:497,500)
__device__ __forceinline__ float petal_turb(float turb) { return uv_min(mm_powf(turb / 0.1f, 0.85f) * 1.5f, 1.0f); }

// PetalTexture::lookup3D (Texture.cpp:447-505).  coords: (u, v, dist) of :465-492, the coordinates the noise is evaluated at and
// the blend factor.
__device__ __forceinline__ void petal_color(const NoiseTables &nt, const float pivot[3], float radius, const float P[3], float rgb[3],
                                            float coords[3], bool &ok) {
    constexpr float kPI = 3.1415926535897932384626433832795028841972f;            // Miro.h:10
    const float base_highlight[3] = {(float)0.2, 0.f, (float)0.8}, tip_highlight[3] = {(float)0.8, (float)0.5, 1.f};     // :457-463
    const float base_depression[3] = {(float)0.2, (float)0.0, (float)0.5}, tip_depression[3] = {(float)0.3, (float)0.15, (float)0.75};
    const float base_color[3] = {(float)0.1, (float)0.0, (float)0.6}, tip_color[3] = {(float)0.6, (float)0.3, (float)1.0};
    float px = P[0] - pivot[0], py = P[1] - pivot[1], pz = P[2] - pivot[2];                                             // :465
    const float len = sqrtf((px * px + py * py) + pz * pz);                                                             // :466
    const float dist = len / radius;                                                                                    // :467
    const float inv = 1.0f / len;                                                  // :476, Vector3::operator/=: *= 1 / length
    px *= inv; py *= inv; pz *= inv;
    // the three dot products with north = (0, 1, 0), equator = (1, 0, 0) and cross(north, equator) = (0, 0, -1) as Vector3.h:242-246
    // forms them: a component that is not finite reaches the sum through its product with 0
    const float phi = mm_acosf(-((0.0f * px + 1.0f * py) + 0.0f * pz));                                                 // :477
    const float v = phi / kPI;                                                                                          // :478
    const float theta = mm_acosf((px * 1.0f + py * 0.0f) + pz * 0.0f) / (2 * kPI);                                      // :488
    const float u = ((0.0f * px + 0.0f * py) + -1.0f * pz) > 0 ? theta : 1 - theta;                                     // :489-492
    coords[0] = u; coords[1] = v; coords[2] = dist;
    const float high = petal_turb(fabsf(turbulence_whole(nt, u, (float)((double)v * 0.25), 4, 2, (float)0.9, 10, ok)));  // :496-497
    const float low = petal_turb(fabsf(turbulence_whole(nt, u, v, 4, 3, (float)0.9, 25, ok)));                           // :499-500
    for (int c = 0; c < 3; c++) {
        const float diffuse = (1 - dist) * base_color[c] + dist * tip_color[c];                                         // :472-474
        const float highlight = (1 - dist) * base_highlight[c] + dist * tip_highlight[c];
        const float depression = (1 - dist) * base_depression[c] + dist * tip_depression[c];
        rgb[c] = (diffuse * high + highlight * (1 - high)) * 0.5f + (diffuse * low + depression * (1 - low)) * 0.5f;    // :502
    }
}

// powf(x, 30.0f) for x >= 0 or NaN: exp(30 ln x) in double, rounded once.  The product is clamped to +-700, mm_exp's range:
// beyond it the float result is 0 or infinity either way (an infinite x takes this road too).  NaN for a NaN, as libm.
__device__ __forceinline__ float powf30(float x) {
    if (x == 0.0f) return 0.0f;
    if (!(x > 0.0f)) return __uint_as_float(0x7fc00000u);
    double z = 30.0 * mm_log((double)x);
    z = z < -700.0 ? -700.0 : (z > 700.0 ? 700.0 : z);
    return (float)mm_exp(z);
}

// FlowerCenterTexture::lookup3D (Texture.h:261-276): no noise
__device__ __forceinline__ void flower_center_color(const float pivot[3], float radius, const float P[3], float rgb[3]) {
    const float dx = P[0] - pivot[0], dy = P[1] - pivot[1], dz = P[2] - pivot[2];
    const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);                                                            // :265
    const float fraction = uv_max(uv_min(powf30(dist / radius), 1.0f), 0.0f);                                           // :266
    const float max_red = 0.92f, max_green = 0.71f, min_red = 0.31f, min_green = 0.18f;
    rgb[0] = uv_min((1.0f - fraction) * min_red + fraction * max_red, 1.0f);                                            // :271-272
    rgb[1] = uv_min((1.0f - fraction) * min_green + fraction * max_green, 1.0f);
    rgb[2] = 0.1f;
}

// lookup3D of a UVW texture (kind: its MR_TEX_*, q1 / q2: the second and third float4 of its record -- pivot and scale, radius) at
// P.  LeafTexture's is StemTexture::lookup2D's body at (P.x, P.y) (Texture.h:230-250).  coords is written for a PETAL alone.
__device__ __forceinline__ void solid_color(const NoiseTables &nt, uint32_t kind, const float4 q1, const float4 q2, const float P[3],
                                            float rgb[3], float coords[3], bool &ok) {
    const float pivot[3] = {q1.x, q1.y, q1.z};
    if (kind == kTexLeaf) stem_color(nt, q1.w, P[0], P[1], rgb, ok);
    else if (kind == kTexPetal) petal_color(nt, pivot, q2.x, P, rgb, coords, ok);
    else flower_center_color(pivot, q2.x, P, rgb);
}

}  // namespace
}  // namespace mr
