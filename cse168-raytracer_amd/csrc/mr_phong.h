// mr_phong.h -- the pieces of Phong::shade (Phong.cpp:44-160) that follow a hit, written once for the batched kernels
// (shadow_rays_kernel, the shade kernels of mr_shade.hip and mr_bounce.hip), the fused frame and level kernels and the
// light-list kernel, so that all of them produce the same bits:
//   shadow_ray_of    the shadow ray towards a point light (Phong.cpp:80-97); shadow_ray_for: towards a light of the list,
//                    point or disc -- one tail (shadow_ray_along) for both
//   light_scale_of   what Phong::shade does with the shadow hit (Phong.cpp:97-113): opaque occluder -> 0,
//                    refractive occluder -> dot(N, l) (0 if negative or < epsilon), no occluder -> 1
//   phong_terms      diffuse term and highlight of a hit (Phong.cpp:116-156) for a material record and a point light;
//                    disc_terms: for a DirectionalAreaLight; highlight_of is the one highlight (:149-156) of all of them
//                    `samples`, where a caller gives it, is the number of shadow rays the light's wattage is divided among
//                    (a SquareLight, Phong.cpp:146 / :154); the callers without it divide by a literal 1, which is no operation
//   phong_combine    the two terms and the light scale put together
//   phong_direct     direct light of an unoccluded hit on the frame's uniform material, with the normal normalised as
//                    Scene::trace leaves it (Scene.cpp:262): phong_terms + phong_combine
//   light_args_of / direct_light_of   the host's mr_light as the kernels take it
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_surface.h"

namespace mr {

constexpr float kPhongEps = 1e-4f;                                               // Miro.h:9
constexpr float kPhongPI = 3.1415926535897932384626433832795028841972f;          // Miro.h:10

struct LightArgs {
    float L[3], color[3], wattage;
};
inline LightArgs light_args_of(const mr_light &light) {
    LightArgs a;
    for (int c = 0; c < 3; c++) { a.L[c] = light.position[c]; a.color[c] = light.color[c]; }
    a.wattage = light.wattage;
    return a;
}

// a point light and the uniform material of mr_shade_direct / mr_render_direct; bg: Scene::m_bgColor
struct DirectLight {
    float L[3], color[3], diffuse[3], bg[3];
    float wattage;
};
inline DirectLight direct_light_of(const mr_light &light, const float diffuse[3]) {
    DirectLight a;
    for (int c = 0; c < 3; c++) { a.L[c] = light.position[c]; a.color[c] = light.color[c]; a.diffuse[c] = diffuse[c]; a.bg[c] = 0.0f; }
    a.wattage = light.wattage;
    return a;
}

// Phong.cpp:84-92 from getLightDirection's l (not normalised) on: falloff = |l|^2, l /= sqrt(falloff);
// Ray(P + l * epsilon, l), tMin = 0, tMax = sqrt(falloff)
__device__ __forceinline__ void shadow_ray_along(const float P[3], float lx, float ly, float lz, float4 &a, float4 &b) {
    const float falloff = (lx * lx + ly * ly) + lz * lz;
    const float len = sqrtf(falloff);
    const float inv = 1.0f / len;                                  // l /= sqrt(falloff)
    lx *= inv; ly *= inv; lz *= inv;
    a = make_float4(P[0] + lx * kPhongEps, P[1] + ly * kPhongEps, P[2] + lz * kPhongEps, 0.0f);
    b = make_float4(lx, ly, lz, len);
}
// PointLight::getLightDirection: l = L - P
__device__ __forceinline__ void shadow_ray_of(const float P[3], float Lx, float Ly, float Lz, float4 &a, float4 &b) {
    shadow_ray_along(P, Lx - P[0], Ly - P[1], Lz - P[2], a, b);
}
// ... of a light of the list.  DirectionalAreaLight::getLightDirection ignores the sampled origin: l = -normal
__device__ __forceinline__ void shadow_ray_for(const ShadeLight &lt, const float P[3], float4 &sa, float4 &sb) {
    if (lt.kind == MR_LIGHT_DISC) shadow_ray_along(P, -lt.normal[0], -lt.normal[1], -lt.normal[2], sa, sb);
    else shadow_ray_of(P, lt.position[0], lt.position[1], lt.position[2], sa, sb);
}

// The factor Phong::shade puts on the light behind a shadow hit (Phong.cpp:97-113).  sa / sb: the shadow ray; sh: its
// hit record (prim = MR_MISS: no occluder).
__device__ __forceinline__ float light_scale_of(const rec::MeshMat &m, const float4 sa, const float4 sb, const float4 sh) {
    const uint32_t prim = __float_as_uint(sh.y);
    float scale = 1.0f;
    if (prim != MR_MISS) {
        scale = 0.0f;
        const float *om = rec::material_of(m, prim);
        if (rec::any_pos(om + 6)) {                                       // refractive occluder (Phong.cpp:99-113)
            float P[3], N[3];
            rec::surface_point_od(m, sa.x, sa.y, sa.z, sb.x, sb.y, sb.z, sh.x, prim, sh.z, sh.w, P, N);
            const float d = (N[0] * sb.x + N[1] * sb.y) + N[2] * sb.z;
            if (!(d < 0) && !(d < kPhongEps)) scale = d;
        }
    }
    return scale;
}

// The specular highlight (Phong.cpp:149-156).  l: the normalised direction to the light, N normalised, (dx, dy, dz) the
// direction of the ray that produced the hit, f2 the light's falloff factor.
//
// ZERO_GUARD (the fused frame): powf(x, 500.0f) is some 125 VALU instructions, and for nearly every
// sample its result is exactly +0 -- x^500 is below half the smallest denormal, 2^-150, for x < 2^-0.3 = 0.8123, that is
// outside a cone of 36 degrees around the mirror direction.  A lane is SURE of the zero when its clamped e is below
// kHighlightZeroBelow; when every lane that is here is sure, e = +0 is written without the call.
//   * The constant: tools/pow_zero_probe.hip runs this device's powf(x, 500.0f) -- through highlight_pow below, the very call of
//     this function -- on every float of [0, 1] and prints the largest X with a bitwise +0 for every float of [0, X]
//     (profiles/pow_zero_probe.log: X = 0x1.a0733cp-1 = 0.8133792).  0.75 is below it; 0.75^500 = 2^-207.5 lies 57 binades
//     under the rounding boundary, so the last bits of powf's log2 and exp2 have no say.
//   * The clamp comes first, as it always did: a negative e and -0 are +0 after fmaxf, and 0^500 = +0 is in the probe's range.
//   * A NaN e leaves the clamp as 1 (fminf and fmaxf return their other operand), 1 < 0.75 is false: never sure.
//   * Inactive lanes: the ballot of the compare holds no bit of a lane that is not here, and is compared with the ballot of
//     `true`, the mask of the lanes that are (inside the caller's `if (hit)`, and `if (shininess < inf)` where that is a branch).
//     A lane without a hit neither blocks the skip nor receives a value.
//   * Otherwise the whole wave calls powf on the same operand as without the guard.  What follows (:154) is the same
//     instructions on +0 either way.
constexpr float kHighlightZeroBelow = 0.75f;
__device__ __forceinline__ float highlight_pow(float e) { return powf(e, 500.0f); }
template <bool ZERO_GUARD = false>
__device__ __forceinline__ float highlight_of(const float l[3], const float N[3], float dx, float dy, float dz, float f2, float wattage,
                                              float samples = 1.0f) {
    const float two = 2 * ((l[0] * N[0] + l[1] * N[1]) + l[2] * N[2]);
    const float rx = -l[0] + two * N[0], ry = -l[1] + two * N[1], rz = -l[2] + two * N[2];
    float e = (-dx * rx + -dy * ry) + -dz * rz;
    e = fmaxf(0.0f, fminf(1.0f, e));
    if (ZERO_GUARD && __builtin_amdgcn_ballot_w64(e < kHighlightZeroBelow) == __builtin_amdgcn_ballot_w64(true)) e = 0.0f;
    else e = highlight_pow(e);
    return fmaxf(0.0f, e * f2 * wattage / samples);                // :154
}
// Phong.cpp:146-156 once the light has given l, nDotL and its falloff factor f2: diffuse[c] (to be multiplied by the light
// scale, :146) and the highlight (added unscaled; 0 for a material of infinite shininess)
// dc: the hit's diffuseColor (Phong.cpp:51-56) -- the texture's colour for a TexturedPhong (mr_texture.h), m_diffuse itself for a
// plain Phong (Phong::diffuse2D), which is the second form.  The highlight does not see it.
template <bool ZERO_GUARD = false>
__device__ __forceinline__ void lit_terms(const float color[3], float wattage, const float *mt, const float *dc, const float N[3],
                                          const float l[3], float nDotL, float f2, float dx, float dy, float dz, float diffuse[3],
                                          float &highlight, float samples = 1.0f) {
    const float diff = fmaxf(0.0f, nDotL * f2 * wattage / samples);
    for (int c = 0; c < 3; c++) diffuse[c] = color[c] * (diff * dc[c] * mt[c]);               // :146
    highlight = mt[9] < __builtin_huge_valf() ? highlight_of<ZERO_GUARD>(l, N, dx, dy, dz, f2, wattage, samples) : 0.0f;
}
__device__ __forceinline__ void lit_terms(const float color[3], float wattage, const float *mt, const float N[3], const float l[3],
                                          float nDotL, float f2, float dx, float dy, float dz, float diffuse[3], float &highlight) {
    lit_terms(color, wattage, mt, mt, N, l, nDotL, f2, dx, dy, dz, diffuse, highlight);
}

// Phong::shade's direct light at a hit (Phong.cpp:116-156) for a point light at L, in lit_terms' two parts.  The shaded value
// of a hit with light scale s != 0 is diffuse[c] * s + highlight, and 0 for s == 0 (Phong.cpp:100-103 skips the light).
// mt: the hit's material record, dc its diffuseColor (lit_terms; the forms without dc are a plain Phong's); N normalised;
// (dx, dy, dz) the direction of the ray that produced the hit.
template <bool ZERO_GUARD = false>
__device__ __forceinline__ void phong_terms(const float L[3], const float color[3], float wattage, const float *mt, const float *dc,
                                            const float P[3], const float N[3], float dx, float dy, float dz, float diffuse[3],
                                            float &highlight, float samples = 1.0f) {
    float l[3] = {L[0] - P[0], L[1] - P[1], L[2] - P[2]};
    const float falloff = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2];
    const float inv = 1.0f / sqrtf(falloff);
    l[0] *= inv; l[1] *= inv; l[2] *= inv;
    const float nDotL = (N[0] * l[0] + N[1] * l[1]) + N[2] * l[2];
    const float f2 = 1.0f / (falloff * 4.0f * kPhongPI * kPhongPI);                           // :140
    lit_terms<ZERO_GUARD>(color, wattage, mt, dc, N, l, nDotL, f2, dx, dy, dz, diffuse, highlight, samples);
}
template <bool ZERO_GUARD = false>
__device__ __forceinline__ void phong_terms(const float L[3], const float color[3], float wattage, const float *mt, const float P[3],
                                            const float N[3], float dx, float dy, float dz, float diffuse[3], float &highlight,
                                            float samples = 1.0f) {
    phong_terms<ZERO_GUARD>(L, color, wattage, mt, mt, P, N, dx, dy, dz, diffuse, highlight, samples);
}
__device__ __forceinline__ void phong_terms(const LightArgs &a, const float *mt, const float *dc, const float P[3], const float N[3],
                                            float dx, float dy, float dz, float diffuse[3], float &highlight) {
    phong_terms(a.L, a.color, a.wattage, mt, dc, P, N, dx, dy, dz, diffuse, highlight);
}
template <bool ZERO_GUARD = false>
__device__ __forceinline__ void phong_terms(const LightArgs &a, const float *mt, const float P[3], const float N[3], float dx,
                                            float dy, float dz, float diffuse[3], float &highlight) {
    phong_terms<ZERO_GUARD>(a.L, a.color, a.wattage, mt, mt, P, N, dx, dy, dz, diffuse, highlight);
}
// Phong.cpp:121-136 for a DirectionalAreaLight.  l: the normalised direction (the shadow ray's).  Returns false when the hit
// lies outside the disc's cylinder (:133, the light is skipped); otherwise lit_terms with nDotL = dot(N, -normal) on the
// normal as given and falloff = 1 / PI.
__device__ __forceinline__ bool disc_terms(const ShadeLight &lt, const float *mt, const float *dc, const float P[3], const float N[3],
                                           const float l[3], float dx, float dy, float dz, float diffuse[3], float &highlight) {
    const float *n = lt.normal;
    const float nDotL = (N[0] * -n[0] + N[1] * -n[1]) + N[2] * -n[2];                          // :128
    const float t = ((n[0] * (lt.position[0] - P[0]) + n[1] * (lt.position[1] - P[1])) + n[2] * (lt.position[2] - P[2])) / -1.0f;   // :132
    const float qx = (P[0] - n[0] * t) - lt.position[0], qy = (P[1] - n[1] * t) - lt.position[1], qz = (P[2] - n[2] * t) - lt.position[2];
    if ((qx * qx + qy * qy) + qz * qz > lt.radius * lt.radius) return false;                   // :133
    lit_terms(lt.color, lt.wattage, mt, dc, N, l, nDotL, 1.0f / kPhongPI, dx, dy, dz, diffuse, highlight);   // :135
    return true;
}
__device__ __forceinline__ bool disc_terms(const ShadeLight &lt, const float *mt, const float P[3], const float N[3], const float l[3],
                                           float dx, float dy, float dz, float diffuse[3], float &highlight) {
    return disc_terms(lt, mt, mt, P, N, l, dx, dy, dz, diffuse, highlight);
}

// The light-list kernels of point and disc lights add a light's two terms to L at once, L += diffuse * scale + highlight.
// Phong.cpp:146 and :155 add them one after the other, L += diffuse * scale; L += highlight, and so does the square-light
// kernel (mr_distribution.hip).  Once L != 0 the two forms round differently; each kernel family keeps its own.
__device__ __forceinline__ void phong_combine(const float diffuse[3], float highlight, float scale, float out[3]) {
    if (scale == 0.0f) { out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; return; }
    for (int c = 0; c < 3; c++) out[c] = diffuse[c] * scale + highlight;
}

// The uniform-material callers' form: N is the un-normalised HitInfo::N and is normalised in place; the material is Phong's
// default but for its diffuse colour (shininess 1 < infinity: the highlight is on), the light is not occluded.
template <bool ZERO_GUARD = false>
__device__ __forceinline__ void phong_direct(const DirectLight &a, const float P[3], float N[3], float dx, float dy, float dz,
                                             float out[3]) {
    normalize3(N);                                                 // Scene.cpp:262
    const float mt[11] = {a.diffuse[0], a.diffuse[1], a.diffuse[2], 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.0f, 1.0f};
    float diffuse[3], highlight;
    phong_terms<ZERO_GUARD>(a.L, a.color, a.wattage, mt, P, N, dx, dy, dz, diffuse, highlight);
    phong_combine(diffuse, highlight, 1.0f, out);
}

}  // namespace mr
