// mr_environment_body.h -- Scene::getEnvironmentMap's lookup (Scene.cpp:657-688) as __device__ functions: the texture
// coordinates of a direction, the four texels LoadedTexture::lookup (Texture.cpp:161-185) reads for them, and the blend.  One
// definition for the two kernels that shade a ray that misses: shade_environment_kernel (mr_environment.hip), which takes the
// texels from the full image or from its low-res copy in LDS, and frame_lights_env_kernel (mr_frame_lights_env.hip), whose eye
// rays read the full image only (env_lookup_full).  The bilinear arithmetic itself is mr_texture.h's, shared with the material
// textures.  Device code only, every operation in fp32 in the reference's order on mm_atan2f / mm_asinf of miro_math.h (the
// units that include this are compiled with -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>

#include "miro_math.h"
#include "mr_internal.h"
#include "mr_recursion.h"
#include "mr_texture.h"

namespace mr {

// Scene.cpp:664-676: the texture coordinates of a direction
__device__ __forceinline__ void env_coords(const float rot[2], float dx, float dy, float dz, float &u, float &v) {
    using rec::kPI;
    float phi = mm_atan2f(dx, dz) + rot[0] + kPI;                       // :665
    float theta = mm_asinf(dy) + rot[1];                                // :666
    if (theta > kPI / 2.0f) {                                           // :667-671
        phi += kPI;
        theta -= 2.0f * (theta - kPI / 2.0f);
    }
    if (phi > 2.0f * kPI) phi -= (2.0f * kPI);                          // :672
    u = phi / (2.0f * kPI);                                             // :675
    v = (float)((double)(theta / kPI) + 0.5);                           // :676 (0.5 is a double)
}

// The texels of a w x h image that the lookup at direction (dx, dy, dz) reads -- columns x1, x2 of rows y1, y2 -- and the two
// error terms.  false: the reference's arithmetic leaves the image (undefined there; the callers define the value as 0 and
// count it); the indices are then not to be used.
__device__ __forceinline__ bool env_texels(const float rot[2], int w, int h, float dx, float dy, float dz, int &x1, int &x2, int &y1,
                                           int &y2, float &xe, float &ye) {
    float u, v;
    env_coords(rot, dx, dy, dz, u, v);
    const bool okx = bilinear_axis(w, u, x1, x2, xe), oky = bilinear_axis(h, v, y1, y2, ye);
    return okx && oky;
}

// Texture.cpp:181 and tonemapValue for the three channels of the four texel records
__device__ __forceinline__ void env_blend(const float4 p11, const float4 p21, const float4 p12, const float4 p22, float xe, float ye,
                                          float max_intensity, float val[3]) {
    val[0] = bilinear_blend(p11.x, p21.x, p12.x, p22.x, xe, ye, max_intensity);
    val[1] = bilinear_blend(p11.y, p21.y, p12.y, p22.y, xe, ye, max_intensity);
    val[2] = bilinear_blend(p11.z, p21.z, p12.z, p22.z, xe, ye, max_intensity);
}

// The lookup of the FULL image (a ray that is not isDiffuse, Scene.cpp:678-681): four dwordx4 fetches.  false: undefined, val
// is left as it was.
__device__ __forceinline__ bool env_lookup_full(const EnvParams &env, float dx, float dy, float dz, float val[3]) {
    const int w = (int)env.W, h = (int)env.H;
    float xe = 0.f, ye = 0.f;
    int x1 = 0, x2 = 0, y1 = 0, y2 = 0;
    if (!env_texels(env.rot, w, h, dx, dy, dz, x1, x2, y1, y2, xe, ye)) return false;
    const float4 *r1 = env.full + (size_t)y1 * w, *r2 = env.full + (size_t)y2 * w;
    env_blend(r1[x1], r1[x2], r2[x1], r2[x2], xe, ye, env.max_intensity, val);
    return true;
}

}  // namespace mr
