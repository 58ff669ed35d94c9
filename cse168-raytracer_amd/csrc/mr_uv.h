// mr_uv.h -- Object::toUVCoordinates(hit.P) of a hit (Phong.cpp:51-56 hands it to Texture::lookup2D), next to mr_surface.h,
// which gives the hit's P.  Device code only.  Every operation is a single-rounded fp32 operation in the reference's order
// (the units that include this are compiled with -ffp-contract=off).
//
//   plane     (P.x, P.z)                                                                   Plane.cpp:50-60
//             -- also Object's default (Object.h:37)
//   sphere    dir = normalize(P - centre);  u = atan2(dir.x, dir.z) / (2 PI) + 0.5;          Sphere.cpp:83-95
//             v = max(-1, min(1, asin(dir.y))) / PI + 0.5.  The clamp is on the ANGLE, to +-1 radian (asin never leaves
//             +-PI/2, so it cuts the poles off): v stays inside about [0.18, 0.82].  Reproduced, not repaired.
//   triangle  a mesh without texture coordinates: (0, 0) (tex_coord2d_t()).  Otherwise the barycentric coordinates of P are
//             recomputed by Cramer's rule on a projection that drops one axis by the reference's own rule -- on the SIGNED,
//             un-normalised cross(B-A, C-A): normal.x > normal.z -> (i, j) = (2, 1), else normal.y > normal.z -> (0, 2), else
//             (0, 1) -- and the vertices' texture coordinates interpolated                  Triangle.cpp:172-222
//
// The reading of the sphere's two lines is the one mr_environment.hip takes for Scene.cpp:664-676: the unqualified atan2 /
// asin on float arguments are the float overloads (<cmath> under `using namespace std`), evaluated as mm_atan2f / mm_asinf
// of miro_math.h (the double function rounded to float: the same bits in a host restatement); the quotient by 2.0f * PI or PI
// is a float operation; `+ 0.5` adds a DOUBLE constant, so the quotient is promoted, the sum formed in double and rounded
// to float by the assignment to tex_coord2d_t's float member.
#pragma once

#include <hip/hip_runtime.h>

#include "miro_math.h"
#include "mr_internal.h"
#include "mr_surface.h"

namespace mr {

// a scene's mesh with its texture coordinates
struct UvPtrs {
    SurfacePtrs s;
    const float *t;           // uv pairs; nullptr: no object of the scene has texture coordinates
    const uint32_t *ti;       // 3 per object, kNoTexcoord = the object's mesh has none
};

inline UvPtrs uv_ptrs(const DeviceScene &ds) {
    UvPtrs m;
    m.s = surface_ptrs(ds); m.t = ds.texcoords; m.ti = ds.ti;
    return m;
}

// std::max(a, b) = a < b ? b : a and std::min(a, b) = b < a ? b : a: a NaN FIRST argument stays
__device__ __forceinline__ float uv_max(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ float uv_min(float a, float b) { return b < a ? b : a; }

// Triangle.cpp:16
__device__ __forceinline__ float uv_det(float a, float b, float c, float d) { return a * d - b * c; }

// toUVCoordinates(P) of the object `prim` (a hit record's prim, not MR_MISS)
__device__ __forceinline__ void uv_of(const UvPtrs &m, uint32_t prim, const float P[3], float &u, float &v) {
    constexpr float kPI = 3.1415926535897932384626433832795028841972f;            // Miro.h:10
    if (m.s.planes && (prim & kPlaneBit)) { u = P[0]; v = P[2]; return; }         // Plane.cpp:52,59
    const size_t t3 = 3 * (size_t)prim;
    if (m.s.spheres && m.s.vi[t3] == kSphereSlot) {
        const float4 sp = m.s.spheres[m.s.vi[t3 + 1]];
        float dir[3] = {P[0] - sp.x, P[1] - sp.y, P[2] - sp.z};                   // Sphere.cpp:86-87
        normalize3(dir);
        u = (float)((double)(mm_atan2f(dir[0], dir[2]) / (2.0f * kPI)) + 0.5);    // :90
        const float a = uv_max(-1.0f, uv_min(1.0f, mm_asinf(dir[1])));            // :92
        v = (float)((double)(a / kPI) + 0.5);
        return;
    }
    u = 0.0f; v = 0.0f;
    if (!m.t) return;                                                             // Triangle.cpp:174-175
    const uint32_t ta = m.ti[t3], tb = m.ti[t3 + 1], tc = m.ti[t3 + 2];
    if (ta == kNoTexcoord) return;
    const uint32_t ia = m.s.vi[t3], ib = m.s.vi[t3 + 1], ic = m.s.vi[t3 + 2];
    float A[3], B[3], C[3], p[3];
    for (int c = 0; c < 3; c++) {
        A[c] = m.s.v[3 * (size_t)ia + c];
        B[c] = m.s.v[3 * (size_t)ib + c] - A[c];                                  // :192,:203
        C[c] = m.s.v[3 * (size_t)ic + c] - A[c];                                  // :192,:204
        p[c] = P[c] - A[c];                                                       // :202
    }
    const float nx = B[1] * C[2] - B[2] * C[1], ny = B[2] * C[0] - B[0] * C[2], nz = B[0] * C[1] - B[1] * C[0];   // :193
    int i = 0, j = 1;
    if (nx > nz) i = 2;                                                           // :197-200
    else if (ny > nz) j = 2;
    const float pi = i == 2 ? p[2] : p[0], Bi = i == 2 ? B[2] : B[0], Ci = i == 2 ? C[2] : C[0];
    const float pj = j == 2 ? p[2] : p[1], Bj = j == 2 ? B[2] : B[1], Cj = j == 2 ? C[2] : C[1];
    const float detPC = uv_det(pi, Ci, pj, Cj);                                   // :207-209
    const float detBP = uv_det(Bi, pi, Bj, pj);
    const float detBC = uv_det(Bi, Ci, Bj, Cj);
    const float beta = uv_max(detPC / detBC, 0.f);                                // :211-214
    const float gamma = uv_max(detBP / detBC, 0.f);
    const float alpha = uv_max(1 - (beta + gamma), 0.f);
    u = (alpha * m.t[2 * (size_t)ta] + beta * m.t[2 * (size_t)tb]) + gamma * m.t[2 * (size_t)tc];               // :218-219
    v = (alpha * m.t[2 * (size_t)ta + 1] + beta * m.t[2 * (size_t)tb + 1]) + gamma * m.t[2 * (size_t)tc + 1];
}

}  // namespace mr
