// mr_bvh_rules.h -- the arithmetic of BVH::build (BVH.cpp:60-339) that decides the tree, each rule written once for the host
// builder (mr_build.cpp) and the device builder (mr_bvh_build.hip): the object table, the cost of a side, the plane of a
// bisection step, the two move predicates, the boundary test and the padding.  Every fp32 operation rounds on its own (both
// translation units are built with -ffp-contract=off); nothing here may become an fmaf.
#pragma once

#include <hip/hip_runtime.h>

namespace mr {
namespace bvh {

constexpr float kEps = 1e-4f;   // Miro.h:9
constexpr int kMaxDepth = 32;   // BVH.h:57
constexpr int kBisectSteps = 32;

struct Box {
    float lo[3], hi[3];
    __host__ __device__ void clear() { for (int k = 0; k < 3; k++) { lo[k] = __builtin_inff(); hi[k] = -__builtin_inff(); } }
    // the reference's compare-and-assign; the device's fminf / fmaxf reductions may differ from it in the sign of a zero
    // corner, which no stored value sees: corners are stored padded and the unpadded box is read by differences and comparisons
    __host__ __device__ void grow(const float plo[3], const float phi[3]) {
        for (int k = 0; k < 3; k++) {
            if (hi[k] < phi[k]) hi[k] = phi[k];
            if (lo[k] > plo[k]) lo[k] = plo[k];
        }
    }
    // 2 * sum of pairwise extents, accumulated in the order (y,z), (z,x), (x,y) (BVH.cpp:41-51)
    __host__ __device__ float area2() const {
        float a = 0;
        for (int d = 0; d < 3; d++) {
            int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
            a += (hi[d1] - lo[d1]) * (hi[d2] - lo[d2]);
        }
        return 2 * a;
    }
    // a box handed down by the parent, or "compute it yourself"
    __host__ __device__ bool cleared() const { return lo[0] == __builtin_inff(); }
    __host__ __device__ void pad() { for (int k = 0; k < 3; k++) { lo[k] -= kEps; hi[k] += kEps; } }
    // Vector3 bestCorners[2][2] default to (0,1,2) (BVH.cpp:173)
    __host__ __device__ void set_default_corners() { for (int k = 0; k < 3; k++) { lo[k] = (float)k; hi[k] = (float)k; } }
};

// ---- the object table (Triangle.cpp:41-48,97-118; Sphere.h:19-21): bounds and centre of one object
__host__ __device__ inline void triangle_ref(const float *a, const float *b, const float *c, float lo[3], float hi[3], float ctr[3]) {
    const float third = 1.0f / 3.0f;      // Vector3::operator/(3): multiply by rounded 1/3
    for (int k = 0; k < 3; k++) {
        float mn = a[k], mx = a[k];
        if (b[k] < mn) mn = b[k];
        if (b[k] > mx) mx = b[k];
        if (c[k] < mn) mn = c[k];
        if (c[k] > mx) mx = c[k];
        lo[k] = mn; hi[k] = mx;
        float ba = b[k] - a[k], ca = c[k] - a[k];
        ctr[k] = (a[k] + ba * third) + ca * third;     // Triangle.cpp:45-47
    }
}
__host__ __device__ inline void sphere_ref(const float *sp, float lo[3], float hi[3], float ctr[3]) {   // m_center -/+ Vector3(m_radius)
    for (int k = 0; k < 3; k++) { lo[k] = sp[k] - sp[3]; hi[k] = sp[k] + sp[3]; ctr[k] = sp[k]; }
}

// ---- one axis of the search (BVH.cpp:178-302)
__host__ __device__ inline float side_cost(const Box &b, int n) { return n == 0 ? 0.0f : (float)n * b.area2(); }
__host__ __device__ inline int heavier_side(float c0, float c1) { return c0 > c1 ? 0 : 1; }      // ties -> right
__host__ __device__ inline float mid_plane(float lo, float hi) { return (lo + hi) / 2.0f; }
__host__ __device__ inline int side_of(float ctr, float plane) { return ctr < plane ? 0 : 1; }   // first classification, final partition
// an object of the heavy side moves to the light side when the new plane has passed its centre -- strictly: a centre on the
// plane stays where it is
__host__ __device__ inline bool moves(int heavy, float ctr, float plane) { return heavy == 0 ? ctr > plane : ctr < plane; }
// a moved object touched the heavy box (as it was before the step): that box has to be computed again from what remains
__host__ __device__ inline bool leaves_boundary(const float plo[3], const float phi[3], const Box &heavy) {
    for (int k = 0; k < 3; k++)
        if (phi[k] >= heavy.hi[k] - kEps || plo[k] <= heavy.lo[k] + kEps) return true;
    return false;
}

}  // namespace bvh
}  // namespace mr
