// mr_photon_tree.h -- the arithmetic on which the host balance of a photon map (mr_photon.cpp, the yardstick) and the device
// build (mr_photon_build.hip) must agree bit for bit, each piece written once.  Integer and comparison code only, except the
// three subtractions of split_axis, which -ffp-contract=off rounds alike on both sides.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mr {

// the median rule of balance_segment (PhotonMap.cpp:421-430): left-balanced split of [start, end]
__host__ __device__ __forceinline__ int32_t left_balanced_median(int32_t start, int32_t end) {
    const int32_t n = end - start + 1;
    int32_t median = 1;
    while (4 * median <= n) median += median;
    if (3 * median <= n) { median += median; median += start - 1; }
    else median = end - median + 1;
    return median;
}

// the split axis of balance_segment (PhotonMap.cpp:436-441): the longest extent of the running box, ties to the later axis
__host__ __device__ __forceinline__ int split_axis(const float bmin[3], const float bmax[3]) {
    int axis = 2;
    if ((bmax[0] - bmin[0]) > (bmax[1] - bmin[1]) && (bmax[0] - bmin[0]) > (bmax[2] - bmin[2])) axis = 0;
    else if ((bmax[1] - bmin[1]) > (bmax[2] - bmin[2])) axis = 1;
    return axis;
}

// the two direction bytes of Photon_map::store from the truncated scaled angles (PhotonMap.cpp:268-283)
__host__ __device__ __forceinline__ uint8_t theta_byte(int theta) { return theta > 255 ? 255 : (uint8_t)theta; }
__host__ __device__ __forceinline__ uint8_t phi_byte(int phi) { return phi > 255 ? 255 : (phi < 0 ? (uint8_t)(phi + 256) : (uint8_t)phi); }

// ascending uint32 <=> ascending float, -0 == +0; key_float gives the float back (+0 for either zero)
__host__ __device__ __forceinline__ uint32_t order_key(float f) {
    uint32_t b = __builtin_bit_cast(uint32_t, f);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float key_float(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

}  // namespace mr
