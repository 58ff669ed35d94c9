// mr_tonemap.h -- the tone map of one channel value, once: mr_tonemap's kernel (mr_shade.hip) and mr_finish_image's second kernel
// (mr_finish_image.hip) call this definition, so their bytes are the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mr {

__device__ __forceinline__ uint8_t tonemap_byte(float v) {
    v = 1.0f / (1.0f + expf(-(6.0f * v - 3.0f)));                   // sigmoid(6v-3), Scene.cpp:89, Utility.h:19-22
    const float m = 255.0f * v;                                     // Image.cpp:44-50
    return m > 255.0f ? 255 : (uint8_t)m;
}

}  // namespace mr
