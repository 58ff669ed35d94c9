// mr_noise.h -- the two noise functions under the reference's procedural textures, on the device: PerlinNoise::noise
// (lib/include/Perlin.h:16-51), generateNoise (Texture.h:20-37) and WorleyNoise::noise2D of order 3 (lib/src/Worley.cpp:95-173,
// 367-436).  Both are pure functions of their arguments over two fixed 256-entry tables -- nothing here is seeded by rand().
// Device code only; every operation is a single-rounded fp32 operation in the reference's order (the unit that includes this
// is compiled with -ffp-contract=off), with the reference's own promotions to double where its constants are double.
//
// The tables are integer data from their published sources: the permutation of Ken Perlin's "Improved Noise" (2002) and the
// Poisson-count table of mean 2.5 of Steven Worley's cellular basis function (1996; "Texturing and Modeling", 3rd ed.).  A
// workgroup stages both in LDS once (512 bytes, stage_noise_tables): the indices differ from lane to lane, which is what LDS
// serves and the scalar cache does not.  The reference's permutation has 512 entries, the 256 twice over; its largest index
// is 511, so p[i & 255] of the 256 reads the same value.
//
// What the reference leaves undefined is defined here: a coordinate that is NaN or whose magnitude reaches 2^30 fails
// int(floor()) there; it gives noise 0 (F = 0, id = 0) here and `ok` is cleared, so that the caller can count it.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "miro_math.h"

namespace mr {
namespace {

alignas(16) __device__ const uint8_t kNoiseTables[512] = {
    // Perlin 2002, the permutation
    151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240, 21, 10, 23, 190,
    6, 148, 247, 120, 234, 75, 0, 26, 197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88, 237, 149, 56, 87, 174, 20, 125,
    136, 171, 168, 68, 175, 74, 165, 71, 134, 139, 48, 27, 166, 77, 146, 158, 231, 83, 111, 229, 122, 60, 211, 133, 230, 220, 105,
    92, 41, 55, 46, 245, 40, 244, 102, 143, 54, 65, 25, 63, 161, 1, 216, 80, 73, 209, 76, 132, 187, 208, 89, 18, 169, 200, 196, 135,
    130, 116, 188, 159, 86, 164, 100, 109, 198, 173, 186, 3, 64, 52, 217, 226, 250, 124, 123, 5, 202, 38, 147, 118, 126, 255, 82, 85,
    212, 207, 206, 59, 227, 47, 16, 58, 17, 182, 189, 28, 42, 223, 183, 170, 213, 119, 248, 152, 2, 44, 154, 163, 70, 221, 153, 101,
    155, 167, 43, 172, 9, 129, 22, 39, 253, 19, 98, 108, 110, 79, 113, 224, 232, 178, 185, 112, 104, 218, 246, 97, 228, 251, 34, 242,
    193, 238, 210, 144, 12, 191, 179, 162, 241, 81, 51, 145, 235, 249, 14, 239, 107, 49, 192, 214, 31, 181, 199, 106, 157, 184, 84,
    204, 176, 115, 121, 50, 45, 127, 4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29, 24, 72, 243, 141, 128, 195, 78, 66, 215, 61,
    156, 180,
    // Worley 1996, feature points per cell: an approximate Poisson distribution of mean 2.5
    4, 3, 1, 1, 1, 2, 4, 2, 2, 2, 5, 1, 0, 2, 1, 2, 2, 0, 4, 3, 2, 1, 2, 1, 3, 2, 2, 4, 2, 2, 5, 1, 2, 3, 2, 2, 2, 2, 2, 3, 2, 4, 2, 5, 3, 2, 2, 2,
    5, 3, 3, 5, 2, 1, 3, 3, 4, 4, 2, 3, 0, 4, 2, 2, 2, 1, 3, 2, 2, 2, 3, 3, 3, 1, 2, 0, 2, 1, 1, 2, 2, 2, 2, 5, 3, 2, 3, 2, 3, 2, 2, 1, 0, 2, 1, 1,
    2, 1, 2, 2, 1, 3, 4, 2, 2, 2, 5, 4, 2, 4, 2, 2, 5, 4, 3, 2, 2, 5, 4, 3, 3, 3, 5, 2, 2, 2, 2, 2, 3, 1, 1, 4, 2, 1, 3, 3, 4, 3, 2, 4, 3, 3, 3, 4,
    5, 1, 4, 2, 4, 3, 1, 2, 3, 5, 3, 2, 1, 3, 1, 3, 3, 3, 2, 3, 1, 5, 5, 4, 2, 2, 4, 1, 3, 4, 1, 5, 3, 3, 5, 3, 4, 3, 2, 2, 1, 1, 1, 1, 1, 2, 4, 5,
    4, 5, 4, 2, 1, 5, 1, 1, 2, 3, 3, 3, 2, 5, 2, 3, 3, 2, 0, 2, 1, 1, 4, 2, 1, 3, 2, 1, 2, 2, 3, 2, 5, 5, 3, 4, 5, 5, 2, 4, 4, 5, 3, 2, 2, 2, 1, 4,
    2, 3, 3, 4, 2, 5, 4, 2, 4, 2, 2, 2, 4, 5, 3, 2};

// the two tables in LDS: s_perm[256] then s_poisson[256]
struct NoiseTables {
    const uint8_t *perm, *poisson;
};

// called once by every thread of a workgroup of at least 128 threads, before the first noise call
__device__ __forceinline__ NoiseTables stage_noise_tables(uint32_t (&s_tab)[128]) {
    if (threadIdx.x < 128) s_tab[threadIdx.x] = reinterpret_cast<const uint32_t *>(kNoiseTables)[threadIdx.x];
    __syncthreads();
    NoiseTables t;
    t.perm = reinterpret_cast<const uint8_t *>(s_tab);
    t.poisson = t.perm + 256;
    return t;
}

// int(floor(c)) is defined: c is a number below 2^30 in magnitude
__device__ __forceinline__ bool noise_coord_ok(float c) { return fabsf(c) < 0x1p30f; }

__device__ __forceinline__ float perlin_fade(float t) { return t * t * t * (t * (t * 6 - 15) + 10); }          // Perlin.h:43
__device__ __forceinline__ float perlin_lerp(float t, float a, float b) { return a + t * (b - a); }             // :44
__device__ __forceinline__ float perlin_grad(int hash, float x, float y, float z) {                             // :45-51
    const int h = hash & 15;
    const float u = h < 8 ? x : y, v = h < 4 ? y : (h == 12 || h == 14 ? x : z);
    return ((h & 1) == 0 ? u : -u) + ((h & 2) == 0 ? v : -v);
}

// PerlinNoise::noise (Perlin.h:16-40)
__device__ __forceinline__ float perlin_noise(const NoiseTables &t, float x, float y, float z, bool &ok) {
    if (!(noise_coord_ok(x) && noise_coord_ok(y) && noise_coord_ok(z))) { ok = false; return 0.0f; }
    const float fx = floorf(x), fy = floorf(y), fz = floorf(z);
    const int X = (int)fx & 255, Y = (int)fy & 255, Z = (int)fz & 255;                                        // :18-20
    x -= fx; y -= fy; z -= fz;                                                                                  // :22-24
    const float u = perlin_fade(x), v = perlin_fade(y), w = perlin_fade(z);
    const uint8_t *p = t.perm;
    const int A = p[X] + Y, AA = p[A & 255] + Z, AB = p[(A + 1) & 255] + Z;                                     // :29-30
    const int B = p[(X + 1) & 255] + Y, BA = p[B & 255] + Z, BB = p[(B + 1) & 255] + Z;
    return perlin_lerp(w, perlin_lerp(v, perlin_lerp(u, perlin_grad(p[AA & 255], x, y, z),                      // :32-39
                                                        perlin_grad(p[BA & 255], x - 1, y, z)),
                                         perlin_lerp(u, perlin_grad(p[AB & 255], x, y - 1, z),
                                                        perlin_grad(p[BB & 255], x - 1, y - 1, z))),
                          perlin_lerp(v, perlin_lerp(u, perlin_grad(p[(AA + 1) & 255], x, y, z - 1),
                                                        perlin_grad(p[(BA + 1) & 255], x - 1, y, z - 1)),
                                         perlin_lerp(u, perlin_grad(p[(AB + 1) & 255], x, y - 1, z - 1),
                                                        perlin_grad(p[(BB + 1) & 255], x - 1, y - 1, z - 1))));
}

// generateNoise (Texture.h:20-37) with z = 0, as every 2-D texture calls it.  `iterations` may differ from lane to lane
// (StoneTexture::bumpHeight2D: id[0] % 3 + 5): the loop runs to the wave's largest count with the other lanes masked off.
__device__ __forceinline__ float turbulence(const NoiseTables &t, float x, float y, float initial_frequency, float frequency_increase,
                                            float amplitude_falloff, int iterations, bool &ok) {
    float amplitude = 1, frequency = initial_frequency, value = 0, max_val = 0;
#pragma unroll 1
    for (int i = 0; i < iterations; i++) {
        value += amplitude * perlin_noise(t, x * frequency, y * frequency, 0.0f * frequency, ok);
        max_val += amplitude;
        frequency *= frequency_increase;
        amplitude *= amplitude_falloff;
    }
    return value / max_val;
}

struct Worley3 {
    float F0, F1, F2;          // squared distances while the search runs, F_1 <= F_2 <= F_3 afterwards
    uint32_t I0, I1, I2;
};

// addSamples (Worley.cpp:367-436) for the cell (xi, yi)
__device__ __forceinline__ void worley_cell(const NoiseTables &t, int xi, int yi, float atx, float aty, Worley3 &w) {
    uint32_t seed = 702395077u * (uint32_t)xi + 915488749u * (uint32_t)yi;                                      // :383
    const int count = t.poisson[seed >> 24];                                                                    // :386
    seed = 1402024253u * seed + 586950981u;                                                                     // :389
#pragma unroll 1
    for (int j = 0; j < count; j++) {
        const uint32_t this_id = seed;
        seed = 1402024253u * seed + 586950981u;
        const float fx = (float)(((double)seed + 0.5) * (1.0 / 4294967296.0));                                  // :397
        seed = 1402024253u * seed + 586950981u;
        const float fy = (float)(((double)seed + 0.5) * (1.0 / 4294967296.0));
        seed = 1402024253u * seed + 586950981u;
        const float dx = (float)xi + fx - atx, dy = (float)yi + fy - aty;                                       // :403-404
        const float d2 = dx * dx + dy * dy;
        if (d2 < w.F2) {                                             // :407-434: the insertion, an earlier point wins a tie
            if (d2 < w.F0) { w.F2 = w.F1; w.I2 = w.I1; w.F1 = w.F0; w.I1 = w.I0; w.F0 = d2; w.I0 = this_id; }
            else if (d2 < w.F1) { w.F2 = w.F1; w.I2 = w.I1; w.F1 = d2; w.I1 = this_id; }
            else { w.F2 = d2; w.I2 = this_id; }
        }
    }
}

// the nine cells in the reference's order (Worley.cpp:130-163) as offsets + 1, two bits per cell
constexpr uint32_t worley_pack(int a0, int a1, int a2, int a3, int a4, int a5, int a6, int a7, int a8) {
    return (uint32_t)(a0 + 1) | (uint32_t)(a1 + 1) << 2 | (uint32_t)(a2 + 1) << 4 | (uint32_t)(a3 + 1) << 6 | (uint32_t)(a4 + 1) << 8 |
           (uint32_t)(a5 + 1) << 10 | (uint32_t)(a6 + 1) << 12 | (uint32_t)(a7 + 1) << 14 | (uint32_t)(a8 + 1) << 16;
}
constexpr uint32_t kWorleyDx = worley_pack(0, -1, 0, 1, 0, -1, 1, -1, 1);
constexpr uint32_t kWorleyDy = worley_pack(0, 0, -1, 0, 1, -1, 1, 1, -1);

// WorleyNoise::noise2D(at, 3, F, delta, ID) (Worley.cpp:95-173) without delta, which no texture reads.  ID of a slot that no
// feature point reached (never seen: nine cells hold 22 points on average) is 0, where the reference leaves it unset.
__device__ __forceinline__ Worley3 worley2(const NoiseTables &t, float atx, float aty, bool &ok) {
    Worley3 w;
    w.F0 = w.F1 = w.F2 = (float)999999.9;                                                                       // :107
    w.I0 = w.I1 = w.I2 = 0u;
    const float nx = (float)(0.398150 * (double)atx), ny = (float)(0.398150 * (double)aty);                     // :110-111
    if (!(noise_coord_ok(nx) && noise_coord_ok(ny))) {
        ok = false;
        w.F0 = w.F1 = w.F2 = 0.0f;
        return w;
    }
    const int ix = (int)floorf(nx), iy = (int)floorf(ny);                                                       // :114-115
    float x2 = nx - (float)ix, y2 = ny - (float)iy;                                                             // :135-136
    const float mx2 = (float)((1.0 - (double)x2) * (1.0 - (double)x2)), my2 = (float)((1.0 - (double)y2) * (1.0 - (double)y2));
    x2 *= x2; y2 *= y2;
    // the central cell, the four face cells, the four edge cells: a neighbour is searched when the squared distance to its
    // nearest border (edge cells: corner) is below the current F[2] (:146-163).  A face cell's bound is x2 + 0: x2 itself.
#pragma unroll 1
    for (int c = 0; c < 9; c++) {
        const int ox = (int)((kWorleyDx >> (2 * c)) & 3u) - 1, oy = (int)((kWorleyDy >> (2 * c)) & 3u) - 1;
        const float bx = ox < 0 ? x2 : (ox > 0 ? mx2 : 0.0f), by = oy < 0 ? y2 : (oy > 0 ? my2 : 0.0f);
        if (c == 0 || bx + by < w.F2) worley_cell(t, ix + ox, iy + oy, nx, ny, w);
    }
    w.F0 = (float)((double)sqrtf(w.F0) * (1.0 / 0.398150));                                                     // :169
    w.F1 = (float)((double)sqrtf(w.F1) * (1.0 / 0.398150));
    w.F2 = (float)((double)sqrtf(w.F2) * (1.0 / 0.398150));
    return w;
}

}  // namespace
}  // namespace mr
