// mr_eye.h -- Camera::eyeRay (Camera.cpp:104-161) for the kernels that generate primary rays: the batched generator
// (eye_rays_kernel, mr_kernels.hip) and the fused frame kernel (mr_frame.hip) share one definition, so their rays
// are the same bits.  The camera frame is computed on the host exactly as the reference does (Camera.h:79-110,
// Camera.cpp:113-124); the per-sample arithmetic keeps the reference's operation order.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "mr_internal.h"
#include "mr_surface.h"
#include "mr_tile.h"

namespace mr {

struct EyeFrame {
    float eye[3], u[3], v[3], w[3];
    float left, right, bottom, top;
    uint32_t W, H, y0, spp, jitter, hbase;
    uint32_t tiled, rows;        // tiled: ray order of mr_tile.h inside the window of `rows` rows
    // rows of the window in the image: contiguous from y0 (band_world == 1), or the interleaved bands of one rank of a
    // multi-GPU frame -- window row j is image row ((j / band_rows) * band_world + band_rank) * band_rows + j % band_rows
    uint32_t band_rows, band_rank, band_world;
    TileShape tile;
    unsigned long long n;        // samples in the window = rows * W * spp
};

// y0/y1: contiguous window.  For banded windows call set_bands() afterwards.  view_dir (optional): m_viewDir, normalised
// once -- f.w is its negative normalised again, which is not the same bits.
inline EyeFrame make_eye_frame(const mr_camera &cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t spp,
                               uint32_t jitter, uint32_t seed, bool tiled, float *view_dir = nullptr) {
    auto unit3 = [](float *a) {
        const float len = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
        const float inv = 1.0f / len;
        a[0] *= inv; a[1] *= inv; a[2] *= inv;
    };
    EyeFrame f;
    float up[3] = {cam.up[0], cam.up[1], cam.up[2]};
    unit3(up);
    float view[3] = {cam.lookat[0] - cam.eye[0], cam.lookat[1] - cam.eye[1], cam.lookat[2] - cam.eye[2]};
    unit3(view);
    if (view_dir) { view_dir[0] = view[0]; view_dir[1] = view[1]; view_dir[2] = view[2]; }
    f.w[0] = -view[0]; f.w[1] = -view[1]; f.w[2] = -view[2];
    unit3(f.w);
    cross3(up, f.w, f.u);
    unit3(f.u);
    cross3(f.w, f.u, f.v);
    const float PI = 3.1415926535897932384626433832795028841972f;
    const float DegToRad = PI / 180.0f, HalfDegToRad = DegToRad / 2.0f;
    const float aspect = (float)W / (float)H;
    f.top = tanf(cam.fov_deg * HalfDegToRad);
    f.right = aspect * f.top; f.bottom = -f.top; f.left = -f.right;
    f.eye[0] = cam.eye[0]; f.eye[1] = cam.eye[1]; f.eye[2] = cam.eye[2];
    f.W = W; f.H = H; f.y0 = y0; f.spp = spp; f.jitter = jitter;
    f.tile = tile_shape(spp);
    f.rows = y1 - y0;
    f.band_rows = f.rows ? f.rows : 1; f.band_rank = 0; f.band_world = 1;
    f.tiled = tiled && (f.tile.th > 1 || f.tile.tw > 1) ? 1u : 0u;
    f.hbase = pcg32(seed);
    f.n = (unsigned long long)(y1 - y0) * W * spp;
    return f;
}

#if defined(__HIPCC__)
// sample k of the window -> pixel (x, window row, image row y) and sample number
__device__ __forceinline__ void eye_sample_of(const EyeFrame &f, unsigned long long k, uint32_t &x, uint32_t &row, uint32_t &y,
                                              uint32_t &sm) {
    const unsigned long long pix_local = k / f.spp;
    sm = (uint32_t)(k - pix_local * f.spp);
    row = (uint32_t)(pix_local / f.W);
    x = (uint32_t)(pix_local % f.W);
    if (f.tiled) tile_decode((uint32_t)pix_local, f.W, f.rows, f.tile, x, row);
    y = f.band_world == 1 ? f.y0 + row
                          : ((row / f.band_rows) * f.band_world + f.band_rank) * f.band_rows + row % f.band_rows;
}

// Camera::eyeRay (Camera.cpp:127-160) in the pieces its plain and its thin-lens form share:
// the key of sample `sm` of pixel (x, y), from which the sample's random numbers are drawn
__device__ __forceinline__ uint32_t eye_sample_key(const EyeFrame &f, uint32_t x, uint32_t y, uint32_t sm) {
    return pcg32(pcg32(f.hbase ^ (y * f.W + x)) + sm);
}
// ... its offset inside the pixel
__device__ __forceinline__ void eye_jitter_of(uint32_t key, float &dx, float &dy) {
    dx = unit01(pcg32(key));
    dy = unit01(pcg32(key ^ 0x68bc21ebu));
}
// ... the film coordinates of pixel (x, y) at offset (dx, dy) (Camera.cpp:157-158)
__device__ __forceinline__ void eye_film_of(const EyeFrame &f, uint32_t x, uint32_t y, float dx, float dy, float &up, float &vp) {
    up = f.left + (f.right - f.left) * (((float)x + dx) / (float)f.W);
    vp = f.bottom + (f.top - f.bottom) * (((float)y + dy) / (float)f.H);
}
// ... and the ray's second half: (up * uDir + vp * vDir - w) normalised (:160), tMax = MIRO_TMAX
__device__ __forceinline__ float4 eye_direction_of(const EyeFrame &f, float up, float vp, const float w[3]) {
    const float ddx = (up * f.u[0] + vp * f.v[0]) - w[0];
    const float ddy = (up * f.u[1] + vp * f.v[1]) - w[1];
    const float ddz = (up * f.u[2] + vp * f.v[2]) - w[2];
    const float len = sqrtf((ddx * ddx + ddy * ddy) + ddz * ddz);
    const float inv = 1.0f / len;
    return make_float4(ddx * inv, ddy * inv, ddz * inv, 1e12f);
}

// Camera::eyeRay for sample `sm` of pixel (x, y): a = (eye, tMin = 0), b = (direction, tMax = MIRO_TMAX)
__device__ __forceinline__ void eye_ray_of(const EyeFrame &f, uint32_t x, uint32_t y, uint32_t sm, float4 &a, float4 &b) {
    float dx = 0.5f, dy = 0.5f, up, vp;
    if (f.jitter) eye_jitter_of(eye_sample_key(f, x, y, sm), dx, dy);
    eye_film_of(f, x, y, dx, dy, up, vp);
    a = make_float4(f.eye[0], f.eye[1], f.eye[2], 0.0f);
    b = eye_direction_of(f, up, vp, f.w);
}
#endif

// ---- the thin lens: Camera::eyeRay under -DDOF (Camera.cpp:135-160, Miro.h:18-19, sampleDisc Utility.h:82-95).  The batched
// generator (eye_rays_lens_kernel, mr_distribution.hip) and the fused lens frame (mr_frame_lens.hip) share the definitions
// below, so their rays are the same bits.
constexpr uint32_t kLensRounds = 32;                  // rounds of sampleDisc's rejection loop before the sample is (0, 0)
constexpr uint32_t kLensDomain = 0x4c454e53u;         // "LENS": the lens draws' keys, see mr_gen_eye_rays_lens (miro_hip.h)

struct LensParams {
    float focus[3];              // m_eye + m_viewDir * DOF_FOCUS_PLANE (Camera.cpp:142), computed on the host
    float aperture;
};
// what launch_eye_rays_lens and the lens frames put into the block; view: make_eye_frame's view_dir
inline LensParams lens_params_of(const mr_camera &cam, const float view[3], const mr_lens_desc &lens) {
    LensParams ln;
    for (int c = 0; c < 3; c++) ln.focus[c] = cam.eye[c] + view[c] * lens.focus_plane;    // Camera.cpp:142's first two terms
    ln.aperture = lens.aperture;
    return ln;
}

#if defined(__HIPCC__)
// the random numbers of sample `sm` of pixel (x, y): its offset inside the pixel (with f.jitter) and sampleDisc's point on the
// lens (Utility.h:86-89).  false: the rejection loop exhausted kLensRounds, and the point is the lens centre
__device__ __forceinline__ bool eye_lens_draw(const EyeFrame &f, float aperture, uint32_t x, uint32_t y, uint32_t sm, float &dx, float &dy,
                                              float &lx, float &ly) {
    const uint32_t h = eye_sample_key(f, x, y, sm);
    if (f.jitter) eye_jitter_of(h, dx, dy);
    bool found = false;
    for (uint32_t r = 0; r < kLensRounds && !found; r++) {
        const float fx = unit01(pcg32(h ^ (kLensDomain + 2u * r))), fy = unit01(pcg32(h ^ (kLensDomain + 2u * r + 1u)));
        const float xr = (2 * fx - 1) * aperture, yr = (2 * fy - 1) * aperture;
        if (!(xr * xr + yr * yr > aperture * aperture)) { lx = xr; ly = yr; found = true; }
    }
    return found;
}
// the ray of pixel (x, y) at offset (dx, dy) through the lens point (lx, ly)
__device__ __forceinline__ void eye_lens_ray(const EyeFrame &f, const LensParams &ln, uint32_t x, uint32_t y, float dx, float dy, float lx,
                                             float ly, float4 &a, float4 &b) {
    float up, vp, e[3], lw[3];
    eye_film_of(f, x, y, dx, dy, up, vp);
    for (int c = 0; c < 3; c++) {
        e[c] = f.eye[c] + (lx * f.u[c] + ly * f.v[c]);                                 // Camera.cpp:140
        lw[c] = -(ln.focus[c] - e[c]);                                                 // :142, :145
    }
    normalize3(lw);
    a = make_float4(e[0], e[1], e[2], 0.0f);
    b = eye_direction_of(f, up, vp, lw);                                               // :160, uDir / vDir of the unmoved eye
}
// Camera::eyeRay under -DDOF for sample `sm` of pixel (x, y): a = (the point on the lens, tMin = 0), b = (direction, tMax)
__device__ __forceinline__ void eye_ray_lens_of(const EyeFrame &f, const LensParams &ln, uint32_t x, uint32_t y, uint32_t sm, float4 &a,
                                                float4 &b) {
    float dx = 0.5f, dy = 0.5f, lx = 0.0f, ly = 0.0f;
    eye_lens_draw(f, ln.aperture, x, y, sm, dx, dy, lx, ly);
    eye_lens_ray(f, ln, x, y, dx, dy, lx, ly, a, b);
}
#endif

}  // namespace mr
