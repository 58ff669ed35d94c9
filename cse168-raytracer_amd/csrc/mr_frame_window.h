// mr_frame_window.h -- the window of a frame descriptor as the fused light-list frames read it: mr_frame.hip's reading
// (MR_FRAME_ENTRY), in its wording, once for mr_render_lights (mr_frame_lights.hip) and mr_render_lights_surface
// (mr_frame_lights_surface.hip).  Host code only: it reads nothing but the descriptor and makes no device call.
#pragma once

#include "mr_eye.h"
#include "mr_internal.h"

namespace mr {

// `fd` has band_world >= 1; `who` names the entry point in the messages
inline mr_status frame_window_of(const char *who, const mr_frame_desc &fd, EyeFrame &eye) {
    const uint32_t spp = fd.spp;
    if (spp == 0 || spp > 64 || (spp & (spp - 1)))
        return fail(MR_ERR_INVALID, "%s: spp must be a power of two <= 64 (got %u); use the batched pipeline", who, spp);
    if (fd.band_world == 0 || fd.band_rank >= fd.band_world || fd.band_rows == 0)
        return fail(MR_ERR_INVALID, "%s: bad band description (%u rows, rank %u of %u)", who, fd.band_rows, fd.band_rank, fd.band_world);
    uint32_t rows = 0;
    if (fd.band_world == 1) {
        if (fd.y1 > fd.H || fd.y0 > fd.y1) return fail(MR_ERR_INVALID, "%s: rows [%u,%u) outside the image", who, fd.y0, fd.y1);
        rows = fd.y1 - fd.y0;
    } else {
        const uint32_t nb = (fd.H + fd.band_rows - 1) / fd.band_rows;
        for (uint32_t b = fd.band_rank; b < nb; b += fd.band_world) {
            const uint32_t y0 = b * fd.band_rows, y1 = y0 + fd.band_rows < fd.H ? y0 + fd.band_rows : fd.H;
            rows += y1 - y0;
        }
    }
    eye = make_eye_frame(fd.camera, fd.W, fd.H, fd.band_world == 1 ? fd.y0 : 0, fd.band_world == 1 ? fd.y1 : rows, spp, fd.jitter, fd.seed,
                         fd.tiled != 0);
    eye.rows = rows;
    eye.n = (unsigned long long)rows * fd.W * spp;
    if (fd.band_world > 1) {
        // (a ragged last band only ever is the LAST window row group of its owner: eye_sample_of's row formula holds for it)
        eye.y0 = 0; eye.band_rows = fd.band_rows; eye.band_rank = fd.band_rank; eye.band_world = fd.band_world;
    }
    if (eye.n >= (1ull << 32) * spp) return fail(MR_ERR_INVALID, "%s: window too large", who);
    return MR_OK;
}

}  // namespace mr
