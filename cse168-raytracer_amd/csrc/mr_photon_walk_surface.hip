// mr_photon_walk_surface.hip -- the photon walk on textured scenes (mr_trace_photons_surface): Scene::tracePhoton's roulette
// reads the looked-up diffuse colour (Scene.cpp:545-553, :608) and bounces about HitInfo::N as Scene::trace leaves it, bumped
// on a STONE material (Scene.cpp:234-263).
//
//   photon_walk_surface_kernel   the walk of mr_photon_walk_body.h with the surface pass's colour and normal at every hit:
//                                photon_walk_body<VAR, WalkSurfaceSource>, whose source calls hit_color_normal
//                                (mr_hit_surface_body.h): the surface pass's per-hit steps over the same shared arms, so a
//                                hit's colour and normal are the bits mr_hit_surface writes for the same ray and hit.
//
// Why the lookup may sit in a kernel that traverses, against the rule of mr_procedural.hip's header: that rule was written for
// shading kernels, which hold a shadow traversal's state across the lookup.  Here the lookup lies between two traversals; only
// the ray, the power, the hit and two state words are live across it.
//
// The launch is the plain walk's (mr_photon_walk.hip): a resident grid of 256-lane workgroups, dynamic LDS stacks, re-arm by
// ballot with one atomic per wave -- plus 512 bytes of static LDS for the two noise tables, staged once per workgroup before
// the first segment.  The noise arms sit behind hit_color_normal's wave-level branch.  The colour, the point and the normal of
// a hit are computed together, before the roulette, for every hit: the colour is needed for every hit (an absorbed photon still
// needs prob[0]), and uv_of needs the point.  The round's bookkeeping kernels stay in mr_photon_walk.hip
// (launch_photon_round_finish).  Lookups the reference leaves undefined take the value the surface pass defines and are not
// counted: a count over walked emissions would depend on the round size.
#include <hip/hip_runtime.h>

#include "mr_hit_surface_body.h"
#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_noise.h"
#include "mr_photon_walk_body.h"

namespace mr {
namespace {

struct WalkSurfaceSource {
    TexParams t;                 // recs / mat_tex nullptr: the scene has no texture table
    NoiseTables nt;
    float col[3], P[3], N[3];
    __device__ __forceinline__ void color(const WalkArgs &a, const float o[3], const float d[3], const mr_hit &h, const float *mt) {
        surface_od<true>(a.m.s, o[0], o[1], o[2], d[0], d[1], d[2], h.t, h.prim, h.beta, h.gamma, P, N);
        bool ok = true;
        hit_color_normal(a.m, t, nt, h.prim, P, N, col, ok);
    }
    __device__ __forceinline__ void point(const WalkArgs &a, const float o[3], const float d[3], const mr_hit &h, float Pq[3], float Nq[3]) const {
        for (int c = 0; c < 3; c++) { Pq[c] = P[c]; Nq[c] = N[c]; }
    }
};

// amdgpu_waves_per_eu(5, 8): the plain walk's 5 waves per SIMD.  Left to itself the compiler takes 101 / 106 VGPRs (4 waves);
// asked for 5 it fits 96 without spilling a VGPR and without scratch.
template <int VAR>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(5, 8))) void photon_walk_surface_kernel(WalkArgs a, TexParams t) {
    __shared__ uint32_t s_tab[128];
    WalkSurfaceSource src;
    src.t = t;
    src.nt = stage_noise_tables(s_tab);
    photon_walk_body<VAR>(a, src);
}

}  // namespace

mr_status launch_photon_round_surface(const DeviceScene &ds, const TexParams &tex, const PhotonWalkLight &lt, uint32_t seed, uint32_t caustic,
                                      uint32_t max_depth, uint32_t first, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b,
                                      hipStream_t stream) {
    if (count == 0 || count > b.capacity) return fail(MR_ERR_INVALID, "photon round of %u emissions (buffers hold %u)", count, b.capacity);
    const WalkArgs a = walk_args_of(ds, lt, seed, caustic, max_depth, first, count, b);
    MR_HIP_CHECK(hipMemsetAsync(b.next, 0, sizeof(unsigned), stream));
    mr_status st = (ds.n_planes || ds.n_spheres) ? launch_walk(&photon_walk_surface_kernel<kTraceVoteObj>, a, stream, tex)
                                                 : launch_walk(&photon_walk_surface_kernel<kTraceVote>, a, stream, tex);
    if (st != MR_OK) return st;
    return launch_photon_round_finish(max_depth, count, need, b, stream);
}

}  // namespace mr
