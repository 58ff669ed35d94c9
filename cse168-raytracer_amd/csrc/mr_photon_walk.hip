// mr_photon_walk.hip -- Scene::tracePhotons / traceCausticPhotons for one DirectionalAreaLight (Scene.cpp:351-472) with
// Scene::tracePhoton (Scene.cpp:529-655) per emitted photon, on the device:
//
//   photon_walk_kernel      the walk of mr_photon_walk_body.h (emission -> Scene::trace -> roulette -> store / absorb / the
//                           next segment, one lane per photon) with the material's own kd and the geometric normal:
//                           photon_walk_body<VAR, WalkMaterialSource>.  The textured form, whose colour and normal are the
//                           surface pass's, is the kernel of mr_photon_walk_surface.hip on the same body.
//   photon_scan_kernel      one workgroup: prefix sum over the round's per-emission store counts, the round's E (the first
//                           emission at which the running total reaches the target), and the round's header
//   photon_compact_kernel   the records of emissions 0 ... E-1 of the round, in emission order and by depth within an emission
//
// Each emission owns max_depth record slots (a photon stores at most once per hit from its second hit on, and walks
// max_depth + 1 segments) and one packed word: stores | segments << 8.
//
// Random numbers: the counter-based generator of the eye-ray jitter (pcg32 / unit01, mr_internal.h).  Keys are documented
// next to mr_trace_photons in miro_hip.h.
#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_photon_walk_body.h"
#include "mr_recursion.h"
#include "mr_traverse.h"

namespace mr {
namespace {

template <int VAR>
__global__ __launch_bounds__(kTraceBlock) void photon_walk_kernel(WalkArgs a) {
    photon_walk_body<VAR>(a, WalkMaterialSource());
}

// ---- per-round bookkeeping -----------------------------------------------------------------------------------------------
constexpr int kScanBlock = 1024;

__global__ __launch_bounds__(kScanBlock) void photon_scan_kernel(const uint32_t *words, uint32_t count, unsigned long long need,
                                                                  uint32_t *offsets, PhotonRoundHeader *hdr) {
    __shared__ unsigned long long s_sum[kScanBlock];
    __shared__ unsigned s_cross;
    const unsigned t = threadIdx.x;
    const unsigned per = (count + kScanBlock - 1) / kScanBlock;
    const unsigned lo = t * per < count ? t * per : count, hi = lo + per < count ? lo + per : count;
    unsigned long long mine = 0;
    for (unsigned i = lo; i < hi; i++) mine += words[i] & 255u;
    s_sum[t] = mine;
    if (t == 0) s_cross = count;
    __syncthreads();
    for (unsigned off = 1; off < kScanBlock; off <<= 1) {               // inclusive scan of the threads' totals
        unsigned long long v = 0;
        if (t >= off) v = s_sum[t - off];
        __syncthreads();
        s_sum[t] += v;
        __syncthreads();
    }
    unsigned long long run = s_sum[t] - mine;
    for (unsigned i = lo; i < hi; i++) {
        offsets[i] = (uint32_t)run;
        run += words[i] & 255u;
        if (need > 0 && run >= need) atomicMin(&s_cross, i);            // the first emission whose running total reaches the target
    }
    __syncthreads();
    const unsigned E = need == 0 ? 0u : (s_cross < count ? s_cross + 1u : count);
    // totals over emissions 0 ... E-1
    unsigned long long st = 0, sg = 0;
    for (unsigned i = lo; i < hi && i < E; i++) { st += words[i] & 255u; sg += words[i] >> 8; }
    __syncthreads();
    s_sum[t] = st;
    __syncthreads();
    for (unsigned off = kScanBlock / 2; off > 0; off >>= 1) { if (t < off) s_sum[t] += s_sum[t + off]; __syncthreads(); }
    const unsigned long long stored = s_sum[0];
    __syncthreads();
    s_sum[t] = sg;
    __syncthreads();
    for (unsigned off = kScanBlock / 2; off > 0; off >>= 1) { if (t < off) s_sum[t] += s_sum[t + off]; __syncthreads(); }
    if (t == 0) { hdr->emitted = E; hdr->reached = (need == 0 || s_cross < count) ? 1u : 0u; hdr->stored = stored; hdr->segments = s_sum[0]; }
}

__global__ __launch_bounds__(kBlock) void photon_compact_kernel(const float4 *slots, const uint32_t *words, const uint32_t *offsets,
                                                                uint32_t count, uint32_t max_depth, const PhotonRoundHeader *hdr,
                                                                float4 *out) {
    const uint32_t E = hdr->emitted;
    const unsigned long long n = (unsigned long long)(E < count ? E : count) * max_depth;
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        const uint32_t e = (uint32_t)(k / max_depth), j = (uint32_t)(k % max_depth);
        if (j >= (words[e] & 255u)) continue;
        const size_t dst = 3 * ((size_t)offsets[e] + j);
        out[dst] = slots[3 * k]; out[dst + 1] = slots[3 * k + 1]; out[dst + 2] = slots[3 * k + 2];
    }
}

}  // namespace

// the bookkeeping kernels behind a round's walk, whichever kernel walked it (mr_photon_walk_surface.hip launches its own)
mr_status launch_photon_round_finish(uint32_t max_depth, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b, hipStream_t stream) {
    hipLaunchKernelGGL(photon_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, b.words, count, need, b.offsets, b.header);
    MR_HIP_CHECK(hipGetLastError());
    unsigned long long blocks = ((unsigned long long)count * max_depth + kBlock - 1) / kBlock;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(photon_compact_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, b.slots, b.words, b.offsets, count, max_depth,
                       b.header, b.compact);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_photon_round(const DeviceScene &ds, const PhotonWalkLight &lt, uint32_t seed, uint32_t caustic, uint32_t max_depth,
                              uint32_t first, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b, hipStream_t stream) {
    if (count == 0 || count > b.capacity) return fail(MR_ERR_INVALID, "photon round of %u emissions (buffers hold %u)", count, b.capacity);
    const WalkArgs a = walk_args_of(ds, lt, seed, caustic, max_depth, first, count, b);
    MR_HIP_CHECK(hipMemsetAsync(b.next, 0, sizeof(unsigned), stream));
    // photons walk incoherently after their first bounce: the voting control flow of the default (exact) traversal
    mr_status st = (ds.n_planes || ds.n_spheres) ? launch_walk(&photon_walk_kernel<kTraceVoteObj>, a, stream)
                                                 : launch_walk(&photon_walk_kernel<kTraceVote>, a, stream);
    if (st != MR_OK) return st;
    return launch_photon_round_finish(max_depth, count, need, b, stream);
}

}  // namespace mr
