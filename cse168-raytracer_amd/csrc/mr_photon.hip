// mr_photon.hip -- Photon_map::irradiance_estimate / locate_photons (PhotonMap.cpp:81-243) on gfx950:
// one wave64 per query, the k-nearest candidate set in LDS.
//
// The reference walks the implicit kd-tree one node at a time with a 500-entry max-heap per query.  What it returns is a SET --
// the k nearest facing photons inside the radius (minus one, see below) -- and a set can be found in any order.  Here a wave
// works on BLOCKS of the heap-ordered tree: the 63 nodes of six consecutive levels below a block root b are b*2^l + o
// (contiguous per level, so the loads coalesce), one node per lane, and every block carries two bounding boxes made at
// balance time (of its own 63 photons, and of everything below its root).  A search is two interleaved phases: EXPAND hands
// each lane one of a pending block's 64 child blocks and measures the query's distance to the child's boxes -- children
// whose own box reaches into the radius are listed, children whose subtree box does are expanded in turn --, EXAMINE tests
// the 63 photons of a listed block (distance, facing) and appends accepted ones to the LDS candidate buffer by ballot +
// prefix sum, four listed blocks per step with all their loads in flight together.  When the buffer is nearly full the wave
// selects the k smallest distances (4-pass radix select on the float bits, LDS histogram) and the k-th becomes the new
// radius.  (Rounds 1-2 walked the kd-tree's planes block by block in the reference's order, with the lanes of a block
// pulling their ancestors' decisions through shuffles: a serial chain of ~2 300 cycles per block and 93 blocks per query
// where the boxes need 61 independent ones; 41.5 -> 24 ms per 2.07 M queries, results identical.)
//
// Kept from the reference: nodes with index >= stored/2-1 do not descend (the photons below them are never found); the normalising radius stays
// max_dist^2 unless more than k candidates were seen; strict comparisons; and the FIRST-OVERFLOW REPLACEMENT
// (PhotonMap.cpp:195-240): when candidate k+1 arrives the reference heapifies the k it holds and replaces the heap
// root -- the farthest of the first k, m* -- by the newcomer even when the newcomer is farther still, and only from
// then on does the radius follow the heap root.  m* therefore never takes part in the result: what the reference
// returns is the k nearest of (all candidates minus m*).  Which photon m* is depends on the reference's visiting
// order (near side first, a node after its subtrees), so a first pass walks exactly that order, one query per lane,
// until k+1 candidates have been seen (first_overflow below); the wave-cooperative search then skips m*.
// found and the radius are the reference's on every query.  Not kept: the order in which the powers are summed
// (float rounding, ~1e-6 relative), and which of two photons at exactly the same squared distance is dropped when they
// tie for m* or at the k-th place (the reference's heap layout decides; distances, found and radius are unaffected).
#include <hip/hip_runtime.h>

#include "mr_irradiance_body.h"

namespace mr {
namespace {

// The kernel's body and the device helpers it uses are mr_irradiance_body.h (irradiance_body<STATS>), which the queued form of
// mr_gather_queued.hip instantiates too.  Five waves per SIMD without STATS, as that header says.
template <bool STATS>
__global__ __launch_bounds__(kIrrBlock) __attribute__((amdgpu_waves_per_eu(STATS ? 4 : 5, 8))) void irradiance_kernel(PhotonMapDev pm, const float *qpos, const float *qnrm,
                                                            unsigned long long nq, float max_dist, int k, float *irrad,
                                                            int *found_out, float *r2_out, unsigned long long *stats, int stack_cap,
                                                            unsigned *work_counter) {
    extern __shared__ int s_lds[];
    irradiance_body<STATS>(pm, qpos, qnrm, nq, max_dist, k, irrad, found_out, r2_out, stats, stack_cap, work_counter, s_lds);
}

}  // namespace

mr_status launch_irradiance(const PhotonMapDev &pm, unsigned *work_counter, const float *d_pos, const float *d_normal, unsigned long long nq,
                            float max_dist, uint32_t k, float *d_irrad, int32_t *d_found, float *d_r2, unsigned long long *d_stats,
                            hipStream_t stream) {
    int stack_cap = 0;
    size_t lds = 0;
    unsigned blocks = 0;
    const mr_status st = irradiance_launch_shape(pm, work_counter, nq, stack_cap, lds, blocks);
    if (st != MR_OK) return st;
    if (d_stats)
        hipLaunchKernelGGL(irradiance_kernel<true>, dim3(blocks), dim3(kIrrBlock), lds, stream, pm, d_pos, d_normal, nq, max_dist,
                           (int)k, d_irrad, d_found, d_r2, d_stats, stack_cap, work_counter);
    else
        hipLaunchKernelGGL(irradiance_kernel<false>, dim3(blocks), dim3(kIrrBlock), lds, stream, pm, d_pos, d_normal, nq, max_dist,
                           (int)k, d_irrad, d_found, d_r2, d_stats, stack_cap, work_counter);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
