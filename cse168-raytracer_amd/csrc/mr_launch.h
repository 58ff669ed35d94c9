// mr_launch.h -- what the host side of every traversal kernel shares: the names of trace_ray's variant bits and of the
// variants in use, the scene half of TraceParams, and the launch plumbing around the per-lane LDS stack.  The kernels are
// in mr_kernels.hip, mr_frame.hip, mr_level.hip, mr_lights.hip and mr_photon_walk.hip; the traversal is mr_traverse.h.
#pragma once

#include <type_traits>

#include "mr_internal.h"

namespace mr {

// The bits of trace_ray's VAR template argument (mr_traverse.h).  A variant's value is part of the mangled names of its
// kernels, which tests/golden/kernel_budget*.json record: the values below do not change.
constexpr int kVarMinMax     = 1;      // min/max slabs on the products (corner - o) * (1/d) for waves that cannot produce a NaN (same decisions as the select chains)
constexpr int kVarWhileWhile = 2;      // "while-while" control flow: lanes run inner nodes until each holds a leaf, then the wave does the leaves
constexpr int kVarLeanFma    = 4;      // lean fma slabs (MR_MATH_FAST)
constexpr int kVarScalar     = 8;      // wave-uniform nodes and leaves through the scalar cache
constexpr int kVarStrict     = 16;     // every slab distance is the reference's true quotient (the default trace; MR_COUNT_STATS implies it)
constexpr int kVarObjects    = 32;     // the scene holds spheres and / or planes
constexpr int kVarVote       = 64;     // the voting control flow instead of while-while
constexpr int kVarOctant     = 256;    // octant-specialised slab tests for waves whose rays share an octant
constexpr int kVarGuarded    = 512;    // guarded products (node_slabs_guarded) instead of the correction steps
constexpr int kVarMixedVote  = 1024;   // waves whose rays point into several octants take the voting control flow

// the variants in use
constexpr int kTraceExact          = kVarMixedVote | kVarGuarded | kVarOctant | kVarStrict | kVarScalar | kVarWhileWhile;   // the default
constexpr int kTraceEyeRel         = kTraceExact & ~kVarMixedVote;                       // the fused frame on its eye-relative tables
constexpr int kTraceExactObj       = kVarGuarded | kVarOctant | kVarObjects | kVarStrict | kVarScalar | kVarWhileWhile;
constexpr int kTraceProduct        = kVarOctant | kVarScalar | kVarWhileWhile | kVarMinMax;                 // MR_MATH_PRODUCT
constexpr int kTraceProductObj     = kVarObjects | kVarScalar | kVarWhileWhile | kVarMinMax;
constexpr int kTraceVote           = kVarVote | kVarStrict | kVarScalar;                 // MR_TRACE_INCOHERENT, on the correction steps alone
constexpr int kTraceVoteProduct    = kVarVote | kVarScalar | kVarMinMax;
constexpr int kTraceVoteObj        = kVarVote | kVarObjects | kVarStrict | kVarScalar;
constexpr int kTraceVoteProductObj = kVarVote | kVarObjects | kVarScalar | kVarMinMax;
constexpr int kTraceCorrection     = kVarOctant | kVarStrict | kVarScalar | kVarWhileWhile;                 // MIRO_DEV: the default without guarded products
constexpr int kTraceFast           = kVarScalar | kVarLeanFma | kVarWhileWhile | kVarMinMax;                // MR_MATH_FAST
constexpr int kTraceDevProduct     = kVarScalar | kVarWhileWhile | kVarMinMax;           // MIRO_DEV: MIRO_TRACE_VARIANT's default
constexpr int kTracePlainObj       = kVarObjects;                                        // MR_COUNT_STATS in scenes with objects
constexpr int kTracePlain          = 0;        // MR_COUNT_STATS: select-form slabs in the reference's control flow, lane by lane
static_assert(kTraceExact == 1818 && kTraceEyeRel == 794 && kTraceExactObj == 826 && kTraceProduct == 267 && kTraceProductObj == 43, "kernel names");
static_assert(kTraceVote == 88 && kTraceVoteProduct == 73 && kTraceVoteObj == 120 && kTraceVoteProductObj == 105, "kernel names");
static_assert(kTraceCorrection == 282 && kTraceFast == 15 && kTraceDevProduct == 11 && kTracePlainObj == 32, "kernel names");

// The variant of a batch that is traced for its hit records, by scene and flags: `f` is called with the variant as a
// std::integral_constant (mr_trace_level, mr_shade_lights).  Scenes with objects have no voting kernel here: `vote` is ignored.
template <typename F>
mr_status with_trace_variant(bool objects, bool product, bool vote, F &&f) {
    using std::integral_constant;
    if (objects) return product ? f(integral_constant<int, kTraceProductObj>()) : f(integral_constant<int, kTraceExactObj>());
    if (vote) return product ? f(integral_constant<int, kTraceVoteProduct>()) : f(integral_constant<int, kTraceVote>());
    return product ? f(integral_constant<int, kTraceProduct>()) : f(integral_constant<int, kTraceExact>());
}

// the scene half of TraceParams; what belongs to one launch (rays, hits, n, n_dev, stats, work_counter, order) is zero
inline TraceParams scene_trace_params(const DeviceScene &ds) {
    TraceParams p = {};
    p.nodes = ds.nodes; p.tris = ds.tris; p.tri_prim = ds.tri_prim; p.leaf_cnt_ext = ds.leaf_cnt_ext;
    for (int c = 0; c < 3; c++) { p.root_lo[c] = ds.root_lo[c]; p.root_hi[c] = ds.root_hi[c]; }
    p.root_ref = ds.root_ref;
    p.stack_depth = (int32_t)ds.stack_depth;
    p.planes = ds.planes; p.n_planes = ds.n_planes; p.n_spheres = ds.n_spheres;
    return p;
}

constexpr int kBlock = 256;          // 4 waves per workgroup
// memory/latency-bound kernels: cap the grid and grid-stride the rest (256 CUs x 8 blocks)
inline unsigned grid_for(unsigned long long n) {
    unsigned long long blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 256ull * 32ull) blocks = 256ull * 32ull;
    if (blocks == 0) blocks = 1;
    return (unsigned)blocks;
}

namespace {      // (mr_frame.hip is compiled with two values of MIRO_TRACE_BLOCK: what depends on it stays local to its unit)

#ifndef MIRO_TRACE_BLOCK
#define MIRO_TRACE_BLOCK 256
#endif
constexpr int kTraceBlock = MIRO_TRACE_BLOCK;   // threads per workgroup of the trace kernels (their LDS stack is [depth][kTraceBlock])
#ifndef MIRO_GRID_CAP
#define MIRO_GRID_CAP 32768
#endif
constexpr int kTraceGridCap = MIRO_GRID_CAP; // workgroups per trace launch (see launch_trace_t)

// workgroups of a one-shot trace launch over n rays
inline unsigned trace_grid(unsigned long long n, unsigned long long cap = kTraceGridCap) {
    const unsigned long long blocks = (n + kTraceBlock - 1) / kTraceBlock;
    return blocks > cap ? (unsigned)cap : blocks ? (unsigned)blocks : 1u;
}

// Dynamic LDS of a traversal kernel: one stack slot per level and lane.  `reject`: the largest stack a launcher accepts;
// above `opt_in` the kernel is first allowed that much dynamic LDS.  trace_kernel and trace_persistent_kernel declare no LDS of
// their own and may fill the CU's 160 KB; the frame, level and light-list kernels keep counters in static LDS beside the stack,
// which 150 KB leaves room for.  The photon walk has no static LDS and the same 150 KB, and why the opt-in starts at 64 KB for
// the first two and at 48 KB for the others is not recorded anywhere: both are kept as they were.
struct StackLds { size_t reject, opt_in; };
constexpr StackLds kStackLdsWhole = {160 * 1024, 64 * 1024}, kStackLdsShared = {150 * 1024, 48 * 1024};

// `lds` = the bytes to launch `kern` with for a stack of `stack_depth` levels (plus `pad` unused ones)
template <typename K>
mr_status stack_lds(K kern, int32_t stack_depth, StackLds limit, size_t &lds, size_t pad = 0) {
    lds = (size_t)stack_depth * kTraceBlock * sizeof(int) + pad;
    if (lds > limit.reject) return fail(MR_ERR_INVALID, "traversal stack of depth %d does not fit in LDS", stack_depth);
    if (lds > limit.opt_in)
        MR_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MR_OK;
}

// One launch of a traversal kernel that keeps static LDS beside its stack (the level, frame and light-list kernels): `grid`
// workgroups of kTraceBlock lanes with the stack of `stack_depth` levels as dynamic LDS, `args` the kernel's arguments
template <typename K, typename... Args>
mr_status launch_traversal(K kern, unsigned grid, int32_t stack_depth, hipStream_t stream, const Args &...args) {
    size_t lds = 0;
    const mr_status st = stack_lds(kern, stack_depth, kStackLdsShared, lds);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kTraceBlock), lds, stream, args...);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

// `grid` = the workgroups of `kern` the device holds at once, `want` at most and one at least
template <typename K>
mr_status resident_grid(K kern, size_t lds, unsigned long long want, unsigned &grid) {
    int dev = 0, cus = 256, per_cu = 1;
    MR_HIP_CHECK(hipGetDevice(&dev));
    MR_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    MR_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(kern), kTraceBlock, lds));
    if (per_cu < 1) per_cu = 1;
    const unsigned long long fit = (unsigned long long)cus * (unsigned)per_cu;
    grid = (unsigned)(want < fit ? want : fit);
    if (grid < 1) grid = 1;
    return MR_OK;
}

}  // namespace
}  // namespace mr
