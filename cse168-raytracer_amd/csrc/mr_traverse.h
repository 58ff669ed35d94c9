// mr_traverse.h -- device-side machinery of the intersection path, shared by the batched trace kernels
// (mr_kernels.hip) and the fused frame kernel (mr_frame.hip): slab tests, Triangle::intersect, Sphere::intersect,
// the per-lane LDS stack and the "while-while" traversal loop; at the end what the kernels around a traversal share: trace_hit,
// whole_workgroups, workgroup_add.  Device code only; include from .hip files.
//
//   BVH::intersect / intersectChildren   BVH.cpp:438-658 (scalar branch)
//   Triangle::intersect                  Triangle.cpp:136-169
//   Sphere::intersect                    Sphere.cpp:28-69
//
// Compiled with -ffp-contract=off: in the default ("exact") mode every fp32 operation below is one individually
// rounded IEEE op in the reference's order, so t / beta / gamma are bit-identical to the reference's scalar build.
#pragma once

#include <hip/hip_runtime.h>

#include "mr_internal.h"
#include "mr_launch.h"

namespace mr {
namespace {

// the fused frame kernel on frames of 2^18 chunks or more (1080p at 64 spp is 518 400): twice the workgroups, and XCD runs of 256
// chunks instead of 64 -- +1.1 % there, while frames of 4 to 16 samples per pixel lose 1.5-4 % to either (profiles/r03_grid_ab.log)
#ifndef MIRO_CAP_LARGE
#define MIRO_CAP_LARGE 65536
#define MIRO_RUN_LARGE 256
#endif
constexpr int kFrameGridCapLarge = MIRO_CAP_LARGE;
constexpr unsigned long long kFrameLargeChunks = 1ull << 18;

// Workgroup ids go round-robin to the 8 XCDs, each with its own L2 (not coherent with the others').  In the plain order
// every XCD traces every eighth 256-ray chunk of the whole image; here an XCD gets runs of kXcdRun consecutive chunks --
// one region of the image, whole cache lines of the output to itself: +4.9 % on the bench frame, +3 % at 16 and 4 spp
// (profiles/r02_xcd_runs.log; DESIGN.md section 4.14 for what the counters show).  Only for grids of kXcdMinGrid workgroups or more: a 1-spp frame is 8 100 workgroups,
// little more than four per resident slot, and there the uneven cost of the regions shows as idle XCDs (-5 %).  Round 3: launches that
// reach kFrameGridCapLarge workgroups (the fused frame kernel at 64 samples per pixel) take runs of kXcdRunLarge chunks.
#ifndef MIRO_XCD_MIN_GRID
#define MIRO_XCD_MIN_GRID 16384
#endif
constexpr unsigned kXcdRun = 64, kXcdRunLarge = MIRO_RUN_LARGE, kXcdMinGrid = MIRO_XCD_MIN_GRID;
__device__ __forceinline__ unsigned xcd_block_id_of(unsigned b, unsigned G, bool large, unsigned min_grid = kXcdMinGrid) {
    if (G < min_grid) return b;
    const unsigned run = large ? kXcdRunLarge : kXcdRun;
    const unsigned xcd = b & 7u, slot = b >> 3, grp = slot / run, k = slot - grp * run;
    return (grp + 1u) * (8u * run) <= G ? grp * (8u * run) + xcd * run + k : b;      // the ragged tail keeps the plain order
}
__device__ __forceinline__ unsigned xcd_block_id() {
    return xcd_block_id_of(blockIdx.x, gridDim.x, gridDim.x >= (unsigned)kFrameGridCapLarge);   // only the large-frame launch has that many workgroups
}
constexpr float kEps = 1e-4f;        // Miro.h:9
constexpr float kInf = __builtin_huge_valf();

#ifdef MIRO_RUN_COUNTS
// measurement build only (make VARIANT=_runc FRAME_DEFS=-DMIRO_RUN_COUNTS; tools/run_counts.py): wave-level node visits of the
// fused frame kernel -- those taken outside uniform_run, those inside it, and those at which a run ended on a split decision.
// One lane of the wave counts each event, so the sum over lanes is the number of wave-visits.
// ... and how the uniform walks go: walks entered, those of them whose lanes are all the lanes of
// the wave that still have work ("whole"), how a walk ends besides a split decision -- at a leaf it may not take, at a pop it
// may not take, at an irregular node, at a node of kRunNodeLimit or more, with every lane done --, the leaves taken inside a
// walk, and the pops inside a walk after which the lanes hold one value / different values.
// ... and the triangle tests of the uniform leaf loops that carry the rejection guard (item 24): wave-level tests, and those of
// them the guard skipped.
constexpr int kRunCounters = 15;
struct Stats {
    unsigned long long box, tri;
    unsigned node_steps, run_visits, run_splits;
    unsigned walks, walks_whole, end_leaf, end_pop, end_irregular, end_far_node, end_done, walk_leaves, pops_agree, pops_differ;
    unsigned tri_uniform, tri_skipped;
};
__device__ __forceinline__ void run_count_once(unsigned &c) {
    const int lane = (int)__lane_id();
    if (__builtin_amdgcn_readfirstlane(lane) == lane) c++;
}
#define MR_RUN_COUNT(field) run_count_once(field)
#else
struct Stats { unsigned long long box, tri; };
#define MR_RUN_COUNT(field) ((void)0)      /* the counters are fields of the counting build's Stats only */
#endif

// The integer codes of a walk (values as ever: the profile logs print the numbers) and the type that carries them.
// Slab form: how a node visit computes and compares the entry / exit distances of its two child boxes.
constexpr int kSlabSelect     = 0;   // the reference's select chains (slab_axis: a NaN falls through every comparison) on the products (corner - o) * (1/d)
constexpr int kSlabMinMax     = 1;   // min/max on the same products (slab_box_minmax): the same decisions for rays that cannot produce a NaN
constexpr int kSlabLean       = 2;   // lean fma form (slab_box_lean, MR_MATH_FAST): distances that differ from the products by rounding
constexpr int kSlabQuotient   = 3;   // select chains on the reference's true quotients (corner - o) / d: the reference's own arithmetic
constexpr int kSlabCorrection = 4;   // min/max on products with one correction step (exact_quot): the quotients without a division, regular rays in regular nodes
constexpr int kSlabGuarded    = 5;   // guarded products: plain products where they provably decide as the quotients do, kSlabCorrection where not (node_slabs_guarded)
constexpr int kSlabGuardedT0  = 6;   // ... for waves whose rays all have tMin == 0 (the octant loops): three pairs to guard instead of five
constexpr bool slab_guarded(int s) { return s == kSlabGuarded || s == kSlabGuardedT0; }
constexpr bool slab_nan_free(int s) { return s == kSlabMinMax || s == kSlabLean || s == kSlabCorrection || slab_guarded(s); }   // no distance is a NaN: node_decide's SAFE form
constexpr bool slab_divides_irregular(int s) { return s == kSlabCorrection || slab_guarded(s); }   // an irregular node takes kSlabQuotient instead
constexpr bool slab_has_octant_body(int s) { return s == kSlabMinMax || s == kSlabLean || s == kSlabCorrection; }   // slab_box_oct
constexpr bool slab_needs_tmin0(int s) { return s == kSlabGuardedT0; }
// Control flow of traverse().  The order of every lane's own steps -- and so its hit record -- is the same in all three.
constexpr int kFlowLane       = 0;   // one step of whatever the lane needs per iteration (the reference's control flow, lane by lane)
constexpr int kFlowWhileWhile = 1;   // "while-while": lanes run inner nodes until each holds a leaf (or is done), then the wave does the leaves
// voting: every iteration the wave counts the lanes that need a node step and those that need a triangle test and runs the step the
// majority needs; the others wait one round.  In while-while a wave's node loop lasts as long as its slowest lane's search for a leaf
// (incoherent batches: 14 of 64 lanes active per VALU instruction, profiles/r02_before_random); with the vote at least half of the
// unfinished lanes are active in every step.
constexpr int kFlowVote       = 2;
constexpr int kNoOct = 8;            // octant of a walk whose wave's rays share none (0..7, bit k set: direction component k is negative)
constexpr bool is_octant(int oct) { return oct != kNoOct; }

// One walk: what traverse, node_step, leaf_step, tri_step, node_slabs, node_slabs_guarded and uniform_run are instantiated on.
//   scalar: try the wave-uniform scalar-load path first (nodes and leaves)     obj: leaves may hold spheres     rel: eye-relative tables
//   run: ... and stay on the scalar side while the lanes decide alike (uniform_run; the octant loops of the fused frame kernel)
template <bool EXACT, bool ANY, bool STATS, int SLAB, int FLOW, bool SCALAR, bool OBJ, int OCT, bool REL, bool RUN>
struct Walk {
    static constexpr bool exact = EXACT, any = ANY, stats = STATS, scalar = SCALAR, obj = OBJ, rel = REL, run = RUN;
    static constexpr int slab = SLAB, flow = FLOW, oct = OCT;
};
// the walk W with one thing changed
template <typename W, int S, int F = W::flow> using walk_slab = Walk<W::exact, W::any, W::stats, S, F, W::scalar, W::obj, W::oct, W::rel, W::run>;
template <typename W, int O> using walk_oct = Walk<W::exact, W::any, W::stats, W::slab, W::flow, W::scalar, W::obj, O, W::rel, W::run>;
template <typename W, bool S> using walk_scalar = Walk<W::exact, W::any, W::stats, W::slab, W::flow, S, W::obj, W::oct, W::rel, W::run>;
template <typename W, bool R> using walk_run = Walk<W::exact, W::any, W::stats, W::slab, W::flow, W::scalar, W::obj, W::oct, W::rel, R>;
// the visit of an irregular node: the reference's own divisions, with no octant body
template <typename W> using walk_divide = walk_oct<walk_slab<W, kSlabQuotient>, kNoOct>;

// ---------------------------------------------------------------------------------------------------
// slab test of one box.  EXACT keeps the reference's predicate structure literally (BVH.cpp:599-608):
// NaNs (0 * inf when the origin sits on a slab plane of an axis the ray does not move along) fall
// through every comparison.  `inv` is 1/d, correctly rounded; STRICT divides instead (bit-equal to
// the reference's (corner - o) / d, used when the -DSTATS counters must match exactly).
// ---------------------------------------------------------------------------------------------------
template <bool STRICT>
__device__ __forceinline__ void slab_axis(float lo, float hi, float o, float d, float inv, float &mn, float &mx) {
    float t0, t1;
    if (STRICT) { t0 = (lo - o) / d; t1 = (hi - o) / d; }
    else        { t0 = (lo - o) * inv; t1 = (hi - o) * inv; }
    const bool m = t0 > t1;
    const float tnear = m ? t1 : t0, tfar = m ? t0 : t1;
    if (tnear > mn) mn = tnear;
    if (tfar < mx) mx = tfar;
}

struct RayRegs {
    float ox, oy, oz, dx, dy, dz;     // origin, direction
    float ix, iy, iz;                 // 1/d
    float mx_, my_, mz_;              // -d (Triangle.cpp:152 uses dot(-r.d, ...))
    float tmin;
    float nox, noy, noz;              // -(o * 1/d): slab distance = fma(corner, 1/d, nox)   (lean slab form)
};

__device__ __forceinline__ void ray_setup(RayRegs &r, const float4 ra, const float4 rb) {
    r.ox = ra.x; r.oy = ra.y; r.oz = ra.z; r.tmin = ra.w;
    r.dx = rb.x; r.dy = rb.y; r.dz = rb.z;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    r.mx_ = -r.dx; r.my_ = -r.dy; r.mz_ = -r.dz;
    r.nox = -(r.ox * r.ix); r.noy = -(r.oy * r.iy); r.noz = -(r.oz * r.iz);
}

// A slab distance (corner - o) * (1/d) -- or fma(corner, 1/d, -(o/d)) -- can only be NaN as 0*inf, inf*0 or
// inf-inf: with o, d, 1/d and o/d all finite (corners are finite or +-inf) none of these can occur, and the
// select form of the reference and the min/max forms take the same decisions.
__device__ __forceinline__ bool lane_is_nan_free(const RayRegs &r) {
    return (__builtin_fabsf(r.ox) < kInf) && (__builtin_fabsf(r.oy) < kInf) && (__builtin_fabsf(r.oz) < kInf) &&
           (__builtin_fabsf(r.dx) < kInf) && (__builtin_fabsf(r.dy) < kInf) && (__builtin_fabsf(r.dz) < kInf) &&
           (__builtin_fabsf(r.ix) < kInf) && (__builtin_fabsf(r.iy) < kInf) && (__builtin_fabsf(r.iz) < kInf) &&
           (__builtin_fabsf(r.nox) < kInf) && (__builtin_fabsf(r.noy) < kInf) && (__builtin_fabsf(r.noz) < kInf);
}

// three-input min/max in one VALU op; inline asm so that no canonicalising v_max x,x is inserted
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float o;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c));
    return o;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float o;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c));
    return o;
}

// two-input min/max as single VALU ops (no canonicalising v_max x,x in front, no NaN quieting: callers guarantee
// NaN-free operands or want exactly the hardware's minNum/maxNum behaviour)
__device__ __forceinline__ float vmax2(float a, float b) {
    float o;
    asm("v_max_f32 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b));
    return o;
}
__device__ __forceinline__ float vmin2(float a, float b) {
    float o;
    asm("v_min_f32 %0, %1, %2" : "=v"(o) : "v"(a), "v"(b));
    return o;
}

// |a - b| of two bit patterns as unsigned integers, and a three-way unsigned minimum: one VALU op each
__device__ __forceinline__ unsigned vsad(float a, float b) {
    unsigned o;
    asm("v_sad_u32 %0, %1, %2, 0" : "=v"(o) : "v"(a), "v"(b));
    return o;
}
__device__ __forceinline__ unsigned vmin3u(unsigned a, unsigned b, unsigned c) {
    unsigned o;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c));
    return o;
}

// min/max slab test of one child box for NaN-free rays on the reference's own products (corner - o) * (1/d):
// 6 sub + 6 mul + 3 min + 3 max + max3 + min3.  Same entry/exit values as the select chain of slab_axis (up to
// the sign of a zero, which no comparison sees).
__device__ __forceinline__ void slab_box_minmax(float lox, float hix, float loy, float hiy, float loz, float hiz,
                                                const RayRegs &r, float &mn, float &mx) {
    const float ax = (lox - r.ox) * r.ix, bx = (hix - r.ox) * r.ix;
    const float ay = (loy - r.oy) * r.iy, by = (hiy - r.oy) * r.iy;
    const float az = (loz - r.oz) * r.iz, bz = (hiz - r.oz) * r.iz;
    mn = vmax3(vmin2(ax, bx), vmin2(ay, by), vmin2(az, bz));
    mx = vmin3(vmax2(ax, bx), vmax2(ay, by), vmax2(az, bz));
}

// The reference's quotient (corner - o) / d without a division: with inv = RN(1/d) and q = RN(a * inv), one
// correction step q' = fma(fma(-q, d, a), inv, q) is the correctly rounded a / d (Markstein's theorem; checked on this
// GPU against v_div_* over 1.1e11 operand pairs incl. every mantissa of a and of d, tools/div_identity_probe.hip) as
// long as nothing under- or overflows on the way.  Callers guarantee that: "regular" rays (lane_is_regular) on
// "regular" nodes (flag in the node record) keep a, d, q well inside the normal range.
__device__ __forceinline__ float exact_quot(float a, float d, float inv) {
    const float q = a * inv;
    return __builtin_fmaf(__builtin_fmaf(-q, d, a), inv, q);
}

// min/max slab test on those exact quotients: the reference's entry/exit distances themselves (up to the sign of a
// zero), 12 VALU more per box than slab_box_minmax and none of its tie caveats.
__device__ __forceinline__ void slab_box_exactq(float lox, float hix, float loy, float hiy, float loz, float hiz,
                                                const RayRegs &r, float &mn, float &mx) {
    const float ax = exact_quot(lox - r.ox, r.dx, r.ix), bx = exact_quot(hix - r.ox, r.dx, r.ix);
    const float ay = exact_quot(loy - r.oy, r.dy, r.iy), by = exact_quot(hiy - r.oy, r.dy, r.iy);
    const float az = exact_quot(loz - r.oz, r.dz, r.iz), bz = exact_quot(hiz - r.oz, r.dz, r.iz);
    mn = vmax3(vmin2(ax, bx), vmin2(ay, by), vmin2(az, bz));
    mx = vmin3(vmax2(ax, bx), vmax2(ay, by), vmax2(az, bz));
}

// Octant-specialised forms (OCT bit k set: the ray's direction component k is negative; the octant is uniform over the
// wave).  Rounding is monotone -- RN(a * inv), fma(c, inv, n) and the correctly rounded quotient all grow with the corner
// when 1/d > 0 and shrink when 1/d < 0 -- and a box has lo <= hi on every axis (boxes that do not are "irregular" and take
// another path), so the smaller of an axis' two slab distances is the one of the lo corner for d > 0 and of the hi corner
// for d < 0: the six per-box min/max of the generic forms become a compile-time choice of operand.  Same entry / exit
// values (up to the sign of a zero), 12 VALU fewer per two-child visit.
template <int OCT, int SLAB>
__device__ __forceinline__ void slab_box_oct(float lox, float hix, float loy, float hiy, float loz, float hiz,
                                             const RayRegs &r, float &mn, float &mx) {
    const float nx = (OCT & 1) ? hix : lox, fx = (OCT & 1) ? lox : hix;
    const float ny = (OCT & 2) ? hiy : loy, fy = (OCT & 2) ? loy : hiy;
    const float nz = (OCT & 4) ? hiz : loz, fz = (OCT & 4) ? loz : hiz;
    switch (SLAB) {      // the forms of slab_has_octant_body
    case kSlabCorrection:
        mn = vmax3(exact_quot(nx - r.ox, r.dx, r.ix), exact_quot(ny - r.oy, r.dy, r.iy), exact_quot(nz - r.oz, r.dz, r.iz));
        mx = vmin3(exact_quot(fx - r.ox, r.dx, r.ix), exact_quot(fy - r.oy, r.dy, r.iy), exact_quot(fz - r.oz, r.dz, r.iz));
        break;
    case kSlabLean:
        mn = vmax3(fmaf(nx, r.ix, r.nox), fmaf(ny, r.iy, r.noy), fmaf(nz, r.iz, r.noz));
        mx = vmin3(fmaf(fx, r.ix, r.nox), fmaf(fy, r.iy, r.noy), fmaf(fz, r.iz, r.noz));
        break;
    default:             // kSlabMinMax
        mn = vmax3((nx - r.ox) * r.ix, (ny - r.oy) * r.iy, (nz - r.oz) * r.iz);
        mx = vmin3((fx - r.ox) * r.ix, (fy - r.oy) * r.iy, (fz - r.oz) * r.iz);
    }
}
__device__ __forceinline__ int octant_of(const RayRegs &r) {
    return (r.dx < 0.0f ? 1 : 0) | (r.dy < 0.0f ? 2 : 0) | (r.dz < 0.0f ? 4 : 0);
}

// magnitudes for which exact_quot is safe: direction components in [2^-40, 2^40], origin components 0 or in
// [2^-36, 2^60] (node corners obey the same bound when the node record's flag is clear, mr_api.cpp), so that a non-zero
// corner - o is at least 2^-59 and every intermediate stays a normal number
__device__ __forceinline__ bool regular_dir(float d) { const float a = __builtin_fabsf(d); return a >= 0x1p-40f && a <= 0x1p40f; }
__device__ __forceinline__ bool regular_pos(float o) { const float a = __builtin_fabsf(o); return a == 0.0f || (a >= 0x1p-36f && a <= 0x1p60f); }
__device__ __forceinline__ bool lane_is_regular(const RayRegs &r) {
    return regular_dir(r.dx) && regular_dir(r.dy) && regular_dir(r.dz) && regular_pos(r.ox) && regular_pos(r.oy) && regular_pos(r.oz);
}

// Lean slab test of one child box for NaN-free rays: 6 fma + 3 min + 3 max + max3 + min3.  Entry/exit
// distances differ from (corner - o) * (1/d) by rounding only; the decisions taken from them (cull, order) are
// protected by the epsilon padding of every box (BVH.cpp:75-79) -- see DESIGN.md section 5.
__device__ __forceinline__ void slab_box_lean(float lox, float hix, float loy, float hiy, float loz, float hiz,
                                              const RayRegs &r, float &mn, float &mx) {
    const float ax = fmaf(lox, r.ix, r.nox), bx = fmaf(hix, r.ix, r.nox);
    const float ay = fmaf(loy, r.iy, r.noy), by = fmaf(hiy, r.iy, r.noy);
    const float az = fmaf(loz, r.iz, r.noz), bz = fmaf(hiz, r.iz, r.noz);
    mn = vmax3(fminf(ax, bx), fminf(ay, by), fminf(az, bz));
    mx = vmin3(fmaxf(ax, bx), fmaxf(ay, by), fmaxf(az, bz));
}

// ---------------------------------------------------------------------------------------------------
// Triangle::intersect (Triangle.cpp:150-158).  q0..q2 = the 48-byte record.  Returns true when the
// reference's reject test passes with tMax = best; outputs t, beta, gamma.
// ---------------------------------------------------------------------------------------------------
// The origin's share of the exact Triangle::intersect: p = o - A, dot(p, n), u = cross(p, C-A), w = cross(B-A, p), each
// fp32 op rounded on its own in the reference's order.  tri_test<true> calls these per ray; the eye-relative table of the
// fused frame (mr_frame.hip: eye_tables) calls them once per frame for o = the camera eye through tri_origin_terms -- the
// same functions, so the stored terms are the bits tri_test<true> would compute for every primary ray.
// (q0..q2: A, B-A, C-A, (B-A)x(C-A) as in the record; tri_test<true> interleaves the pieces with the direction's terms as
// before -- computing all of them first cost the 267 frame kernel two spilled registers.)
__device__ __forceinline__ float3 tri_p(const float4 q0, float ox, float oy, float oz) {
    return make_float3(ox - q0.x, oy - q0.y, oz - q0.z);                                 // o - A
}
__device__ __forceinline__ float tri_pn(const float3 p, const float4 q2) {
    return (p.x * q2.y + p.y * q2.z) + p.z * q2.w;                                       // dot(o - A, n)
}
__device__ __forceinline__ float3 tri_u(const float3 p, const float4 q1, const float4 q2) {
    const float Cx = q1.z, Cy = q1.w, Cz = q2.x;                                         // cross(o - A, C - A)
    return make_float3(p.y * Cz - p.z * Cy, p.z * Cx - p.x * Cz, p.x * Cy - p.y * Cx);
}
__device__ __forceinline__ float3 tri_w(const float3 p, const float4 q0, const float4 q1) {
    const float Bx = q0.w, By = q1.x, Bz = q1.y;                                         // cross(B - A, o - A)
    return make_float3(By * p.z - Bz * p.y, Bz * p.x - Bx * p.z, Bx * p.y - By * p.x);
}
struct TriOriginTerms { float pn; float3 u, w; };
__device__ __forceinline__ TriOriginTerms tri_origin_terms(const float4 q0, const float4 q1, const float4 q2, float ox, float oy,
                                                           float oz) {
    const float3 p = tri_p(q0, ox, oy, oz);
    TriOriginTerms o;
    o.pn = tri_pn(p, q2);
    o.u = tri_u(p, q1, q2);
    o.w = tri_w(p, q0, q1);
    return o;
}

template <bool EXACT>
__device__ __forceinline__ bool tri_test(const float4 q0, const float4 q1, const float4 q2, const RayRegs &r,
                                         float tmax, float &t, float &beta, float &gamma) {
    if (EXACT) {
        const float nx = q2.y, ny = q2.z, nz = q2.w;      // (B-A) x (C-A)
        const float3 p = tri_p(q0, r.ox, r.oy, r.oz);
        const float ddotn = (r.mx_ * nx + r.my_ * ny) + r.mz_ * nz;
        t = tri_pn(p, q2) / ddotn;
        // (Leaving with "rejected" as soon as t alone rejects the triangle in every active lane -- skipping the two other
        // divisions and both cross products -- was measured: 16.21 vs 16.32 Grays/s on the bench frame, 7.56 vs 7.65 at 1 spp:
        // the wave-wide test costs more than the rare whole-wave rejection saves, profiles/r03_t_first_ab.log.)
        const float3 u = tri_u(p, q1, q2);
        beta = ((r.mx_ * u.x + r.my_ * u.y) + r.mz_ * u.z) / ddotn;
        const float3 w = tri_w(p, q0, q1);
        gamma = ((r.mx_ * w.x + r.my_ * w.y) + r.mz_ * w.z) / ddotn;
    } else {
        const float Bx = q0.w, By = q1.x, Bz = q1.y;      // B - A
        const float Cx = q1.z, Cy = q1.w, Cz = q2.x;      // C - A
        const float nx = q2.y, ny = q2.z, nz = q2.w;      // (B-A) x (C-A)
        const float px = r.ox - q0.x, py = r.oy - q0.y, pz = r.oz - q0.z;   // o - A
        const float ddotn = fmaf(r.mz_, nz, fmaf(r.my_, ny, r.mx_ * nx));
        const float rcp = __builtin_amdgcn_rcpf(ddotn);
        t = fmaf(pz, nz, fmaf(py, ny, px * nx)) * rcp;
        const float ux = fmaf(py, Cz, -(pz * Cy)), uy = fmaf(pz, Cx, -(px * Cz)), uz = fmaf(px, Cy, -(py * Cx));
        beta = fmaf(r.mz_, uz, fmaf(r.my_, uy, r.mx_ * ux)) * rcp;
        const float wx = fmaf(By, pz, -(Bz * py)), wy = fmaf(Bz, px, -(Bx * pz)), wz = fmaf(Bx, py, -(By * px));
        gamma = fmaf(r.mz_, wz, fmaf(r.my_, wy, r.mx_ * wx)) * rcp;
    }
    // reject iff beta < -eps || gamma < -eps || beta+gamma > 1+eps || t < tMin || t > tMax  (:158)
    const bool reject = (beta < -kEps) || (gamma < -kEps) || (beta + gamma > 1 + kEps) || (t < r.tmin) || (t > tmax);
    return !reject;
}

// The exact test on an eye-relative record (REL traversals: every ray starts at the origin of the table, the eye):
// q0 = (n, dot(eye - A, n)), q1 = (u, w.x), q2 = (w.y, w.z) from tri_origin_terms.  What is left per ray is what depends on
// the direction -- dot(-d, n), the two numerator dots, the three divisions and the reject test -- on the same operands in
// the same order as tri_test<true>: the same t, beta, gamma.
__device__ __forceinline__ bool tri_test_rel(const float4 q0, const float4 q1, const float2 q2, const RayRegs &r,
                                             float tmax, float &t, float &beta, float &gamma) {
    const float ddotn = (r.mx_ * q0.x + r.my_ * q0.y) + r.mz_ * q0.z;
    t = q0.w / ddotn;
    beta = ((r.mx_ * q1.x + r.my_ * q1.y) + r.mz_ * q1.z) / ddotn;
    gamma = ((r.mx_ * q1.w + r.my_ * q2.x) + r.mz_ * q2.y) / ddotn;
    const bool reject = (beta < -kEps) || (gamma < -kEps) || (beta + gamma > 1 + kEps) || (t < r.tmin) || (t > tmax);
    return !reject;
}

// Sphere::intersect (Sphere.cpp:28-69) on the record (c.xyz, radius): the quadratic in the reference's order of
// operations, true divisions, strict range test on both roots.
__device__ __forceinline__ bool sphere_test(const float4 q0, const RayRegs &r, float tmax, float &t) {
    const float tx = r.ox - q0.x, ty = r.oy - q0.y, tz = r.oz - q0.z;       // toO = ray.o - m_center
    const float a = (r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz;               // ray.d.length2()
    const float b = ((r.dx * 2) * tx + (r.dy * 2) * ty) + (r.dz * 2) * tz;   // dot(2*ray.d, toO)
    const float c = ((tx * tx + ty * ty) + tz * tz) - q0.w * q0.w;
    const float discrim = b * b - 4.0f * a * c;
    if (discrim < 0) return false;
    const float sq = sqrtf(discrim);
    const float t0 = (-b - sq) / (2.0f * a), t1 = (-b + sq) / (2.0f * a);
    if ((t0 > r.tmin) && (t0 < tmax)) { t = t0; return true; }
    if ((t1 > r.tmin) && (t1 < tmax)) { t = t1; return true; }
    return false;
}

// the object test of a leaf slot: Triangle::intersect, or Sphere::intersect when OBJ and the record carries the tag;
// REL: the eye-relative record of tri_test_rel (triangle-only scenes, exact test)
template <bool EXACT, bool OBJ, bool REL = false>
__device__ __forceinline__ bool object_test(const float4 q0, const float4 q1, const float4 q2, const RayRegs &r,
                                            float tmax, float &t, float &beta, float &gamma) {
    static_assert(!REL || (EXACT && !OBJ), "eye-relative records hold exact triangle tests only");
    if (REL) return tri_test_rel(q0, q1, make_float2(q2.x, q2.y), r, tmax, t, beta, gamma);
    if (OBJ && __float_as_uint(q2.w) == kSphereTag) {
        beta = 0.0f; gamma = 0.0f;
        return sphere_test(q0, r, tmax, t);
    }
    return tri_test<EXACT>(q0, q1, q2, r, tmax, t, beta, gamma);
}

// The rejection guard of the uniform leaf loops.  In a uniform leaf the whole wave tests ONE
// triangle, and most of those tests end with every lane rejecting it: two or three IEEE division sequences (11 VALU each, one of
// them a quarter-rate v_rcp_f32) and the reject test computed for nothing.  A lane is SURE of the reference's rejection when, for the
// numerator nb of beta (or ng of gamma),
//     nb * k < -|ddotn|      with k = 2^13 carrying the sign bit of ddotn.
//   * Scaling by a power of two is exact (a denormal scaled UP stays exact); if nb * k overflows it is +-inf of the product's
//     sign, which keeps the inequality because |ddotn| is finite wherever the compare can hold (ddotn = +-inf: nothing is below
//     -inf, the lane is not sure) -- and |nb| * 2^13 >= 2^128 > |ddotn| then holds in the reals too.
//   * k has ddotn's sign, so nb * k = 2^13 * nb * sgn(ddotn): the compare says nb * sgn(ddotn) * 2^13 < -|ddotn|, that is
//     nb / ddotn < -2^-13 in the reals for ddotn != 0.  The sign bit is read as a bit, which is what IEEE division does with
//     +-0: for ddotn = +0 the lane is sure iff nb < 0 and the reference's quotient is -inf; for ddotn = -0 iff nb > 0, again -inf;
//     nb = +-0 over ddotn = +-0 is NaN in the reference and 0 < -0 is false here.
//   * Rounding is monotone and 2^-13 is a float: the real quotient below -2^-13 rounds to a quotient <= -2^-13 < -1e-4f = -kEps
//     (2^-13 = 1.2207e-4), so the reference's `beta < -epsilon` (Triangle.cpp:158) rejects the triangle.
//   * A NaN operand fails every compare: the lane is not sure.
// When every lane that takes part is sure the test is skipped: a rejected test writes nothing, so hit records and pixels keep
// their bits.  Otherwise the wave runs the test as it was -- the same quotients of the same operands, the same reject test.
// Cost: v_and + v_or for k, two v_mul, and the two compares as the compiler emits them -- one v_min and one v_cmp with source
// modifiers (minNum keeps the number when one product is a NaN: the same decision) --, one scalar compare of the mask with exec, a branch.
__device__ __forceinline__ bool tri_surely_rejects(float nb, float ng, float ddotn) {
    // 2^13 with ddotn's sign.  (Two VOP2 instructions that carry their constants as literals: written as an and-or the constant
    // is moved to a vector register of its own in front of the frame's loop, alive through the whole kernel.)
    float k;
    asm("v_and_b32 %0, 0x80000000, %1\n\tv_or_b32 %0, 0x46000000, %0" : "=v"(k) : "v"(ddotn));
    const float lim = -__builtin_fabsf(ddotn);
    return (nb * k < lim) || (ng * k < lim);
}

// the exact triangle test of a uniform leaf behind that guard: ddotn and the numerators of beta and gamma by today's operations
// (tri_test<true> / tri_test_rel: for the scene's own records that includes p, u and w), the guard, and -- unless every lane is
// sure -- the three divisions and the reject test on those operands.  False for a skipped test, t / beta / gamma unwritten.
template <bool REL>
__device__ __forceinline__ bool tri_test_guarded(const float4 q0, const float4 q1, const float4 q2, const RayRegs &r, float tmax,
                                                 float &t, float &beta, float &gamma, Stats &st) {
    float ddotn, pn, nb, ng;
    if (REL) {
        ddotn = (r.mx_ * q0.x + r.my_ * q0.y) + r.mz_ * q0.z;
        nb = (r.mx_ * q1.x + r.my_ * q1.y) + r.mz_ * q1.z;
        ng = (r.mx_ * q1.w + r.my_ * q2.x) + r.mz_ * q2.y;
        pn = q0.w;
    } else {
        const float3 p = tri_p(q0, r.ox, r.oy, r.oz);
        ddotn = (r.mx_ * q2.y + r.my_ * q2.z) + r.mz_ * q2.w;
        pn = tri_pn(p, q2);
        const float3 u = tri_u(p, q1, q2);
        nb = (r.mx_ * u.x + r.my_ * u.y) + r.mz_ * u.z;
        const float3 w = tri_w(p, q0, q1);
        ng = (r.mx_ * w.x + r.my_ * w.y) + r.mz_ * w.z;
    }
    MR_RUN_COUNT(st.tri_uniform);
    if (__builtin_amdgcn_ballot_w64(tri_surely_rejects(nb, ng, ddotn)) == __builtin_amdgcn_ballot_w64(true)) {
        MR_RUN_COUNT(st.tri_skipped);
        return false;
    }
    // Triangle.cpp:158's reject test in its own order of comparisons, t divided only for the lanes that beta and gamma let through
    // (what the compiler makes of tri_test's `||` chain by itself; behind the guard's branch it has to be told)
    beta = nb / ddotn;
    gamma = ng / ddotn;
    if ((beta < -kEps) || (gamma < -kEps) || (beta + gamma > 1 + kEps)) return false;
    asm("" : "+v"(ddotn));      // (an empty statement the division depends on: it is not computed ahead of the branch for every lane)
    t = pn / ddotn;
    return !((t < r.tmin) || (t > tmax));
}

// ---------------------------------------------------------------------------------------------------
// closest-hit / any-hit traversal, one ray per lane (its slab forms and control flows: the kVar... bits of mr_launch.h)
// ---------------------------------------------------------------------------------------------------
// `cur` is the node the lane is at: >= 0 inner node, < 0 leaf reference, kDone = no more work.  `sp` is the BYTE
// offset in LDS of the lane's next free stack slot (slots of one lane are kTraceBlock * 4 bytes apart); the bottom slot
// of every lane holds kDone, so a pop needs no emptiness test: popping the sentinel ends the ray.
constexpr int kDone = (int)0x80000000;
constexpr int kStackStride = kTraceBlock * (int)sizeof(int);
struct Lane {
    float best_t, best_b, best_g;
    int best_pos;
    int sp, cur;
    int lpos, lend;      // voting traversal only: next / one-past-last triangle of the leaf in progress (lpos == lend: not begun)
    __device__ __forceinline__ bool have() const { return cur != kDone; }
};

// L.sp is the lane's stack pointer as an ABSOLUTE LDS address (the base of the dynamic LDS block is added once, in
// stack_reset): a push or pop is one ds instruction on that register -- through a generic `s_stack + offset` the compiler
// emitted a v_add with the (link-time) base in front of every one of them.
typedef __attribute__((address_space(3))) int lds_int;
__device__ __forceinline__ void stack_push(Lane &L, int *s_stack, int v) {
    *reinterpret_cast<lds_int *>((unsigned)L.sp) = v;
    L.sp += kStackStride;
}
__device__ __forceinline__ int stack_pop(Lane &L, int *s_stack) {
    L.sp -= kStackStride;
    return *reinterpret_cast<lds_int *>((unsigned)L.sp);
}
__device__ __forceinline__ void stack_reset(Lane &L, int *s_stack, int tid) {
    L.sp = (int)(unsigned)reinterpret_cast<__UINTPTR_TYPE__>((lds_int *)s_stack) + tid * (int)sizeof(int);
    stack_push(L, s_stack, kDone);
}

// One 64-byte node record through the scalar data cache: when every active lane of the wave sits at the same
// node (coherent camera / shadow rays near the top of the tree), one s_load_dwordx16 replaces 64 lanes x 4
// global_load_dwordx4 -- the vector L1 (64 B/clk/CU) is what bounds this kernel (profiles/r01_pmc_sq.txt).
typedef float v16f __attribute__((ext_vector_type(16)));
__device__ __forceinline__ v16f load_node_scalar(const float4 *nodes, int cur_uniform) {
    const float4 *ptr = nodes + 4 * (size_t)cur_uniform;
    v16f v;
    asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(ptr) : "memory");
    return v;
}

template <typename W>
__device__ __forceinline__ void node_slabs(const float4 q0, const float4 q1, const float4 q2, const RayRegs &r,
                                           float &mn0, float &mx0, float &mn1, float &mx1);
template <typename W>
__device__ __forceinline__ void node_slabs_guarded(const float4 q0, const float4 q1, const float4 q2, const RayRegs &r, float best_t,
                                                   float &mn0, float &mx0, float &mn1, float &mx1, float &k0, float &k1);

// the post-test bookkeeping of BVH.cpp:609-651: near child first (ties -> child 0), far child pushed, else pop
// HAVE_K: the caller already holds k0 = minNum(mx0, best_t), k1 = minNum(mx1, best_t) (node_slabs_guarded computes them for
// its tie test: recomputing them here cost two VALU instructions per visit of the hot loop)
template <bool STATS, bool SAFE, bool HAVE_K = false>
__device__ __forceinline__ void node_decide(float mn0, float mx0, float mn1, float mx1, int ref0, int ref1,
                                            const RayRegs &r, Lane &L, int *s_stack, Stats &st, float k0 = 0.0f, float k1 = 0.0f) {
    // tMax of this call == best_t: nothing changed since the node was entered
    bool h0, h1;
    if (SAFE) {
        // mn, mx are not NaN here; (mn > mx || mn > best) == (mn > minNum(mx, best)) also when best is NaN
        if (!HAVE_K) { k0 = vmin2(mx0, L.best_t); k1 = vmin2(mx1, L.best_t); }
        h0 = !((mn0 > k0) || (mx0 < r.tmin));
        h1 = !((mn1 > k1) || (mx1 < r.tmin));
    } else {
        h0 = !((mn0 > mx0) || (mn0 > L.best_t) || (mx0 < r.tmin));
        h1 = !((mn1 > mx1) || (mn1 > L.best_t) || (mx1 < r.tmin));
    }
    const bool one_first = h1 && (!h0 || (mn0 > mn1));
    // (a select-only formulation with predicated push/pop was measured 5 % slower than this branch nest)
    if (h0 && h1) {
        stack_push(L, s_stack, one_first ? ref0 : ref1);
        L.cur = one_first ? ref1 : ref0;
        if (STATS) st.box++;
    } else if (h0 || h1) {
        L.cur = h0 ? ref0 : ref1;
        if (STATS) st.box++;
    } else {
        L.cur = stack_pop(L, s_stack);        // the far child is entered unconditionally (:640-650); kDone at the bottom
        if (STATS && L.cur != kDone) st.box++;
    }
}

// The uniform run (octant loops with the three-pair guard, kSlabGuardedT0, of the fused frame kernel): entered by node_step once its test
// has found every active lane of the wave at the node `cur`; from there `cur` is a SCALAR for as long as the lanes also take the
// same decision.  At 64 samples per pixel a wave is one pixel -- 64 jittered rays through it, or 64 shadow rays from one patch
// of surface to one light -- and what node_step pays per visit for lanes that may part at any moment (v_readfirstlane + v_cmp +
// branch to find the wave at one node again, the exec-mask nest of node_decide, the child references moved to VGPRs and selected
// per lane for L.cur and the push) is then spent on finding out what the compare masks already say: all active lanes hit both
// children with the same near one, all hit only child 0, all only child 1, or none hits either.  In the first three cases the
// next node is the scalar child reference and the far one, if any, is pushed from one v_mov; the loop goes on without touching
// L.cur.  Otherwise -- a split decision, an irregular node, and for a run that holds only SOME of the wave's working lanes
// (uniform_run) a pop or a leaf too -- L.cur is written per lane exactly as node_decide writes it and the run ends: node_step's
// own test starts the next one.  A run that holds ALL of them goes on through pops and leaves (uniform_walk, below).  Same bits: every floating-point instruction of a visit is the one node_step issues (the same load_node_scalar,
// node_slabs_guarded -- its wave-wide exact-quotient recomputation included -- and, for irregular nodes, walk_divide) on the
// same operands; every lane keeps its own stack, pushes what node_decide would have pushed and visits the nodes in the same
// order -- a wave in the run is a wave for which node_step's test would have succeeded at every visit.  Nothing is shared between
// the lanes but the knowledge that their values are equal, so leaving the run needs no recovery step.
// The scalar side of a visit in the run.  The run keeps its node as a BYTE offset into the table:
// the scalar load adds a 32-bit offset register to its base itself, so one shift stands where a sign extension, a 64-bit shift
// and a 64-bit add stood in front of every load.  Offsets stay below 2^31 -- the run is for node indices below kRunNodeLimit;
// in a larger table the nodes beyond are visited lane by lane (node_step's per-lane visit, which is right for any node).
constexpr unsigned kRunNodeLimit = 1u << 25;
__device__ __forceinline__ v16f load_node_scalar_at(const float4 *nodes, unsigned off) {
    v16f v;
    asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(nodes), "s"(off) : "memory");
    return v;
}
// How a descent ends travels in `cur` itself: the loop of visits keeps ONE exit and one scalar test for it.  `cur` is the next node
// while the descent goes on, and otherwise a child reference that is no node of the run (a leaf; an index of kRunNodeLimit or more)
// or one of the values below that are no reference at all.  (Leaf references end at ~((2^27 - 2) << 4 | 15) = 0x80000010:
// mr_api.cpp refuses 2^27 records or more.)
//
// The uniform walk (uniform_walk): the run of a wave whose lanes at the node are ALL its lanes that
// still have work (m_have, traverse's own ballot of L.have()).  It does not end at a leaf or a pop:
//   * `cur` a leaf reference (closest-hit walks): the uniform leaf loop runs in place -- leaf_step's scalar arm: the same
//     load_tri_uniform, object_test, triangle order, strict-less replacement and running best_t, the leaf_cnt_ext lookup for the
//     extended count -- and then the lanes pop;
//   * no lane hits a child: the lanes pop;
//   * a pop: every lane pops ITS OWN stack; one v_readfirstlane and one compare say whether the values are equal.
//     Equal: `cur` is that value (kDone: the wave has finished).  Not equal: the walk ends with L.cur as popped.
// A run that holds a subset of the working lanes is uniform_run, unchanged: the others wait at their leaves, and going on without
// them would undo the while-while grouping (1-spp frames).  An any-hit walk ends at every leaf (a lane that is done leaves the wave's
// working set there) and takes the pops.  Same bits: every floating-point instruction is one node_step / leaf_step issue on the
// same operands, every lane visits the same nodes and triangles in the same order with its own stack and its own best_t -- a wave
// in the walk is one for which node_step's and leaf_step's uniformity tests would have succeeded at every step; the only new
// knowledge used is that the popped values are equal.
// Shape: the visits of a descent keep the run's own loop and foot; the pop and the leaves sit behind it.  Nothing of a visit is
// carried out of that loop (child references and distances would be alive across the leaves: a spilled sixteen-register tuple,
// six vector registers), so a visit that node_decide has to finish is computed again behind the loops.
constexpr int kRunIrregular = kDone + 1;
constexpr int kWalkDecide = kDone + 2;       // node_decide has to finish the visit lane by lane (split decision)
constexpr int kWalkParted = kDone + 3;       // the lanes popped different values
constexpr int kWalkPop = kDone + 4;          // (inside the walk only) no lane hits a child
constexpr int kWalkFirstLeaf = kDone + 16;   // the smallest leaf reference (above)

template <bool REL>
__device__ __forceinline__ void load_tri_uniform(const float4 *tris, unsigned pos_uniform, float4 &q0, float4 &q1, float4 &q2);

// the walks whose uniform leaf loops carry the rejection guard (tri_test_guarded): those that take the uniform run -- the octant
// loops of the fused frame kernel's eye-relative, uniform-material forms, both traces; exact triangle records only
template <typename W> constexpr bool walk_guards_tris() {
    return W::run && slab_needs_tmin0(W::slab) && is_octant(W::oct) && !W::stats && W::exact && !W::obj;
}
// the object test of a uniform leaf: behind the guard in those walks, object_test as ever in all others.
// IN_WALK: the leaf loop of uniform_walk (else leaf_step's scalar arm).  The walk's loop carries the guard on the eye-relative
// tables only: with it in the shadow trace's walk as well -- numerators first or beta before w, the divisions in any order or
// chained one behind the other -- frame_kernel<794, 0, false> spills 6 vector registers / 28 bytes of scratch against the 4 / 20
// of tests/golden/kernel_budget.json, so that loop keeps today's code.
template <typename W, bool IN_WALK = false>
__device__ __forceinline__ bool uniform_object_test(const float4 q0, const float4 q1, const float4 q2, const RayRegs &r, float tmax,
                                                    float &t, float &beta, float &gamma, Stats &st) {
    if constexpr (walk_guards_tris<W>() && (W::rel || !IN_WALK)) return tri_test_guarded<W::rel>(q0, q1, q2, r, tmax, t, beta, gamma, st);
    else return object_test<W::exact, W::obj, W::rel>(q0, q1, q2, r, tmax, t, beta, gamma);
}

template <typename W>
__device__ __forceinline__ void uniform_run(const TraceParams &p, const RayRegs &r, Lane &L, int *s_stack, Stats &st, int cur) {
    const unsigned long long m_all = __builtin_amdgcn_ballot_w64(true);
    float mn0, mx0, mn1, mx1, k0, k1;        // (written by every visit that can reach node_decide<.., true, true> below)
    int ref0, ref1;
    unsigned off;
    MR_RUN_COUNT(st.walks);
    do {
        off = (unsigned)cur << 6;
        const v16f v = load_node_scalar_at(p.nodes, off);
        const float4 q0 = make_float4(v[0], v[1], v[2], v[3]), q1 = make_float4(v[4], v[5], v[6], v[7]);
        const float4 q2 = make_float4(v[8], v[9], v[10], v[11]);
        // (moved out of the record's sixteen-register tuple by hand: as parts of it they keep the whole tuple alive to the loop's exit
        // and beyond, and next to the walk's loops the tuple is then spilled -- 64 bytes of scratch per lane)
        asm("s_mov_b32 %0, %2\n\ts_mov_b32 %1, %3" : "=&s"(ref0), "=&s"(ref1) : "s"(__float_as_int(v[12])), "s"(__float_as_int(v[13])));
        MR_RUN_COUNT(st.run_visits);
        cur = kRunIrregular;
        if (__float_as_int(v[14]) == 0) {
            cur = kDone;
            k0 = 0.0f; k1 = 0.0f;
            node_slabs_guarded<W>(q0, q1, q2, r, L.best_t, mn0, mx0, mn1, mx1, k0, k1);
            // node_decide's comparisons (its SAFE form) as lane masks: out = the lanes whose ray misses the child.  A compare mask
            // has zero bits for inactive lanes, so the masks need no and with m_all.
            const unsigned long long out0 = __builtin_amdgcn_ballot_w64(mn0 > k0) | __builtin_amdgcn_ballot_w64(mx0 < r.tmin);
            const unsigned long long out1 = __builtin_amdgcn_ballot_w64(mn1 > k1) | __builtin_amdgcn_ballot_w64(mx1 < r.tmin);
            if ((out0 | out1) == 0ull) {                              // every lane hits both: near child first, ties -> child 0
                const unsigned long long one_first = __builtin_amdgcn_ballot_w64(mn0 > mn1);
                if (__builtin_expect(one_first == 0ull, 1)) { stack_push(L, s_stack, ref1); cur = ref0; }
                else if (one_first == m_all) { stack_push(L, s_stack, ref0); cur = ref1; }
            } else {                                                  // every lane hits child 0 only / child 1 only: no branch
                const bool only0 = (out0 | (out1 ^ m_all)) == 0ull, only1 = (out1 | (out0 ^ m_all)) == 0ull;
                cur = only0 ? ref0 : only1 ? ref1 : kDone;
            }
        }
    } while ((unsigned)cur < kRunNodeLimit);
    if (cur == kDone) {                                // no child hit in some lanes or all (pop), or the lanes part
        if (((unsigned long long)__builtin_amdgcn_ballot_w64((mn0 > k0) || (mx0 < r.tmin)) &
             (unsigned long long)__builtin_amdgcn_ballot_w64((mn1 > k1) || (mx1 < r.tmin))) != m_all) MR_RUN_COUNT(st.run_splits);
        else MR_RUN_COUNT(st.end_pop);
        node_decide<false, true, true>(mn0, mx0, mn1, mx1, ref0, ref1, r, L, s_stack, st, k0, k1);
    } else if (cur == kRunIrregular) {                 // the reference's own divisions, decided lane by lane
        MR_RUN_COUNT(st.end_irregular);
        // (the record is loaded a second time on purpose: kept live across the loop's exit its twelve corners cost the hot loop
        // scalar registers it spills for, and irregular nodes are rare -- a frame whose eye is irregular, where every visit comes
        // this way, pays the run's entry and two loads per visit and is slower than before)
        const v16f v = load_node_scalar_at(p.nodes, off);
        const float4 q0 = make_float4(v[0], v[1], v[2], v[3]), q1 = make_float4(v[4], v[5], v[6], v[7]);
        const float4 q2 = make_float4(v[8], v[9], v[10], v[11]);
        node_slabs<walk_divide<W>>(q0, q1, q2, r, mn0, mx0, mn1, mx1);
        node_decide<false, false>(mn0, mx0, mn1, mx1, ref0, ref1, r, L, s_stack, st);
    } else {                                           // a leaf: the wave's leaf_step finds it uniform by its own test
        L.cur = cur;
#ifdef MIRO_RUN_COUNTS
        if (cur < 0) MR_RUN_COUNT(st.end_leaf);
        else MR_RUN_COUNT(st.end_far_node);
#endif
    }
}

template <typename W>
__device__ __forceinline__ void uniform_walk(const TraceParams &p, const RayRegs &r, Lane &L, int *s_stack, Stats &st, int cur) {
    const unsigned long long m_all = __builtin_amdgcn_ballot_w64(true);
    // the leaves a walk takes: every leaf reference in a closest-hit walk, none in an any-hit one -- [kWalkFirstLeaf, 0) as one unsigned test
    constexpr unsigned leaf_span = W::any ? 0u : 0u - (unsigned)kWalkFirstLeaf;
    unsigned off;
    // each lane pops its own stack (kDone at the bottom): `cur` is the popped value when the lanes agree on it.  (The popped values live
    // for this test only: when they differ the slot is given back and popped again behind the loop -- L.cur carried round the loop
    // is a register of every visit.)
    auto pop_uniform = [&]() {
        const int mine = stack_pop(L, s_stack);
        cur = __builtin_amdgcn_readfirstlane(mine);
        if (__builtin_amdgcn_ballot_w64(mine == cur) != m_all) { cur = kWalkParted; L.sp += kStackStride; MR_RUN_COUNT(st.pops_differ); }
        else MR_RUN_COUNT(st.pops_agree);
    };
    MR_RUN_COUNT(st.walks);
    MR_RUN_COUNT(st.walks_whole);
    // The shape is a plain loop nest, so that best_t / best_b / best_g / best_pos stay in their registers from the walk's entry to its
    // exit: the visits of a descent -- the run's loop as it was, one scalar test at its foot --, behind them the pop and the leaves
    // that follow, each with its pop; in a leaf its triangles.
    for (;;) {
      do {      // (the descent)
        off = (unsigned)cur << 6;
        const v16f v = load_node_scalar_at(p.nodes, off);
        const float4 q0 = make_float4(v[0], v[1], v[2], v[3]), q1 = make_float4(v[4], v[5], v[6], v[7]);
        const float4 q2 = make_float4(v[8], v[9], v[10], v[11]);
        const int ref0 = __float_as_int(v[12]), ref1 = __float_as_int(v[13]);
        MR_RUN_COUNT(st.run_visits);
        cur = kRunIrregular;
        if (__float_as_int(v[14]) == 0) {
            cur = kWalkDecide;
            float mn0, mx0, mn1, mx1, k0 = 0.0f, k1 = 0.0f;
            node_slabs_guarded<W>(q0, q1, q2, r, L.best_t, mn0, mx0, mn1, mx1, k0, k1);
            // node_decide's comparisons (its SAFE form) as lane masks: out = the lanes whose ray misses the child.  A compare mask
            // has zero bits for inactive lanes, so the masks need no and with m_all.
            const unsigned long long out0 = __builtin_amdgcn_ballot_w64(mn0 > k0) | __builtin_amdgcn_ballot_w64(mx0 < r.tmin);
            const unsigned long long out1 = __builtin_amdgcn_ballot_w64(mn1 > k1) | __builtin_amdgcn_ballot_w64(mx1 < r.tmin);
            if ((out0 | out1) == 0ull) {                              // every lane hits both: near child first, ties -> child 0
                const unsigned long long one_first = __builtin_amdgcn_ballot_w64(mn0 > mn1);
                if (__builtin_expect(one_first == 0ull, 1)) { stack_push(L, s_stack, ref1); cur = ref0; }
                else if (one_first == m_all) { stack_push(L, s_stack, ref0); cur = ref1; }
            } else {                                                  // every lane hits child 0 only / child 1 only: no branch
                const bool only0 = (out0 | (out1 ^ m_all)) == 0ull, only1 = (out1 | (out0 ^ m_all)) == 0ull;
                cur = only0 ? ref0 : only1 ? ref1 : (out0 & out1) == m_all ? kWalkPop : kWalkDecide;
            }
        }
      } while ((unsigned)cur < kRunNodeLimit);
        if (cur == kWalkPop) pop_uniform();                           // no lane hits a child
        while ((unsigned)cur - (unsigned)kWalkFirstLeaf < leaf_span) {
            // a leaf, every lane of the walk in it (leaf_step's scalar arm)
            const unsigned bits = ~(unsigned)cur;
            const unsigned first0 = bits >> kLeafCountBits;
            unsigned cnt0 = bits & kLeafCountMask;
            if (cnt0 == kLeafCountMask) cnt0 = p.leaf_cnt_ext[first0];
            MR_RUN_COUNT(st.walk_leaves);
            for (unsigned k = 0; k < cnt0; k++) {
                float4 t0, t1, t2;
                load_tri_uniform<W::rel>(p.tris, first0 + k, t0, t1, t2);
                float t, b, g;
                const bool ok = uniform_object_test<W, true>(t0, t1, t2, r, L.best_t, t, b, g, st);
                if (ok && t < L.best_t) {             // strict-less replacement (BVH.cpp:500)
                    L.best_t = t; L.best_b = b; L.best_g = g; L.best_pos = (int)(first0 + k);
                }
            }
            pop_uniform();
        }
        if ((unsigned)cur >= kRunNodeLimit) break;
    }
    if (cur == kWalkParted) {                          // the lanes part at a pop
        L.cur = stack_pop(L, s_stack);
    } else if (cur == kWalkDecide) {                   // the lanes part: no child hit in some, a child in others, or another near one
        // node_step's visit of a node the wave shares, decided lane by lane.  (The record is loaded and the distances are computed a
        // second time on purpose, as below: six distances alive across the loop's exit are alive across its leaves.)
        const v16f v = load_node_scalar_at(p.nodes, off);
        const float4 q0 = make_float4(v[0], v[1], v[2], v[3]), q1 = make_float4(v[4], v[5], v[6], v[7]);
        const float4 q2 = make_float4(v[8], v[9], v[10], v[11]);
        float mn0, mx0, mn1, mx1, k0 = 0.0f, k1 = 0.0f;
        node_slabs_guarded<W>(q0, q1, q2, r, L.best_t, mn0, mx0, mn1, mx1, k0, k1);
#ifdef MIRO_RUN_COUNTS
        if (((unsigned long long)__builtin_amdgcn_ballot_w64((mn0 > k0) || (mx0 < r.tmin)) &
             (unsigned long long)__builtin_amdgcn_ballot_w64((mn1 > k1) || (mx1 < r.tmin))) != m_all) MR_RUN_COUNT(st.run_splits);
        else MR_RUN_COUNT(st.end_pop);
#endif
        node_decide<false, true, true>(mn0, mx0, mn1, mx1, __float_as_int(v[12]), __float_as_int(v[13]), r, L, s_stack, st, k0, k1);
    } else if (cur == kRunIrregular) {                 // the reference's own divisions, decided lane by lane
        MR_RUN_COUNT(st.end_irregular);
        // (the record is loaded a second time on purpose: kept live across the loop's exit its twelve corners -- or just its two child
        // references: they are part of the sixteen-register tuple -- cost the hot loop scalar registers it spills for, and irregular
        // nodes are rare -- a frame whose eye is irregular, where every visit comes this way, pays the run's entry and two loads per
        // visit and is slower than before)
        const v16f v = load_node_scalar_at(p.nodes, off);
        const float4 q0 = make_float4(v[0], v[1], v[2], v[3]), q1 = make_float4(v[4], v[5], v[6], v[7]);
        const float4 q2 = make_float4(v[8], v[9], v[10], v[11]);
        float mn0, mx0, mn1, mx1;
        node_slabs<walk_divide<W>>(q0, q1, q2, r, mn0, mx0, mn1, mx1);
        node_decide<false, false>(mn0, mx0, mn1, mx1, __float_as_int(v[12]), __float_as_int(v[13]), r, L, s_stack, st);
    } else {                                         // kDone: every lane popped its sentinel.  A leaf the walk may not take (the
        L.cur = cur;                                   // wave's leaf_step finds it uniform by its own test), a node of kRunNodeLimit or more
#ifdef MIRO_RUN_COUNTS
        if (cur == kDone) MR_RUN_COUNT(st.end_done);
        else if (cur < 0) MR_RUN_COUNT(st.end_leaf);
        else MR_RUN_COUNT(st.end_far_node);
#endif
    }
}

// the walks that take the uniform run: the octant loops with the three-pair guard, without counters
template <typename W> constexpr bool walk_runs() { return W::run && slab_needs_tmin0(W::slab) && is_octant(W::oct) && !W::stats; }

// one inner node (W::slab, W::scalar, W::oct, W::run: the slab forms and Walk at the top of this file)
// m_have (run walks): the lanes of the wave that had work when traverse last looked
template <typename W>
__device__ __forceinline__ void node_step(const TraceParams &p, const RayRegs &r, Lane &L, int *s_stack, int tid, Stats &st,
                                          unsigned long long m_have = 0ull) {
    float mn0, mx0, mn1, mx1;
    constexpr bool kStats = W::stats, kSafe = slab_nan_free(W::slab), kGuarded = slab_guarded(W::slab);
    if (W::scalar) {
        const int cur0 = __builtin_amdgcn_readfirstlane(L.cur);
        // (a wave of a run walk at a node beyond the run's offsets takes the per-lane visit below: it is correct for any node)
        constexpr bool kRuns = walk_runs<W>();
        if (__all(L.cur == cur0) && (!kRuns || (unsigned)cur0 < kRunNodeLimit)) {
            if (kRuns) {
                // The lanes the walk leaves at inner nodes take the per-lane visit below at once, as traverse's node loop would have
                // them do next.  (If-then and fall through, not if-else: laid out after the walk as its else branch, the per-lane visit
                // keeps the values L had BEFORE the walk alive all through it -- best_t / best_b / best_g / best_pos twice.)
                if ((unsigned long long)__builtin_amdgcn_ballot_w64(true) != m_have) {      // a subset of the working lanes: the run
                    uniform_run<W>(p, r, L, s_stack, st, cur0);
                    return;
                }
                uniform_walk<W>(p, r, L, s_stack, st, cur0);
                if (L.cur < 0) return;
            } else {
                MR_RUN_COUNT(st.node_steps);
                const v16f v = load_node_scalar(p.nodes, cur0);
                const float4 q0 = make_float4(v[0], v[1], v[2], v[3]), q1 = make_float4(v[4], v[5], v[6], v[7]);
                const float4 q2 = make_float4(v[8], v[9], v[10], v[11]);
                if (slab_divides_irregular(W::slab) && __float_as_int(v[14]) != 0) {   // irregular node (wave-uniform): the reference's own divisions
                    node_slabs<walk_divide<W>>(q0, q1, q2, r, mn0, mx0, mn1, mx1);
                    node_decide<kStats, false>(mn0, mx0, mn1, mx1, __float_as_int(v[12]), __float_as_int(v[13]), r, L, s_stack, st);
                    return;
                }
                float k0 = 0.0f, k1 = 0.0f;
                node_slabs_guarded<W>(q0, q1, q2, r, L.best_t, mn0, mx0, mn1, mx1, k0, k1);
                node_decide<kStats, kSafe, kGuarded>(mn0, mx0, mn1, mx1, __float_as_int(v[12]), __float_as_int(v[13]), r, L, s_stack, st, k0, k1);
                return;
            }
        }
    }
    // ---- inner node: test both children (BVH.cpp:593-624)
    MR_RUN_COUNT(st.node_steps);
    const float4 *nd = p.nodes + 4 * (size_t)L.cur;
    const float4 q0 = nd[0], q1 = nd[1], q2 = nd[2];
    const int4 q3 = *reinterpret_cast<const int4 *>(nd + 3);
    if (slab_divides_irregular(W::slab) && q3.z != 0) {
        node_slabs<walk_divide<W>>(q0, q1, q2, r, mn0, mx0, mn1, mx1);
        node_decide<kStats, false>(mn0, mx0, mn1, mx1, q3.x, q3.y, r, L, s_stack, st);
        return;
    }
    float k0 = 0.0f, k1 = 0.0f;
    node_slabs_guarded<W>(q0, q1, q2, r, L.best_t, mn0, mx0, mn1, mx1, k0, k1);
    node_decide<kStats, kSafe, kGuarded>(mn0, mx0, mn1, mx1, q3.x, q3.y, r, L, s_stack, st, k0, k1);
}

template <typename W>
__device__ __forceinline__ void node_slabs(const float4 q0, const float4 q1, const float4 q2, const RayRegs &r,
                                           float &mn0, float &mx0, float &mn1, float &mx1) {
    constexpr bool kQuot = W::slab == kSlabQuotient;
    if (is_octant(W::oct) && slab_has_octant_body(W::slab)) {
        slab_box_oct<W::oct, W::slab>(q0.x, q0.y, q0.z, q0.w, q2.x, q2.y, r, mn0, mx0);
        slab_box_oct<W::oct, W::slab>(q1.x, q1.y, q1.z, q1.w, q2.z, q2.w, r, mn1, mx1);
    } else if (W::slab == kSlabLean) {
        slab_box_lean(q0.x, q0.y, q0.z, q0.w, q2.x, q2.y, r, mn0, mx0);
        slab_box_lean(q1.x, q1.y, q1.z, q1.w, q2.z, q2.w, r, mn1, mx1);
    } else if (W::slab == kSlabCorrection) {
        slab_box_exactq(q0.x, q0.y, q0.z, q0.w, q2.x, q2.y, r, mn0, mx0);
        slab_box_exactq(q1.x, q1.y, q1.z, q1.w, q2.z, q2.w, r, mn1, mx1);
    } else if (W::exact && !slab_nan_free(W::slab)) {          // kSlabSelect, kSlabQuotient
        mn0 = -kInf; mx0 = kInf; mn1 = -kInf; mx1 = kInf;
        slab_axis<kQuot>(q0.x, q0.y, r.ox, r.dx, r.ix, mn0, mx0);
        slab_axis<kQuot>(q0.z, q0.w, r.oy, r.dy, r.iy, mn0, mx0);
        slab_axis<kQuot>(q2.x, q2.y, r.oz, r.dz, r.iz, mn0, mx0);
        slab_axis<kQuot>(q1.x, q1.y, r.ox, r.dx, r.ix, mn1, mx1);
        slab_axis<kQuot>(q1.z, q1.w, r.oy, r.dy, r.iy, mn1, mx1);
        slab_axis<kQuot>(q2.z, q2.w, r.oz, r.dz, r.iz, mn1, mx1);
    } else {
        slab_box_minmax(q0.x, q0.y, q0.z, q0.w, q2.x, q2.y, r, mn0, mx0);
        slab_box_minmax(q1.x, q1.y, q1.z, q1.w, q2.z, q2.w, r, mn1, mx1);
    }
}

// kSlabGuarded (5), "guarded products": the slab distances of a regular ray in a regular node as products (corner - o) * RN(1/d)
// -- 24 VALU fewer per two-child visit than the correction steps of kSlabCorrection (4) -- whenever the decisions taken from them are
// PROVABLY the ones the reference's quotients give, and the quotients themselves otherwise.
//   * q~ = RN(a * RN(1/d)) = (a/d)(1+e), |e| <= 2^-23 + 2^-48, against q = RN(a/d) = (a/d)(1+e'), |e'| <= 2^-24 (no
//     under- or overflow: lane_is_regular, regular nodes): q~ and q are less than 4 ulps apart, have the same sign, and
//     are zero together.  max3 / min3 / min with best_t are monotone, so each of mn0, mx0, mn1, mx1, min(mx, best_t)
//     computed from products is less than 4 ulps from the same expression on quotients.
//   * node_decide takes five comparisons from them: mn0 > min(mx0, best), mx0 < tmin, the same two for child 1, and
//     mn0 > mn1.  Two floats further than 8 ulps apart compare the same way after each moves by less than 4.  The ulp
//     distance of two floats of one sign is the difference of their bit patterns (v_sad_u32); patterns of opposite sign
//     are 2^31 apart, and there the comparison is decided by the signs, which are exact.
//   * so: if in every lane all five pairs are more than 16 patterns apart (margin of two), the product decisions stand;
//     if any lane has a closer pair the whole wave recomputes the node with exact quotients (kSlabCorrection) -- about one visit
//     in a few thousand.
// Same hits, same visiting order, same bits as kSlabCorrection (tests: test_gpu_parity, the fuzz campaigns run both).
template <typename W>
__device__ __forceinline__ void node_slabs_guarded(const float4 q0, const float4 q1, const float4 q2, const RayRegs &r, float best_t,
                                                   float &mn0, float &mx0, float &mn1, float &mx1, float &k0, float &k1) {
    if (!slab_guarded(W::slab)) {
        node_slabs<W>(q0, q1, q2, r, mn0, mx0, mn1, mx1);
        return;
    }
    node_slabs<walk_slab<W, kSlabMinMax>>(q0, q1, q2, r, mn0, mx0, mn1, mx1);
    // k = minNum(exit, best_t) of both children and the smallest of the pattern distances, in ONE asm block (separate
    // asm statements are fenced by hazard no-ops: three s_nop per visit when the two v_min stood alone)
    unsigned near, t0, t1;
    if (slab_needs_tmin0(W::slab)) {
        // tMin == 0 in every lane of the wave (camera, shadow and bounce rays: all of them): "exit < tMin" is a SIGN test,
        // and a product and its quotient have the same sign and are zero together -- that comparison needs no guard.
        // Three pairs are left: entry against min(exit, best) for each child, entry against entry.
        asm("v_min_f32 %3, %7, %9\n\tv_min_f32 %4, %8, %9\n\t"
            "v_sad_u32 %0, %5, %3, 0\n\tv_sad_u32 %1, %6, %4, 0\n\tv_sad_u32 %2, %5, %6, 0\n\tv_min3_u32 %0, %0, %1, %2"
            : "=&v"(near), "=&v"(t0), "=&v"(t1), "=&v"(k0), "=&v"(k1)
            : "v"(mn0), "v"(mn1), "v"(mx0), "v"(mx1), "v"(best_t));
    } else {
        asm("v_min_f32 %3, %8, %10\n\tv_min_f32 %4, %9, %10\n\t"
            "v_sad_u32 %0, %5, %3, 0\n\tv_sad_u32 %1, %8, %6, 0\n\tv_sad_u32 %2, %7, %4, 0\n\tv_min3_u32 %0, %0, %1, %2\n\t"
            "v_sad_u32 %1, %9, %6, 0\n\tv_sad_u32 %2, %5, %7, 0\n\tv_min3_u32 %0, %0, %1, %2"
            : "=&v"(near), "=&v"(t0), "=&v"(t1), "=&v"(k0), "=&v"(k1)
            : "v"(mn0), "v"(r.tmin), "v"(mn1), "v"(mx0), "v"(mx1), "v"(best_t));
    }
    // (run walks say that the recomputation is rare: it is laid out behind the loop and the visit's own path falls through)
    if (W::run ? __builtin_expect(__any(near <= 16u), 0) : __any(near <= 16u)) {
        node_slabs<walk_slab<W, kSlabCorrection>>(q0, q1, q2, r, mn0, mx0, mn1, mx1);
        k0 = vmin2(mx0, best_t); k1 = vmin2(mx1, best_t);
    }
}

// one 48-byte triangle record through the scalar data cache (all active lanes at the same leaf)
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void load_tri_scalar(const float4 *tris, unsigned pos_uniform, float4 &q0, float4 &q1, float4 &q2) {
    const float4 *ptr = tris + 3 * (size_t)pos_uniform;
    v4f a, b, c;
    asm volatile("s_load_dwordx4 %0, %3, 0x0\n\ts_load_dwordx4 %1, %3, 0x10\n\ts_load_dwordx4 %2, %3, 0x20\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b), "=&s"(c) : "s"(ptr) : "memory");
    q0 = make_float4(a[0], a[1], a[2], a[3]);
    q1 = make_float4(b[0], b[1], b[2], b[3]);
    q2 = make_float4(c[0], c[1], c[2], c[3]);
}
// the 40 bytes an eye-relative record uses (tri_test_rel), through the scalar cache
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void load_tri_rel_scalar(const float4 *tris, unsigned pos_uniform, float4 &q0, float4 &q1, float4 &q2) {
    const float4 *ptr = tris + 3 * (size_t)pos_uniform;
    v4f a, b;
    v2f c;
    asm volatile("s_load_dwordx4 %0, %3, 0x0\n\ts_load_dwordx4 %1, %3, 0x10\n\ts_load_dwordx2 %2, %3, 0x20\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b), "=&s"(c) : "s"(ptr) : "memory");
    q0 = make_float4(a[0], a[1], a[2], a[3]);
    q1 = make_float4(b[0], b[1], b[2], b[3]);
    q2 = make_float4(c[0], c[1], 0.0f, 0.0f);
}
template <bool REL>
__device__ __forceinline__ void load_tri_uniform(const float4 *tris, unsigned pos_uniform, float4 &q0, float4 &q1, float4 &q2) {
    if (REL) load_tri_rel_scalar(tris, pos_uniform, q0, q1, q2);
    else load_tri_scalar(tris, pos_uniform, q0, q1, q2);
}
// one record per lane (REL: its first 40 bytes)
template <bool REL>
__device__ __forceinline__ void load_tri(const float4 *tr, float4 &q0, float4 &q1, float4 &q2) {
    q0 = tr[0]; q1 = tr[1];
    if (REL) { const float2 c = *reinterpret_cast<const float2 *>(tr + 2); q2 = make_float4(c.x, c.y, 0.0f, 0.0f); }
    else q2 = tr[2];
}

template <typename W>
__device__ __forceinline__ void leaf_step(const TraceParams &p, const RayRegs &r, Lane &L, int *s_stack, int tid, Stats &st) {
    constexpr bool EXACT = W::exact, ANY = W::any, STATS = W::stats, SCALAR = W::scalar, OBJ = W::obj, REL = W::rel;
    // ---- leaf (BVH.cpp:493-509)
    const unsigned bits = ~(unsigned)L.cur;
    const unsigned first = bits >> kLeafCountBits;
    unsigned cnt = bits & kLeafCountMask;
    if (cnt == kLeafCountMask) cnt = p.leaf_cnt_ext[first];
    bool done = false;
    bool uniform = false;
    if (SCALAR) {
        const int cur0 = __builtin_amdgcn_readfirstlane(L.cur);
        uniform = __all(L.cur == cur0);
        if (uniform) {
            const unsigned first0 = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
            const unsigned cnt0 = (unsigned)__builtin_amdgcn_readfirstlane((int)cnt);
            for (unsigned k = 0; k < cnt0; k++) {
                float4 q0, q1, q2;
                load_tri_uniform<REL>(p.tris, first0 + k, q0, q1, q2);
                if (!(ANY && done)) {
                    float t, b, g;
                    const bool ok = uniform_object_test<W>(q0, q1, q2, r, L.best_t, t, b, g, st);
                    if (ok && t < L.best_t) {
                        L.best_t = t; L.best_b = b; L.best_g = g; L.best_pos = (int)(first0 + k);
                        if (ANY) done = true;
                    }
                }
            }
        }
    }
    if (!uniform) {
        for (unsigned k = 0; k < cnt; k++) {
            float4 q0, q1, q2;
            load_tri<REL>(p.tris + 3 * (size_t)(first + k), q0, q1, q2);
            float t, b, g;
            const bool ok = object_test<EXACT, OBJ, REL>(q0, q1, q2, r, L.best_t, t, b, g);
            if (ok && t < L.best_t) {             // strict-less replacement (:500)
                L.best_t = t; L.best_b = b; L.best_g = g; L.best_pos = (int)(first + k);
                if (ANY) { done = true; break; }
            }
        }
    }
    if (STATS) {
        if (OBJ) {   // Stats::Ray_Tri_Intersect counts Triangle objects only (the dynamic_cast of BVH.cpp:496)
            for (unsigned k = 0; k < cnt; k++)
                if (__float_as_uint(p.tris[3 * (size_t)(first + k) + 2].w) != kSphereTag) st.tri++;
        } else {
            st.tri += cnt;
        }
    }
    if (ANY && done) {
        L.cur = kDone;
    } else {
        L.cur = stack_pop(L, s_stack);
        if (STATS && L.cur != kDone) st.box++;
    }
}

// One triangle of the lane's current leaf (voting traversal): the leaf is decoded on its first step, popped after its
// last.  Same tests in the same order with the same running best_t as leaf_step.  When every participating lane is at
// the start of the same leaf, the whole leaf goes through the scalar cache in this one step (the coherent case).
template <typename W>
__device__ __forceinline__ void tri_step(const TraceParams &p, const RayRegs &r, Lane &L, int *s_stack, Stats &st) {
    constexpr bool EXACT = W::exact, ANY = W::any, STATS = W::stats, SCALAR = W::scalar, OBJ = W::obj, REL = W::rel;
    bool done = false;
    if (SCALAR) {
        const int cur0 = __builtin_amdgcn_readfirstlane(L.cur);
        if (__all(L.cur == cur0 && L.lpos == L.lend)) {
            const unsigned bits0 = ~(unsigned)cur0;
            const unsigned first0 = bits0 >> kLeafCountBits;
            unsigned cnt0 = bits0 & kLeafCountMask;
            if (cnt0 == kLeafCountMask) cnt0 = p.leaf_cnt_ext[first0];
            for (unsigned k = 0; k < cnt0; k++) {
                float4 q0, q1, q2;
                load_tri_uniform<REL>(p.tris, first0 + k, q0, q1, q2);
                if (!(ANY && done)) {
                    float t, b, g;
                    const bool ok = object_test<EXACT, OBJ, REL>(q0, q1, q2, r, L.best_t, t, b, g);
                    if (ok && t < L.best_t) {
                        L.best_t = t; L.best_b = b; L.best_g = g; L.best_pos = (int)(first0 + k);
                        if (ANY) done = true;
                    }
                }
            }
            if (STATS) {
                if (OBJ) { for (unsigned k = 0; k < cnt0; k++) if (__float_as_uint(p.tris[3 * (size_t)(first0 + k) + 2].w) != kSphereTag) st.tri++; }
                else st.tri += cnt0;
            }
            if (ANY && done) { L.cur = kDone; }
            else { L.cur = stack_pop(L, s_stack); if (STATS && L.cur != kDone) st.box++; }
            return;
        }
    }
    if (L.lpos == L.lend) {                          // first step in this leaf
        const unsigned bits = ~(unsigned)L.cur;
        const unsigned first = bits >> kLeafCountBits;
        unsigned cnt = bits & kLeafCountMask;
        if (cnt == kLeafCountMask) cnt = p.leaf_cnt_ext[first];
        L.lpos = (int)first; L.lend = (int)(first + cnt);
        if (STATS) {
            if (OBJ) { for (unsigned k = 0; k < cnt; k++) if (__float_as_uint(p.tris[3 * (size_t)(first + k) + 2].w) != kSphereTag) st.tri++; }
            else st.tri += cnt;
        }
    }
    if (L.lpos < L.lend) {
        float4 q0, q1, q2;
        load_tri<REL>(p.tris + 3 * (size_t)L.lpos, q0, q1, q2);
        float t, b, g;
        const bool ok = object_test<EXACT, OBJ, REL>(q0, q1, q2, r, L.best_t, t, b, g);
        if (ok && t < L.best_t) {                    // strict-less replacement (BVH.cpp:500)
            L.best_t = t; L.best_b = b; L.best_g = g; L.best_pos = L.lpos;
            if (ANY) done = true;
        }
        L.lpos++;
    }
    if (ANY && done) {
        L.cur = kDone; L.lpos = L.lend;
    } else if (L.lpos == L.lend) {                   // leaf finished (or empty): on to the next pending node
        L.cur = stack_pop(L, s_stack);
        if (STATS && L.cur != kDone) st.box++;
    }
}

// the walk W in its control flow (kFlowLane / kFlowWhileWhile / kFlowVote)
template <typename W>
__device__ __forceinline__ void traverse(const TraceParams &p, const RayRegs &r, Lane &L, int *s_stack, int tid, Stats &st) {
    if (W::flow == kFlowVote) {
        using Node = walk_run<W, false>;                       // the voting flow takes no uniform run
        L.lpos = 0; L.lend = 0;
        while (true) {
            const bool want_node = L.cur >= 0, want_tri = L.cur < 0 && L.cur != kDone;
            const unsigned long long m_node = __ballot(want_node), m_tri = __ballot(want_tri);
            if ((m_node | m_tri) == 0ull) break;
            if (__popcll(m_node) >= __popcll(m_tri)) {
                if (want_node) node_step<Node>(p, r, L, s_stack, tid, st);
            } else {
                if (want_tri) tri_step<W>(p, r, L, s_stack, st);
            }
        }
    } else if (W::flow == kFlowWhileWhile && walk_runs<W>()) {
        // the lanes with work, handed down: a run that holds them all is a whole walk (uniform_run)
        unsigned long long m_have;
        while ((m_have = __builtin_amdgcn_ballot_w64(L.have())) != 0ull) {
            while (L.cur >= 0) node_step<W>(p, r, L, s_stack, tid, st, m_have);
            if (L.have()) leaf_step<W>(p, r, L, s_stack, tid, st);
        }
    } else if (W::flow == kFlowWhileWhile) {
        while (__any(L.have())) {
            while (L.cur >= 0) node_step<W>(p, r, L, s_stack, tid, st);
            if (L.have()) leaf_step<W>(p, r, L, s_stack, tid, st);
        }
    } else {
        // the per-lane flow has neither octant bodies nor the uniform run, and loads its leaves per lane
        using Node = walk_run<walk_oct<W, kNoOct>, false>;
        using Leaf = walk_scalar<W, false>;
        while (L.have()) {
            if (L.cur >= 0) node_step<Node>(p, r, L, s_stack, tid, st);
            else leaf_step<Leaf>(p, r, L, s_stack, tid, st);
        }
    }
}

// What trace_ray does with a variant (the kVar... bits of mr_launch.h): the slab form and control flow of each of its four paths,
// kNoPath where the variant has none.
//   oct       a good wave whose live rays share an octant (kVarOctant)
//   good      a good wave without one: NaN-free rays for the product variants (kVarMinMax), regular rays for the quotients (kVarStrict)
//   fallback  any other wave of such a variant: the reference's own arithmetic
//   plain     variants that do not sort their waves: counting runs (STATS) and those with neither bit
struct PathPlan { int slab, flow; };
struct TracePlan {
    PathPlan oct, good, fallback, plain;
    bool strict, scalar, obj;      // the root test, the fallback and the plain path divide; kVarScalar; kVarObjects
};
constexpr PathPlan kNoPath = {-1, -1};
constexpr bool operator==(PathPlan a, PathPlan b) { return a.slab == b.slab && a.flow == b.flow; }
constexpr bool operator==(TracePlan a, TracePlan b) {
    return a.oct == b.oct && a.good == b.good && a.fallback == b.fallback && a.plain == b.plain && a.strict == b.strict && a.scalar == b.scalar && a.obj == b.obj;
}
constexpr bool has_path(PathPlan a) { return !(a == kNoPath); }
constexpr TracePlan trace_plan(int var, bool stats) {
    const bool strict = stats || (var & kVarStrict), minmax = !strict && (var & kVarMinMax), sorts = minmax || (strict && !stats);
    const int flow = (var & kVarVote) ? kFlowVote : ((var & kVarWhileWhile) ? kFlowWhileWhile : kFlowLane);
    const int safe = (var & kVarLeanFma) ? kSlabLean : kSlabMinMax;            // for waves whose rays cannot produce a NaN
    const int exact = (var & kVarGuarded) ? kSlabGuarded : kSlabCorrection;    // guarded products instead of the correction steps
    const int good = minmax ? safe : exact;
    TracePlan P = {kNoPath, kNoPath, kNoPath, kNoPath, strict, (var & kVarScalar) != 0, (var & kVarObjects) != 0};
    if (!sorts) { P.plain = {strict ? kSlabQuotient : kSlabSelect, flow}; return P; }
    // the octant loops' guard assumes tMin == 0 (node_slabs_guarded)
    if (var & kVarOctant) P.oct = {good == kSlabGuarded ? kSlabGuardedT0 : good, flow};
    // A wave of regular rays that point into several octants is an incoherent one: bound by its record fetches, it gains nothing
    // from the guarded products and would pay for their wave-wide branch -- the correction steps alone there.
    // kVarMixedVote: ... and the voting control flow suits it better (random rays 3.86 -> 4.09 Grays/s, the atrium's bounce
    // rays 4.96 -> 5.31, 1-spp shadow rays in image order 3.73 -> 4.31 without the caller's MR_TRACE_INCOHERENT hint)
    if (minmax) P.good = {safe, flow};
    else P.good = {kSlabCorrection, ((var & kVarMixedVote) && flow == kFlowWhileWhile) ? kFlowVote : flow};
    P.fallback = {minmax ? kSlabSelect : kSlabQuotient, flow};
    return P;
}
// every variant mr_launch.h names, as launched (STATS: MR_COUNT_STATS)                  oct                                 good                                fallback                          plain                      strict scalar obj
static_assert(trace_plan(kTraceExact, false) ==           TracePlan{{kSlabGuardedT0, kFlowWhileWhile},  {kSlabCorrection, kFlowVote},       {kSlabQuotient, kFlowWhileWhile}, kNoPath,                     true,  true,  false});
static_assert(trace_plan(kTraceEyeRel, false) ==          TracePlan{{kSlabGuardedT0, kFlowWhileWhile},  {kSlabCorrection, kFlowWhileWhile}, {kSlabQuotient, kFlowWhileWhile}, kNoPath,                     true,  true,  false});
static_assert(trace_plan(kTraceExactObj, false) ==        TracePlan{{kSlabGuardedT0, kFlowWhileWhile},  {kSlabCorrection, kFlowWhileWhile}, {kSlabQuotient, kFlowWhileWhile}, kNoPath,                     true,  true,  true});
static_assert(trace_plan(kTraceCorrection, false) ==      TracePlan{{kSlabCorrection, kFlowWhileWhile}, {kSlabCorrection, kFlowWhileWhile}, {kSlabQuotient, kFlowWhileWhile}, kNoPath,                     true,  true,  false});
static_assert(trace_plan(kTraceProduct, false) ==         TracePlan{{kSlabMinMax, kFlowWhileWhile},     {kSlabMinMax, kFlowWhileWhile},     {kSlabSelect, kFlowWhileWhile},   kNoPath,                     false, true,  false});
static_assert(trace_plan(kTraceProductObj, false) ==      TracePlan{kNoPath,                            {kSlabMinMax, kFlowWhileWhile},     {kSlabSelect, kFlowWhileWhile},   kNoPath,                     false, true,  true});
static_assert(trace_plan(kTraceDevProduct, false) ==      TracePlan{kNoPath,                            {kSlabMinMax, kFlowWhileWhile},     {kSlabSelect, kFlowWhileWhile},   kNoPath,                     false, true,  false});
static_assert(trace_plan(kTraceFast, false) ==            TracePlan{kNoPath,                            {kSlabLean, kFlowWhileWhile},       {kSlabSelect, kFlowWhileWhile},   kNoPath,                     false, true,  false});
static_assert(trace_plan(kTraceVote, false) ==            TracePlan{kNoPath,                            {kSlabCorrection, kFlowVote},       {kSlabQuotient, kFlowVote},       kNoPath,                     true,  true,  false});
static_assert(trace_plan(kTraceVoteObj, false) ==         TracePlan{kNoPath,                            {kSlabCorrection, kFlowVote},       {kSlabQuotient, kFlowVote},       kNoPath,                     true,  true,  true});
static_assert(trace_plan(kTraceVoteProduct, false) ==     TracePlan{kNoPath,                            {kSlabMinMax, kFlowVote},           {kSlabSelect, kFlowVote},         kNoPath,                     false, true,  false});
static_assert(trace_plan(kTraceVoteProductObj, false) ==  TracePlan{kNoPath,                            {kSlabMinMax, kFlowVote},           {kSlabSelect, kFlowVote},         kNoPath,                     false, true,  true});
static_assert(trace_plan(kTracePlain, false) ==           TracePlan{kNoPath,                            kNoPath,                            kNoPath,                          {kSlabSelect, kFlowLane},    false, false, false});
static_assert(trace_plan(kTracePlainObj, false) ==        TracePlan{kNoPath,                            kNoPath,                            kNoPath,                          {kSlabSelect, kFlowLane},    false, false, true});
static_assert(trace_plan(kTracePlain, true) ==            TracePlan{kNoPath,                            kNoPath,                            kNoPath,                          {kSlabQuotient, kFlowLane},  true,  false, false});
static_assert(trace_plan(kTracePlainObj, true) ==         TracePlan{kNoPath,                            kNoPath,                            kNoPath,                          {kSlabQuotient, kFlowLane},  true,  false, true});

// ---------------------------------------------------------------------------------------------------
// One ray per lane from the root test to the unbounded-object scan: Scene::trace (Scene.cpp:214-230) ->
// BVH::intersect (BVH.cpp:438-469) -> intersectChildren.  `live` = the lane holds a ray; the call is made by whole
// waves (the while-while loop votes with __any).  Result in L (best_t / best_pos / beta / gamma) and plane_hit.
// VAR: the kVar... bits of mr_launch.h, which also names the combinations the launchers use.
// REL: p holds the eye-relative tables of the fused frame (mr_frame.hip: eye_tables) -- node corners and root box minus the
//     eye, triangle records of tri_test_rel -- and every ray starts at the eye: the origin is taken as the constant 0, so the
//     slab distances (corner - o) / d become (corner - eye) / d on the stored differences with no subtraction left, the
//     same operands and the same bits as on the scene's own tables.  The eye's own regularity (lane_is_regular sees 0 here)
//     travels in the node flags: an irregular eye marks every node irregular, so every visit divides (kSlabQuotient) as the
//     scene's tables would have had it do.  Default traversal of triangle-only scenes only.
// ---------------------------------------------------------------------------------------------------
template <bool EXACT, bool ANY, bool STATS, int VAR, bool REL = false, bool RUN = false>
__device__ __forceinline__ void trace_ray(const TraceParams &p, const RayRegs &r_in, float tmax0, bool live, Lane &L,
                                          int &plane_hit, int *s_stack, int tid, Stats &st) {
    static_assert(!REL || ((VAR & kVarStrict) && !(VAR & kVarObjects) && !STATS), "eye-relative tables: default traversal, triangles only");
    RayRegs r = r_in;
    if (REL) { r.ox = 0.0f; r.oy = 0.0f; r.oz = 0.0f; }
    constexpr TracePlan P = trace_plan(VAR, STATS);
    // what the walks of all four paths share; each path adds its slab form and control flow
    using Base = Walk<EXACT, ANY, STATS, kSlabSelect, kFlowLane, P.scalar, P.obj, kNoOct, REL, false>;
    // the fallback and the plain path take the scalar loads only where they divide: on kSlabSelect (the NaN-unsafe wave of a
    // kVarMinMax variant, the plain path without kVarStrict) every node and leaf is loaded per lane
    using Other = walk_scalar<Base, P.scalar && P.strict>;

    L.best_t = tmax0;                             // minHit.t = tMax (BVH.cpp:444)
    L.best_b = 0.0f; L.best_g = 0.0f;
    L.best_pos = -1;                              // leaf-order position of the winning triangle
    stack_reset(L, s_stack, tid);                 // this lane's LDS stack: the kDone sentinel only
    {   // BVH::intersect root test (BVH.cpp:447-466)
        float mn = -kInf, mx = kInf;
        slab_axis<P.strict>(p.root_lo[0], p.root_hi[0], r.ox, r.dx, r.ix, mn, mx);
        slab_axis<P.strict>(p.root_lo[1], p.root_hi[1], r.oy, r.dy, r.iy, mn, mx);
        slab_axis<P.strict>(p.root_lo[2], p.root_hi[2], r.oz, r.dz, r.iz, mn, mx);
        if (STATS && live) st.box++;
        L.cur = (live && !((mn > mx) || (mn > tmax0) || (mx < r.tmin))) ? p.root_ref : kDone;
    }

    // a good wave: NaN-free rays for the product forms (a slab product (corner - o) * (1/d) can only be NaN as 0*inf or inf*0 or from a
    // non-finite origin: with o, d and 1/d all finite in every lane the select form and the min/max form decide identically), regular
    // rays for the default trace (the quotients' decisions from guarded products or from the correction steps -- then the lanes'
    // quotients are NaN-free too and the min/max form decides like the select form)
    const bool good_wave = !has_path(P.good) ? false : (P.strict ? __all(lane_is_regular(r) || !live) : __all(lane_is_nan_free(r) || !live));
    // kVarOctant: when the wave's live rays all point into one octant the slab tests take their near / far corners by
    // position (slab_box_oct): eight copies of the loop, chosen once per ray batch of the wave
    bool done_oct = false;
    if constexpr (has_path(P.oct)) {
        if (good_wave) {
            const unsigned long long m_live = __ballot(live);
            if (m_live) {
                const int oct = octant_of(r);
                const int oct0 = __builtin_amdgcn_readlane(oct, __ffsll((long long)m_live) - 1);
                if (__all(!live || oct == oct0) && (!slab_needs_tmin0(P.oct.slab) || __all(!live || r.tmin == 0.0f))) {
                    done_oct = true;
                    using Oct = walk_run<walk_slab<Base, P.oct.slab, P.oct.flow>, RUN>;
#define MR_OCT_CASE(LABEL, O) LABEL: traverse<walk_oct<Oct, O>>(p, r, L, s_stack, tid, st); break;
                    switch (oct0) {
                        MR_OCT_CASE(case 0, 0) MR_OCT_CASE(case 1, 1) MR_OCT_CASE(case 2, 2) MR_OCT_CASE(case 3, 3)
                        MR_OCT_CASE(case 4, 4) MR_OCT_CASE(case 5, 5) MR_OCT_CASE(case 6, 6) MR_OCT_CASE(default, 7)
                    }
#undef MR_OCT_CASE
                }
            }
        }
    }
    if (done_oct) {
    } else if constexpr (has_path(P.good)) {
        if (good_wave) traverse<walk_slab<Base, P.good.slab, P.good.flow>>(p, r, L, s_stack, tid, st);
        else traverse<walk_slab<Other, P.fallback.slab, P.fallback.flow>>(p, r, L, s_stack, tid, st);
    } else {
        traverse<walk_slab<Other, P.plain.slab, P.plain.flow>>(p, r, L, s_stack, tid, st);
    }

    // Scene::trace's scan of the unbounded objects (Scene.cpp:220-230): every plane is tested against the
    // caller's tMin / tMax (Plane.cpp:33-48) and kept when nothing was hit yet or it is strictly nearer
    plane_hit = -1;
    if (P.obj && live && !(ANY && L.best_pos >= 0)) {
        for (uint32_t k = 0; k < p.n_planes; k++) {
            const float4 pn = p.planes[2 * k], po = p.planes[2 * k + 1];
            const float ndotd = (pn.x * r.dx + pn.y * r.dy) + pn.z * r.dz;
            if ((double)__builtin_fabsf(ndotd) < 1e-6) continue;          // fabs(float) < double literal
            const float t = ((pn.x * (po.x - r.ox) + pn.y * (po.y - r.oy)) + pn.z * (po.z - r.oz)) / ndotd;
            if (t < r.tmin || t > tmax0) continue;
            if ((L.best_pos < 0 && plane_hit < 0) || t < L.best_t) { L.best_t = t; plane_hit = (int)k; }
        }
    }
}

// the mr_hit record of a finished lane (HitInfo in its device form, miro_hip.h)
template <bool OBJ>
__device__ __forceinline__ mr_hit make_hit(const TraceParams &p, const Lane &L, int plane_hit, float tmax0) {
    mr_hit h;
    if (OBJ && plane_hit >= 0) {
        h.t = L.best_t; h.prim = kPlaneBit | (uint32_t)plane_hit; h.beta = 0.0f; h.gamma = 0.0f;
    } else if (L.best_pos >= 0) {
        h.t = L.best_t; h.prim = p.tri_prim[L.best_pos]; h.beta = L.best_b; h.gamma = L.best_g;
    } else {
        h.t = tmax0; h.prim = MR_MISS; h.beta = 0.0f; h.gamma = 0.0f;
    }
    return h;
}

// "Trace one ray held in registers (ra = origin | tMin, rb = direction | -) and give me its hit record": trace_ray and
// make_hit on a fresh RayRegs / Lane.  Called by whole waves like trace_ray; a lane that is not live gets the miss record.
template <bool EXACT, bool ANY, bool STATS, int VAR, bool REL = false>
__device__ __forceinline__ mr_hit trace_hit(const TraceParams &p, const float4 &ra, const float4 &rb, float tmax, bool live,
                                            int *s_stack, int tid, Stats &st) {
    RayRegs r;
    ray_setup(r, ra, rb);
    Lane L;
    int plane_hit;
    trace_ray<EXACT, ANY, STATS, VAR, REL>(p, r, tmax, live, L, plane_hit, s_stack, tid, st);
    return make_hit<(VAR & kVarObjects) != 0>(p, L, plane_hit, tmax);
}

// n rounded up to whole workgroups: the loop bound of kernels whose iterations hold a barrier (workgroup_reserve)
__device__ __forceinline__ unsigned long long whole_workgroups(unsigned long long n) {
    return (n + (unsigned long long)kTraceBlock - 1ull) / kTraceBlock * kTraceBlock;
}

// counters[j] += the workgroup's sum of mine[j]: a wave shuffle-reduce, one LDS slot per wave, then ONE atomic per word
// and workgroup, and none for a sum of zero (a single counter word drains ~88 atomics per microsecond: a 1-spp frame's
// 8 100 workgroups are already a measurable 4 % with two words each).  Called once, by all threads of the workgroup.
template <int BLOCK, int WORDS>
__device__ __forceinline__ void workgroup_add(const unsigned (&mine)[WORDS], unsigned long long *counters) {
    __shared__ unsigned s_part[WORDS][BLOCK / 64];
    const int tid = threadIdx.x;
    unsigned w[WORDS];
    for (int j = 0; j < WORDS; j++) w[j] = mine[j];
    for (int off = 32; off > 0; off >>= 1)
        for (int j = 0; j < WORDS; j++) w[j] += __shfl_down(w[j], off, 64);
    if ((tid & 63) == 0)
        for (int j = 0; j < WORDS; j++) s_part[j][tid >> 6] = w[j];
    __syncthreads();
    if (tid < WORDS) {
        unsigned long long tot = 0;
        for (int k = 0; k < BLOCK / 64; k++) tot += s_part[tid][k];
        if (tot) atomicAdd(&counters[tid], tot);
    }
}
template <int BLOCK>
__device__ __forceinline__ void workgroup_add(unsigned mine, unsigned long long *counter) {
    const unsigned m[1] = {mine};
    workgroup_add<BLOCK, 1>(m, counter);
}

}  // namespace
}  // namespace mr
