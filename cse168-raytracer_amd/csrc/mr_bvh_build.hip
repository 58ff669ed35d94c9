// mr_bvh_build.hip -- BVH::build (BVH.cpp:60-339) on the device: the tree of mr_build.cpp, bit for bit, built level by level
// (MR_BUILD_REFERENCE_DEVICE).  The yardstick is the host builder; the arithmetic that decides the tree is mr_bvh_rules.h's,
// shared with it.
//
// Why the reference's bisection can run in parallel: its two sides are scratch arrays reordered by swap-remove, with a frozen
// prefix and boxes that grow object by object, but every quantity a step computes is a count, a min / max or an OR over a set,
// and the set is a function of one side flag per object and the plane:
//   moved set      objects of the heavy side whose centre the new plane has passed (strictly; bvh::moves).  The frozen prefix
//                  never holds such an object: every object of the left side has centre <= plane and every object of the right
//                  side centre >= plane, and when a side is the light one the bisection interval closes on that plane
//   light box      grows by the min / max over the moved set
//   boundary_left  OR over the moved set of bvh::leaves_boundary against the heavy box as it was before the step
//   heavy box      unchanged, or -- boundary_left -- min / max over what remains on the heavy side
// The side flag is state, not a function of the plane: a centre equal to a plane stays where it is (the predicates are strict),
// and only the final partition, by centre < best plane, sends it right.  fminf / fmaxf against the reference's compare-and-assign
// can differ in the sign of a zero corner, which no stored value sees (mr_bvh_rules.h).
//
// Kernels:
//   bvh_objects_kernel  lo / hi / centre of every object from the raw mesh arrays, the identity permutation, the non-finite flag
//   bvh_level_kernel    per depth, one workgroup per node of that depth -- four waves for a node of more than 256 objects, one wave
//                       (no LDS, no barrier in its reductions) for a smaller one, each kind in a launch of its own over its list
//                       of nodes: bounds if the parent handed down the cleared box, padding, leaf test; an inner node runs the
//                       three axes (classification, 32 steps, 33 costs), keeps the first strict minimum, stable-partitions its
//                       segment -- the permutation and, with it, the rows of the object table, so that every pass reads its
//                       segment front to back -- into the other table, appends its two children (adjacent records) to the node
//                       array and puts each on the next depth's list of its size; a leaf copies its segment of the
//                       permutation to its place in leaf_prims.  Segments nest and a left child's precedes its right
//                       sibling's, so the leaves' segments together are leaf_prims in depth-first order.
//   bvh_sizes_kernel / bvh_preorder_kernel / bvh_emit_kernel   subtree sizes deepest depth first, pre-order indices from the
//                       root down (child0 = parent + 1, child1 = parent + 1 + size(child0)), then the HostNode records in
//                       pre-order, which the host downloads as they are.
// No workgroup waits on another: the launch boundary separates depths, the host reads the node count back after each launch
// (at most 33 times) and sizes the next from it.  Every loop is bounded by 3 axes, 33 costs or a segment length.
#include <algorithm>
#include <vector>

#include "mr_internal.h"
#include "mr_bvh_rules.h"

namespace mr {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kSmallNode = 256;     // a node of at most this many objects is built by one wave, a larger one by four
constexpr float kInf = __builtin_inff();

// nodes in the order they were appended: the root, then each depth's nodes behind the one before; siblings adjacent
struct BuildNode {
    float lo[3], hi[3];      // the box the parent handed down (cleared: none) until the node's own workgroup stores the padded corners
    uint32_t first, count;   // the node's segment of the object table
    int32_t child;           // the left child's index (the right one follows it); -1: leaf
    int32_t depth;
};
static_assert(sizeof(HostNode) == 40, "bvh_emit_kernel writes HostNode records");

enum { kCtrNodes = 0, kCtrLeaves = 1, kCtrOverflow = 2, kCtrNonFinite = 3, kCtrBig = 4, kCtrSmall = 5, kCounters = 6 };

// The object table in the order of the permutation: position i holds object perm[i] with its box and centre.  A partition moves
// the rows with the permutation, into the other table, so that every pass of a node reads its segment front to back.
struct ObjTable {
    uint32_t *perm;
    float4 *lo, *hi;             // (lo.xyz, -), (hi.xyz, -)
    float *ctr;                  // centres, one plane of n per axis
};

struct BuildArrays {
    ObjTable in, out;            // this depth's segments, the next depth's
    uint32_t n, leaf_size;
    BuildNode *nodes;
    uint32_t node_capacity;
    uint32_t *leaf_out;          // leaf_prims
    uint8_t *side;               // the side flag of every position of a segment, for the axis its node is at
    uint32_t *counters;
    const uint32_t *list;        // the nodes of this launch: the large or the small nodes of one depth
    uint32_t *next_big, *next_small, list_capacity;      // the same two lists of the next depth (counters kCtrBig / kCtrSmall)
};

__global__ __launch_bounds__(kBlock) void bvh_objects_kernel(const float *v, const uint32_t *vi, const float *spheres, uint32_t n_spheres,
                                                             uint32_t n, ObjTable table, uint32_t *counters) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float lo[3], hi[3], c[3];
    bool finite = true;
    const uint32_t i0 = vi[3 * (size_t)i];
    if (n_spheres && i0 == kSphereSlot) {       // HostMesh::is_sphere
        const float *sp = spheres + 4 * (size_t)vi[3 * (size_t)i + 1];
        for (int k = 0; k < 4; k++) finite = finite && __builtin_isfinite(sp[k]);
        bvh::sphere_ref(sp, lo, hi, c);
    } else {
        const float *a = v + 3 * (size_t)i0, *b = v + 3 * (size_t)vi[3 * (size_t)i + 1], *cc = v + 3 * (size_t)vi[3 * (size_t)i + 2];
        for (int k = 0; k < 3; k++) finite = finite && __builtin_isfinite(a[k]) && __builtin_isfinite(b[k]) && __builtin_isfinite(cc[k]);
        bvh::triangle_ref(a, b, cc, lo, hi, c);
    }
    for (int k = 0; k < 3; k++) finite = finite && __builtin_isfinite(lo[k]) && __builtin_isfinite(hi[k]) && __builtin_isfinite(c[k]);
    table.lo[i] = make_float4(lo[0], lo[1], lo[2], 0.f);
    table.hi[i] = make_float4(hi[0], hi[1], hi[2], 0.f);
    for (int k = 0; k < 3; k++) table.ctr[(size_t)k * n + i] = c[k];
    table.perm[i] = i;
    if (!finite) atomicOr(&counters[kCtrNonFinite], 1u);
}

// min of mn[0 .. NMIN), max of mx[0 .. NMAX) and sum of sm[0 .. NSUM) over the workgroup of WAVES waves, the results in every
// lane.  min and max are exact in any order (up to the sign of a zero), the sums are integers.
template <int WAVES, int NMIN, int NMAX, int NSUM>
__device__ __forceinline__ void block_reduce(float *mn, float *mx, uint32_t *sm, uint32_t (*lds)[16]) {
    static_assert(NMIN + NMAX + NSUM <= 16, "one LDS row per wave");
#pragma unroll
    for (int m = 32; m; m >>= 1) {
#pragma unroll
        for (int k = 0; k < NMIN; k++) mn[k] = fminf(mn[k], __shfl_xor(mn[k], m, 64));
#pragma unroll
        for (int k = 0; k < NMAX; k++) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], m, 64));
#pragma unroll
        for (int k = 0; k < NSUM; k++) sm[k] += __shfl_xor(sm[k], m, 64);
    }
    if (WAVES == 1) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                 // the row's readers of the reduction before are done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NMIN; k++) lds[wave][k] = __float_as_uint(mn[k]);
#pragma unroll
        for (int k = 0; k < NMAX; k++) lds[wave][NMIN + k] = __float_as_uint(mx[k]);
#pragma unroll
        for (int k = 0; k < NSUM; k++) lds[wave][NMIN + NMAX + k] = sm[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NMIN; k++) {
        float r = __uint_as_float(lds[0][k]);
#pragma unroll
        for (int w = 1; w < WAVES; w++) r = fminf(r, __uint_as_float(lds[w][k]));
        mn[k] = r;
    }
#pragma unroll
    for (int k = 0; k < NMAX; k++) {
        float r = __uint_as_float(lds[0][NMIN + k]);
#pragma unroll
        for (int w = 1; w < WAVES; w++) r = fmaxf(r, __uint_as_float(lds[w][NMIN + k]));
        mx[k] = r;
    }
#pragma unroll
    for (int k = 0; k < NSUM; k++) {
        uint32_t r = lds[0][NMIN + NMAX + k];
#pragma unroll
        for (int w = 1; w < WAVES; w++) r += lds[w][NMIN + NMAX + k];
        sm[k] = r;
    }
}

__device__ __forceinline__ float pick3(const float *a, int k) { return k == 0 ? a[0] : (k == 1 ? a[1] : a[2]); }   // no indexed registers
__device__ __forceinline__ void grow3(float *mn, float *mx, const float4 &l, const float4 &h) {
    mn[0] = fminf(mn[0], l.x); mn[1] = fminf(mn[1], l.y); mn[2] = fminf(mn[2], l.z);
    mx[0] = fmaxf(mx[0], h.x); mx[1] = fmaxf(mx[1], h.y); mx[2] = fmaxf(mx[2], h.z);
}

// The passes over a segment take kBatch positions per lane and trip and issue their loads before they look at any: a lane that
// waited for one position's flag before it asked for its centre would spend the pass waiting.  A position past the end reads
// the segment's last row (count > 0) and is ignored.
constexpr int kBatch = 4;

// min / max of the boxes at the positions of a segment (lo, hi: its first row) whose side flag is `want` (want < 0: of all), in
// every lane
template <int WAVES>
__device__ __forceinline__ bvh::Box block_bounds(const float4 *lo, const float4 *hi, const uint8_t *side, int want, uint32_t count,
                                                 uint32_t (*lds)[16]) {
    constexpr uint32_t kLanes = 64 * WAVES;
    float mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
    for (uint32_t base = threadIdx.x; base < count; base += kBatch * kLanes) {
        float4 l[kBatch], h[kBatch];
        bool take[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
            const uint32_t i = base + u * kLanes, at = i < count ? i : count - 1;
            l[u] = lo[at]; h[u] = hi[at];
            take[u] = i < count && (want < 0 || side[at] == (uint8_t)want);
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++)
            if (take[u]) grow3(mn, mx, l[u], h[u]);
    }
    block_reduce<WAVES, 3, 3, 0>(mn, mx, nullptr, lds);
    bvh::Box b;
    for (int k = 0; k < 3; k++) { b.lo[k] = mn[k]; b.hi[k] = mx[k]; }
    return b;
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void bvh_level_kernel(BuildArrays p) {
    constexpr uint32_t kLanes = 64 * WAVES;
    __shared__ uint32_t lds[WAVES][16];
    const uint32_t t = threadIdx.x;
    BuildNode &nd = p.nodes[p.list[blockIdx.x]];
    const uint32_t first = nd.first, count = nd.count;
    const int depth = nd.depth;
    bvh::Box given;
    for (int k = 0; k < 3; k++) { given.lo[k] = nd.lo[k]; given.hi[k] = nd.hi[k]; }
    const uint32_t *perm = p.in.perm + first;
    const float4 *olo = p.in.lo + first, *ohi = p.in.hi + first;
    if (given.cleared() && count) given = block_bounds<WAVES>(olo, ohi, nullptr, -1, count, lds);
    given.pad();
    const bool leaf = count <= p.leaf_size || depth >= bvh::kMaxDepth;
    __syncthreads();                 // every lane has read the box handed down before lane 0 replaces it
    if (t == 0) {
        for (int k = 0; k < 3; k++) { nd.lo[k] = given.lo[k]; nd.hi[k] = given.hi[k]; }
        if (leaf) {
            nd.child = -1;
            atomicAdd(&p.counters[kCtrLeaves], 1u);
        }
    }
    if (leaf) {                      // its segment is final
        for (uint32_t i = t; i < count; i += kLanes) p.leaf_out[first + i] = perm[i];
        return;
    }

    float best_cost = kInf, best_plane = 0.0f;
    int best_axis = 0;
    bvh::Box best0, best1;
    best0.set_default_corners();
    best1.set_default_corners();
    uint8_t *side = p.side + first;  // lane t reads and writes positions t, t + kLanes, ... only
    for (int axis = 0; axis < 3; axis++) {
        const float *ctr = p.in.ctr + (size_t)axis * p.n + first;
        float lo = pick3(given.lo, axis), hi = pick3(given.hi, axis), plane = bvh::mid_plane(lo, hi);
        bvh::Box box0, box1;
        uint32_t cnt0, cnt1;
        {
            float mn[6] = {kInf, kInf, kInf, kInf, kInf, kInf}, mx[6] = {-kInf, -kInf, -kInf, -kInf, -kInf, -kInf};
            uint32_t sm[2] = {0u, 0u};
            for (uint32_t base = t; base < count; base += kBatch * kLanes) {
                float c[kBatch];
                float4 l[kBatch], h[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    const uint32_t i = base + u * kLanes, at = i < count ? i : count - 1;
                    c[u] = ctr[at]; l[u] = olo[at]; h[u] = ohi[at];
                }
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    const uint32_t i = base + u * kLanes;
                    if (i >= count) continue;
                    const int s = bvh::side_of(c[u], plane);
                    side[i] = (uint8_t)s;
                    if (s == 0) { grow3(mn, mx, l[u], h[u]); sm[0]++; }
                    else { grow3(mn + 3, mx + 3, l[u], h[u]); sm[1]++; }
                }
            }
            block_reduce<WAVES, 6, 6, 2>(mn, mx, sm, lds);
            for (int k = 0; k < 3; k++) { box0.lo[k] = mn[k]; box0.hi[k] = mx[k]; box1.lo[k] = mn[3 + k]; box1.hi[k] = mx[3 + k]; }
            cnt0 = sm[0]; cnt1 = sm[1];
        }
        for (int step = 0; step <= bvh::kBisectSteps; step++) {
            const float c0 = bvh::side_cost(box0, (int)cnt0), c1 = bvh::side_cost(box1, (int)cnt1);
            if (c0 + c1 < best_cost) {
                best_cost = c0 + c1; best_axis = axis; best_plane = plane;
                best0 = box0; best1 = box1;
            }
            if (step == bvh::kBisectSteps) break;            // the closing cost
            const int heavy = bvh::heavier_side(c0, c1);
            if (heavy == 0) hi = plane; else lo = plane;
            plane = bvh::mid_plane(lo, hi);
            bvh::Box hb = box1, lb = box0;                    // heavy and light box
            if (heavy == 0) { hb = box0; lb = box1; }
            float mn[3] = {kInf, kInf, kInf}, mx[3] = {-kInf, -kInf, -kInf};
            uint32_t sm[2] = {0u, 0u};                        // objects moved; of them, objects that touched the heavy box
            for (uint32_t base = t; base < count; base += kBatch * kLanes) {
                float c[kBatch];
                uint8_t sd[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    const uint32_t i = base + u * kLanes, at = i < count ? i : count - 1;
                    sd[u] = side[at]; c[u] = ctr[at];
                }
#pragma unroll
                for (int u = 0; u < kBatch; u++) {
                    const uint32_t i = base + u * kLanes;
                    if (i >= count || sd[u] != (uint8_t)heavy || !bvh::moves(heavy, c[u], plane)) continue;
                    const float4 l = olo[i], h = ohi[i];
                    const float plo[3] = {l.x, l.y, l.z}, phi[3] = {h.x, h.y, h.z};
                    grow3(mn, mx, l, h);
                    sm[0]++;
                    sm[1] += bvh::leaves_boundary(plo, phi, hb) ? 1u : 0u;
                    side[i] = (uint8_t)(heavy ^ 1);
                }
            }
            block_reduce<WAVES, 3, 3, 2>(mn, mx, sm, lds);
            for (int k = 0; k < 3; k++) { lb.lo[k] = fminf(lb.lo[k], mn[k]); lb.hi[k] = fmaxf(lb.hi[k], mx[k]); }
            if (sm[1]) hb = block_bounds<WAVES>(olo, ohi, side, heavy, count, lds);
            if (heavy == 0) { box0 = hb; box1 = lb; cnt0 -= sm[0]; cnt1 += sm[0]; }
            else { box1 = hb; box0 = lb; cnt1 -= sm[0]; cnt0 += sm[0]; }
        }
    }

    // stable partition by centre < best plane (not by the side flags: a centre on the plane goes right); the rows move with it
    const float *bc = p.in.ctr + (size_t)best_axis * p.n + first;
    uint32_t nl = 0;
    for (uint32_t i = t; i < count; i += kLanes) nl += bvh::side_of(bc[i], best_plane) == 0 ? 1u : 0u;
    block_reduce<WAVES, 0, 0, 1>(nullptr, nullptr, &nl, lds);
    const int wave = t >> 6, lane = t & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t run_l = 0, run_r = 0;
    for (uint32_t base = 0; base < count; base += kLanes) {
        const uint32_t i = base + t;
        const bool valid = i < count;
        const bool left = valid && bvh::side_of(bc[i], best_plane) == 0, right = valid && !left;
        const unsigned long long bl = __ballot(left), br = __ballot(right);
        uint32_t pl = 0, pr = 0, tl = (uint32_t)__popcll(bl), tr = (uint32_t)__popcll(br);
        if (WAVES > 1) {
            __syncthreads();
            if (lane == 0) { lds[wave][0] = tl; lds[wave][1] = tr; }
            __syncthreads();
            tl = tr = 0;
#pragma unroll
            for (int w = 0; w < WAVES; w++) {
                const uint32_t a = lds[w][0], b = lds[w][1];
                if (w < wave) { pl += a; pr += b; }
                tl += a; tr += b;
            }
        }
        if (valid) {
            const size_t from = (size_t)first + i;
            const size_t to = (size_t)first + (left ? run_l + pl + (uint32_t)__popcll(bl & below) : nl + run_r + pr + (uint32_t)__popcll(br & below));
            p.out.perm[to] = p.in.perm[from];
            p.out.lo[to] = p.in.lo[from];
            p.out.hi[to] = p.in.hi[from];
            for (int k = 0; k < 3; k++) p.out.ctr[(size_t)k * p.n + to] = p.in.ctr[(size_t)k * p.n + from];
        }
        run_l += tl; run_r += tr;
    }

    if (t == 0) {
        const uint32_t c = atomicAdd(&p.counters[kCtrNodes], 2u);
        if (c > p.node_capacity || p.node_capacity - c < 2u) {       // the host sizes the array so that this cannot happen
            atomicExch(&p.counters[kCtrOverflow], 1u);
            nd.child = -1;
            return;
        }
        BuildNode &a = p.nodes[c], &b = p.nodes[c + 1];
        for (int k = 0; k < 3; k++) { a.lo[k] = best0.lo[k]; a.hi[k] = best0.hi[k]; b.lo[k] = best1.lo[k]; b.hi[k] = best1.hi[k]; }
        a.first = first;      a.count = nl;         a.child = -1; a.depth = depth + 1;
        b.first = first + nl; b.count = count - nl; b.child = -1; b.depth = depth + 1;
        nd.child = (int32_t)c;
        for (uint32_t s = 0; s < 2; s++) {                           // each child onto the list of its size
            const bool big = (s == 0 ? nl : count - nl) > kSmallNode;
            const uint32_t at = atomicAdd(&p.counters[big ? kCtrBig : kCtrSmall], 1u);
            if (at < p.list_capacity) (big ? p.next_big : p.next_small)[at] = c + s;
            else atomicExch(&p.counters[kCtrOverflow], 1u);
        }
    }
}

// the three passes of the finish over the nodes [begin, begin + count) of one depth (sizes, preorder) or over all (emit)
__global__ __launch_bounds__(kBlock) void bvh_sizes_kernel(const BuildNode *nodes, uint32_t *size, uint32_t begin, uint32_t count) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= count) return;
    const int32_t c = nodes[begin + g].child;
    size[begin + g] = c < 0 ? 1u : 1u + size[c] + size[c + 1];
}
__global__ __launch_bounds__(kBlock) void bvh_preorder_kernel(const BuildNode *nodes, const uint32_t *size, uint32_t *pre, uint32_t begin, uint32_t count) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= count) return;
    const int32_t c = nodes[begin + g].child;
    if (c < 0) return;
    const uint32_t me = pre[begin + g];
    pre[c] = me + 1u;
    pre[c + 1] = me + 1u + size[c];
}
__global__ __launch_bounds__(kBlock) void bvh_emit_kernel(const BuildNode *nodes, const uint32_t *pre, uint32_t count, HostNode *out) {
    const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
    if (g >= count) return;
    const BuildNode nd = nodes[g];
    HostNode h;
    for (int k = 0; k < 3; k++) { h.lo[k] = nd.lo[k]; h.hi[k] = nd.hi[k]; }
    h.is_leaf = nd.child < 0 ? 1 : 0;
    h.a = nd.child < 0 ? (int32_t)nd.first : (int32_t)pre[nd.child];
    h.b = nd.child < 0 ? (int32_t)nd.count : (int32_t)pre[nd.child + 1];
    h.depth = nd.depth;
    out[pre[g]] = h;
}

// the call's device memory: freed when the call returns, on every path
struct Temporaries {
    std::vector<void *> ptrs;
    ~Temporaries() { for (void *q : ptrs) (void)hipFree(q); }
    template <typename T>
    hipError_t alloc(T *&out, size_t count) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(q);
        out = static_cast<T *>(q);
        return e;
    }
    void release(void *q) {
        ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), q), ptrs.end());
        (void)hipFree(q);
    }
};

inline uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

mr_status build_reference_tree_device(const HostMesh &mesh, uint32_t leaf_size, HostTree &tree, BvhBuildPhases &phases, bool &nonfinite) {
    if (leaf_size == 0) leaf_size = 4;
    nonfinite = false;
    phases = BvhBuildPhases();
    const uint32_t n = mesh.n_triangles();
    tree.nodes.clear();
    tree.leaf_prims.clear();
    tree.n_leaves = 0;
    tree.max_depth = 0;
    tree.leaf_size = leaf_size;
    if (n == 0) {                    // the root leaf of nothing: the cleared box, padded; no launch
        bvh::Box none;
        none.clear();
        none.pad();
        HostNode root = HostNode();
        for (int k = 0; k < 3; k++) { root.lo[k] = none.lo[k]; root.hi[k] = none.hi[k]; }
        root.is_leaf = 1;
        tree.nodes.push_back(root);
        tree.n_leaves = 1;
        return MR_OK;
    }
    // inner nodes of one depth hold disjoint objects and more than leaf_size each; a split may put every object on one side, so
    // the tree may have that many inner nodes at each of 32 depths: at most 1 + 64 * max_inner nodes, not 2 n - 1
    const uint64_t max_inner = n / ((uint64_t)leaf_size + 1u);
    const uint64_t bound = 1u + 64u * max_inner;
    if (bound > 0x7fffffffull) return fail(MR_ERR_INVALID, "mr_bvh_build: %u objects are too many for the device builder", n);

    auto t0 = std::chrono::steady_clock::now();
    Temporaries tmp;
    float *d_v = nullptr, *d_spheres = nullptr;
    uint32_t *d_vi = nullptr, *d_leaf = nullptr, *d_counters = nullptr, *d_list[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    ObjTable table[2];
    uint8_t *d_side = nullptr;
    BuildNode *d_nodes = nullptr;
    uint32_t capacity = (uint32_t)std::min<uint64_t>(bound, (uint64_t)n + 64u);
    const uint32_t list_capacity = (uint32_t)(2u * max_inner + 1u);      // the nodes of one depth: the root, or two per inner node above
    MR_HIP_CHECK(tmp.alloc(d_v, mesh.v.size()));
    MR_HIP_CHECK(tmp.alloc(d_vi, mesh.vi.size()));
    MR_HIP_CHECK(tmp.alloc(d_spheres, mesh.spheres.size()));
    for (ObjTable &t : table) {
        MR_HIP_CHECK(tmp.alloc(t.perm, n));
        MR_HIP_CHECK(tmp.alloc(t.lo, n));
        MR_HIP_CHECK(tmp.alloc(t.hi, n));
        MR_HIP_CHECK(tmp.alloc(t.ctr, 3 * (size_t)n));
    }
    for (int k = 0; k < 4; k++) MR_HIP_CHECK(tmp.alloc(d_list[k >> 1][k & 1], list_capacity));     // [depth parity][large, small]
    MR_HIP_CHECK(tmp.alloc(d_leaf, n));
    MR_HIP_CHECK(tmp.alloc(d_side, n));
    MR_HIP_CHECK(tmp.alloc(d_counters, (size_t)kCounters));
    MR_HIP_CHECK(tmp.alloc(d_nodes, capacity));
    if (!mesh.v.empty()) MR_HIP_CHECK(hipMemcpy(d_v, mesh.v.data(), mesh.v.size() * sizeof(float), hipMemcpyHostToDevice));
    MR_HIP_CHECK(hipMemcpy(d_vi, mesh.vi.data(), mesh.vi.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!mesh.spheres.empty())
        MR_HIP_CHECK(hipMemcpy(d_spheres, mesh.spheres.data(), mesh.spheres.size() * sizeof(float), hipMemcpyHostToDevice));
    uint32_t counters[kCounters] = {1u, 0u, 0u, 0u, 0u, 0u};
    MR_HIP_CHECK(hipMemcpy(d_counters, counters, sizeof(counters), hipMemcpyHostToDevice));
    BuildNode root;
    for (int k = 0; k < 3; k++) { root.lo[k] = kInf; root.hi[k] = -kInf; }
    root.first = 0; root.count = n; root.child = -1; root.depth = 0;
    MR_HIP_CHECK(hipMemcpy(d_nodes, &root, sizeof(root), hipMemcpyHostToDevice));

    bvh_objects_kernel<<<blocks_for(n), kBlock>>>(d_v, d_vi, d_spheres, mesh.n_spheres(), n, table[0], d_counters);
    MR_HIP_CHECK(hipGetLastError());
    MR_HIP_CHECK(hipMemcpy(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost));
    phases.prims_ms = ms_since(t0);
    if (counters[kCtrNonFinite]) { nonfinite = true; return MR_OK; }

    t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> level_begin;       // first node of every depth, then the total
    uint32_t total = 1, level_count[2] = {n > kSmallNode ? 1u : 0u, n > kSmallNode ? 0u : 1u};      // large, small nodes of the depth
    const uint32_t zero = 0;
    MR_HIP_CHECK(hipMemcpy(d_list[0][n > kSmallNode ? 0 : 1], &zero, sizeof(zero), hipMemcpyHostToDevice));     // the root is node 0
    for (int depth = 0; depth <= bvh::kMaxDepth && level_count[0] + level_count[1]; depth++) {
        const uint32_t level_nodes = level_count[0] + level_count[1];
        const uint64_t need = (uint64_t)total + 2u * std::min<uint64_t>(level_nodes, max_inner);
        if (need > capacity) {
            const uint32_t grown = (uint32_t)std::min<uint64_t>(bound, std::max<uint64_t>(need, 2u * (uint64_t)capacity));
            BuildNode *d_more = nullptr;
            MR_HIP_CHECK(tmp.alloc(d_more, grown));
            MR_HIP_CHECK(hipMemcpy(d_more, d_nodes, (size_t)total * sizeof(BuildNode), hipMemcpyDeviceToDevice));
            tmp.release(d_nodes);
            d_nodes = d_more;
            capacity = grown;
        }
        BuildArrays p;
        p.in = table[depth & 1]; p.out = table[(depth + 1) & 1];
        p.n = n; p.leaf_size = leaf_size;
        p.nodes = d_nodes; p.node_capacity = capacity;
        p.leaf_out = d_leaf; p.side = d_side; p.counters = d_counters;
        p.next_big = d_list[(depth + 1) & 1][0]; p.next_small = d_list[(depth + 1) & 1][1]; p.list_capacity = list_capacity;
        MR_HIP_CHECK(hipMemsetAsync(d_counters + kCtrBig, 0, 2 * sizeof(uint32_t), nullptr));
        if (level_count[0]) {
            p.list = d_list[depth & 1][0];
            bvh_level_kernel<4><<<level_count[0], 256>>>(p);
        }
        if (level_count[1]) {
            p.list = d_list[depth & 1][1];
            bvh_level_kernel<1><<<level_count[1], 64>>>(p);
        }
        MR_HIP_CHECK(hipGetLastError());
        MR_HIP_CHECK(hipMemcpy(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost));
        if (counters[kCtrOverflow] || counters[kCtrNodes] < total || counters[kCtrNodes] > capacity ||
            counters[kCtrBig] + counters[kCtrSmall] != counters[kCtrNodes] - total)
            return fail(MR_ERR_HIP, "mr_bvh_build: the device builder's node array overflowed (%u of %u at depth %d)", counters[kCtrNodes], capacity, depth);
        level_begin.push_back(total - level_nodes);
        level_count[0] = counters[kCtrBig];
        level_count[1] = counters[kCtrSmall];
        total = counters[kCtrNodes];
    }
    const uint32_t level_nodes = level_count[0] + level_count[1];
    if (level_nodes) return fail(MR_ERR_HIP, "mr_bvh_build: the device builder went below depth %d", bvh::kMaxDepth);
    level_begin.push_back(total);
    phases.levels_ms = ms_since(t0);

    t0 = std::chrono::steady_clock::now();
    uint32_t *d_size = nullptr, *d_pre = nullptr;
    HostNode *d_out = nullptr;
    MR_HIP_CHECK(tmp.alloc(d_size, total));
    MR_HIP_CHECK(tmp.alloc(d_pre, total));
    MR_HIP_CHECK(tmp.alloc(d_out, total));
    const size_t depths = level_begin.size() - 1;
    for (size_t d = depths; d-- > 0;) {
        const uint32_t count = level_begin[d + 1] - level_begin[d];
        bvh_sizes_kernel<<<blocks_for(count), kBlock>>>(d_nodes, d_size, level_begin[d], count);
    }
    MR_HIP_CHECK(hipMemsetAsync(d_pre, 0, sizeof(uint32_t), nullptr));       // the root is node 0 of the pre-order
    for (size_t d = 0; d < depths; d++) {
        const uint32_t count = level_begin[d + 1] - level_begin[d];
        bvh_preorder_kernel<<<blocks_for(count), kBlock>>>(d_nodes, d_size, d_pre, level_begin[d], count);
    }
    bvh_emit_kernel<<<blocks_for(total), kBlock>>>(d_nodes, d_pre, total, d_out);
    MR_HIP_CHECK(hipGetLastError());
    tree.nodes.resize(total);
    tree.leaf_prims.resize(n);
    MR_HIP_CHECK(hipMemcpy(tree.nodes.data(), d_out, (size_t)total * sizeof(HostNode), hipMemcpyDeviceToHost));
    MR_HIP_CHECK(hipMemcpy(tree.leaf_prims.data(), d_leaf, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    tree.n_leaves = counters[kCtrLeaves];
    tree.max_depth = (uint32_t)(depths - 1);
    phases.finish_ms = ms_since(t0);
    return MR_OK;
}

}  // namespace mr
