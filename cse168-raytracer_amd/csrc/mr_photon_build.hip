// mr_photon_build.hip -- Photon_map::store, scale_photon_power and balance (PhotonMap.cpp:255-359, 409-476) for one batch of
// records on an empty map, on the device (mr_photon_map_build_device).  The yardstick is the host path of mr_photon.cpp; every
// kernel below reproduces its bits:
//
//   build_store_kernel     capping, power * scale, bounding box, the two direction bytes -- or the photon's deferral to the
//                          host when the device's double acos / atan2 could round the scaled angle across a whole number
//   build_fix_kernel       writes the bytes the host computed for the deferred photons
//   build_init_kernel      radix keys of the three coordinates (order-preserving, -0 folded onto +0), index-ordered lists, root
//   radix_hist_kernel      |
//   radix_scatter_kernel   | four stable 8-bit LSD passes per axis: three lists sorted by (coordinate, storage index)
//   build_node_kernel      one heap level: axis from the running box, left-balanced median, heap / plane, the child segments
//   build_mark_kernel      "goes left" of every live list position, by the host comparator against the segment's median
//   build_scatter_kernel   stable partition of the three lists inside every segment, from one exclusive scan of the marks
//   build_scan_kernel / build_scan_sums_kernel   that scan (and the radix passes')
//   build_pack_kernel      rec / power / direction bytes in heap order, directions through the host's tables
//   build_subtree_kernel   bounds of every subtree, bottom-up one heap level per launch, in the host's operand order
//   build_boxes_kernel     per block root: bounds of its own six levels, and its subtree's
//
// A segment is the position range [start, end] it has in all three lists; a stable partition keeps each child sorted on
// all three axes, so nothing is sorted twice.  Nodes are addressed by heap index: the children of h are 2h and 2h + 1, and in
// a left-balanced tree of n nodes exactly the indices 1 ... n exist.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_photon_tree.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

namespace mr {
namespace {

constexpr int kRadixTile = 1024;        // elements per one-wave workgroup of a radix pass
constexpr int kScanItems = 16, kScanTile = kBlock * kScanItems;

// one node of the tree under construction
struct BuildNode {
    int32_t start, end, median, axis;   // segment, the median's position in the list of `axis`
    uint32_t photon;                    // storage index of the node's photon
    int32_t medpos[3];                  // where that photon sits in each list
    float lo[3], hi[3];                 // running box
    int32_t pad[2];
};
static_assert(sizeof(BuildNode) == 64, "one node per 64 bytes");

// ---- store --------------------------------------------------------------------------------------------------------------
// The scaled angle decides a byte on the device only when it is finite and farther than 2^-20 from every whole number.
__device__ __forceinline__ bool decided(double scaled) {
    return isfinite(scaled) && fabs(scaled - rint(scaled)) > (1.0 / 1048576.0);
}

__global__ __launch_bounds__(kBlock) void build_store_kernel(const float *records, uint32_t m, float scale, float *pos, float *power,
                                                             uint8_t *dir, float4 *deferred, PhotonBuildStatus *status) {
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * kBlock;
    const uint32_t m_round = (m + 63u) & ~63u;                         // whole waves: the ballot below
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    bool bad = false;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < m_round; i += stride) {
        bool defer = false;
        float d[3] = {0.f, 0.f, 0.f};
        if (i < m) {
            const float *r = records + 12 * (size_t)i;
            for (int c = 0; c < 3; c++) {
                const float p = r[c];
                if (!isfinite(p)) bad = true;
                pos[3 * (size_t)i + c] = p;
                const uint32_t k = order_key(p);
                lo[c] = k < lo[c] ? k : lo[c];
                hi[c] = k > hi[c] ? k : hi[c];
                d[c] = r[3 + c];
                power[3 * (size_t)i + c] = r[6 + c] * scale;
            }
            const double t = acos((double)d[2]) * (256.0 / M_PI);
            const double f = atan2((double)d[1], (double)d[0]) * (256.0 / (2.0 * M_PI));
            if (decided(t) && decided(f)) {
                const int theta = int(t), phi = int(f);
                dir[2 * (size_t)i] = theta_byte(theta);
                dir[2 * (size_t)i + 1] = phi_byte(phi);
            } else {
                defer = true;
            }
        }
        const unsigned long long mask = __ballot(defer);
        if (mask) {                                                     // wave-uniform
            const int leader = __ffsll((long long)mask) - 1;
            uint32_t base = 0;
            if ((int)lane == leader) base = atomicAdd(&status->deferred, (uint32_t)__popcll(mask));
            base = __shfl(base, leader, 64);
            if (defer) {
                const uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (at < m) deferred[at] = make_float4(__uint_as_float(i), d[0], d[1], d[2]);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int c = 0; c < 3; c++) {
            const uint32_t l = __shfl_xor(lo[c], off, 64), h = __shfl_xor(hi[c], off, 64);
            lo[c] = l < lo[c] ? l : lo[c];
            hi[c] = h > hi[c] ? h : hi[c];
        }
    if (lane == 0)
        for (int c = 0; c < 3; c++) { atomicMin(&status->lo[c], lo[c]); atomicMax(&status->hi[c], hi[c]); }
    if (bad) atomicOr(&status->nonfinite, 1u);
}

// deferred[j] = (index bits, theta | phi << 8 as bits, -, -) after the host's pass
__global__ __launch_bounds__(kBlock) void build_fix_kernel(const float4 *deferred, uint32_t count, uint32_t m, uint8_t *dir) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < count; j += stride) {
        const float4 e = deferred[j];
        const uint32_t i = __float_as_uint(e.x), b = __float_as_uint(e.y);
        if (i < m) { dir[2 * (size_t)i] = (uint8_t)(b & 255u); dir[2 * (size_t)i + 1] = (uint8_t)((b >> 8) & 255u); }
    }
}

// ---- the three sorted lists -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void build_init_kernel(const float *pos, uint32_t m, const PhotonBuildStatus *status, uint32_t *keys,
                                                            uint32_t *lists, uint32_t *pseg, BuildNode *nodes) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) {
        for (int a = 0; a < 3; a++) {
            keys[(size_t)a * m + i] = order_key(pos[3 * (size_t)i + a]);
            lists[(size_t)a * m + i] = i;
        }
        pseg[i] = 1u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        BuildNode r = {};
        r.start = 0; r.end = (int32_t)m - 1;
        for (int c = 0; c < 3; c++) { r.lo[c] = key_float(status->lo[c]); r.hi[c] = key_float(status->hi[c]); }
        nodes[1] = r;
    }
}

// grid (tiles, 3), one wave per workgroup; hist[(axis * 256 + digit) * tiles + tile]
__global__ __launch_bounds__(64) void radix_hist_kernel(const uint32_t *keys, uint32_t m, uint32_t shift, uint32_t tiles, uint32_t *hist) {
    __shared__ uint32_t cnt[256];
    const uint32_t lane = threadIdx.x, a = blockIdx.y, tile = blockIdx.x;
    for (int d = lane; d < 256; d += 64) cnt[d] = 0;
    __syncthreads();
    for (int r = 0; r < kRadixTile / 64; r++) {
        const uint32_t i = tile * kRadixTile + r * 64 + lane;
        if (i < m) atomicAdd(&cnt[(keys[(size_t)a * m + i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (int d = lane; d < 256; d += 64) hist[((size_t)a * 256 + d) * tiles + tile] = cnt[d];
}

// hist: exclusively scanned over all three axes (axis a's offsets start at a * m)
__global__ __launch_bounds__(64) void radix_scatter_kernel(const uint32_t *keys, const uint32_t *vals, uint32_t m, uint32_t shift, uint32_t tiles,
                                                           const uint32_t *hist, uint32_t *keys_out, uint32_t *vals_out) {
    __shared__ uint32_t base[256];
    const uint32_t lane = threadIdx.x, a = blockIdx.y, tile = blockIdx.x;
    for (int d = lane; d < 256; d += 64) base[d] = hist[((size_t)a * 256 + d) * tiles + tile] - a * m;
    __syncthreads();
    for (int r = 0; r < kRadixTile / 64; r++) {
        const uint32_t i = tile * kRadixTile + r * 64 + lane;
        const bool valid = i < m;
        uint32_t key = 0, val = 0;
        if (valid) { key = keys[(size_t)a * m + i]; val = vals[(size_t)a * m + i]; }
        const uint32_t d = (key >> shift) & 255u;
        unsigned long long peers = __ballot(valid);                    // the valid lanes with my digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(valid && bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        uint32_t at = 0;
        if (valid) at = base[d] + rank;
        __syncthreads();
        if (valid && rank == 0) base[d] += (uint32_t)__popcll(peers);   // one lane per digit
        __syncthreads();
        if (valid && at < m) { keys_out[(size_t)a * m + at] = key; vals_out[(size_t)a * m + at] = val; }
    }
}

// ---- exclusive scan of uint32 -----------------------------------------------------------------------------------------------
// WRITE = false: sums[block] = the block's total.  WRITE = true: out = exclusive scan, starting at sums[block] (0 if NULL).
// in == out is allowed: a thread reads and writes its own items only.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void build_scan_kernel(const uint32_t *in, uint32_t *out, uint32_t *sums, uint32_t n) {
    __shared__ uint32_t s[kBlock];
    const uint32_t t = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)t * kScanItems;
    uint32_t v[kScanItems], mine = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) { v[k] = first + k < n ? in[first + k] : 0u; mine += v[k]; }
    s[t] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < kBlock; off <<= 1) {
        uint32_t add = 0;
        if (t >= off) add = s[t - off];
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    if (WRITE) {
        uint32_t run = s[t] - mine + (sums ? sums[blockIdx.x] : 0u);
#pragma unroll
        for (int k = 0; k < kScanItems; k++) { if (first + k < n) out[first + k] = run; run += v[k]; }
    } else if (t == kBlock - 1) {
        sums[blockIdx.x] = s[t];
    }
}

// one workgroup: sums[0 .. nb) becomes its exclusive scan
__global__ __launch_bounds__(kBlock) void build_scan_sums_kernel(uint32_t *sums, uint32_t nb) {
    __shared__ uint32_t s[kBlock];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t first = 0; first < nb; first += kBlock) {
        const uint32_t v = first + t < nb ? sums[first + t] : 0u;
        s[t] = v;
        __syncthreads();
        for (uint32_t off = 1; off < kBlock; off <<= 1) {
            uint32_t add = 0;
            if (t >= off) add = s[t - off];
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        if (first + t < nb) sums[first + t] = carry + s[t] - v;
        carry += s[kBlock - 1];
        __syncthreads();
    }
}

// ---- one level ------------------------------------------------------------------------------------------------------------
// nodes first ... last of one heap level
__global__ __launch_bounds__(kBlock) void build_node_kernel(BuildNode *nodes, uint32_t first, uint32_t last, uint32_t m, const float *pos,
                                                            const uint32_t *lists, uint32_t *heap, int32_t *plane) {
    const uint32_t h = first + blockIdx.x * kBlock + threadIdx.x;
    if (h > last) return;
    BuildNode nd = nodes[h];
    if (nd.start < 0 || nd.end >= (int32_t)m || nd.start > nd.end) return;     // never: a broken segment writes nothing
    if (nd.start == nd.end) {                                           // Balancer::segment writes it into the parent's child slot
        heap[h] = lists[nd.start];
        plane[h] = 0;
        return;
    }
    const int axis = split_axis(nd.lo, nd.hi);
    const int32_t median = left_balanced_median(nd.start, nd.end);
    const uint32_t photon = lists[(size_t)axis * m + median];
    if (photon >= m) return;                                            // never
    heap[h] = photon;
    plane[h] = axis;
    nodes[h].median = median; nodes[h].axis = axis; nodes[h].photon = photon;
    const float split = pos[3 * (size_t)photon + axis];
    if (median > nd.start && 2 * (size_t)h <= m) {
        BuildNode c = nd;
        c.end = median - 1;
        for (int k = 0; k < 3; k++) c.hi[k] = k == axis ? split : c.hi[k];
        nodes[2 * (size_t)h] = c;
    }
    if (median < nd.end && 2 * (size_t)h + 1 <= m) {
        BuildNode c = nd;
        c.start = median + 1;
        for (int k = 0; k < 3; k++) c.lo[k] = k == axis ? split : c.lo[k];
        nodes[2 * (size_t)h + 1] = c;
    }
}

// marks[a * m + p] = the photon at position p of list a goes to the left child of its segment
__global__ __launch_bounds__(kBlock) void build_mark_kernel(BuildNode *nodes, uint32_t m, const float *pos, const uint32_t *lists,
                                                            const uint32_t *pseg, uint32_t *marks) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < 3 * m; k += stride) {
        const uint32_t a = k / m, p = k - a * m;
        const uint32_t h = pseg[p];
        uint32_t left = 0;
        if (h != 0 && h <= m) {
            const BuildNode *nd = &nodes[h];
            const uint32_t e = lists[k], mp = nd->photon;
            const int axis = nd->axis;
            if (nd->start != nd->end && e < m && mp < m && (unsigned)axis < 3u) {
                if (e == mp) {
                    nodes[h].medpos[a] = (int32_t)p;
                } else {
                    const float pa = pos[3 * (size_t)e + axis], pb = pos[3 * (size_t)mp + axis];
                    left = (pa != pb ? pa < pb : e < mp) ? 1u : 0u;     // the comparator of Balancer::segment
                }
            }
        }
        marks[k] = left;
    }
}

// left elements to [start, median - 1], right ones to [median + 1, end], both in their old order; the median's slot is dead
__global__ __launch_bounds__(kBlock) void build_scatter_kernel(const BuildNode *nodes, uint32_t m, const uint32_t *lists, const uint32_t *pseg,
                                                               const uint32_t *marks, const uint32_t *scan, uint32_t *lists_out,
                                                               uint32_t *pseg_out) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t k = blockIdx.x * kBlock + threadIdx.x; k < 3 * m; k += stride) {
        const uint32_t a = k / m, p = k - a * m;
        const uint32_t h = pseg[p];
        if (h == 0 || h > m) { if (a == 0) pseg_out[p] = 0u; continue; }
        const BuildNode *nd = &nodes[h];
        const int32_t start = nd->start, end = nd->end, median = nd->median;
        if (start == end) { if (a == 0) pseg_out[p] = 0u; continue; }
        if (start < 0 || end >= (int32_t)m || median < start || median > end) continue;      // never
        const uint32_t e = lists[k];
        if (e == nd->photon) { if (a == 0) pseg_out[median] = 0u; continue; }
        const int32_t lefts = (int32_t)(scan[k] - scan[(size_t)a * m + start]);
        int32_t q;
        uint32_t child;
        if (marks[k]) { q = start + lefts; child = 2u * h; }
        else { q = median + 1 + ((int32_t)p - start) - lefts - ((int32_t)p > nd->medpos[a] ? 1 : 0); child = 2u * h + 1u; }
        if (q < start || q > end) continue;                             // never
        lists_out[(size_t)a * m + q] = e;
        if (a == 0) pseg_out[q] = child;
    }
}

// ---- planes and boxes -------------------------------------------------------------------------------------------------------
// tables: the host's DirTables (costheta, sintheta, cosphi, sinphi, 256 floats each)
__global__ __launch_bounds__(kBlock) void build_pack_kernel(uint32_t m, const uint32_t *heap, const int32_t *plane, const float *pos,
                                                            const float *power, const uint8_t *dir, const float *tables, float4 *rec,
                                                            float4 *out_power, uint8_t *out_dir) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i <= m; i += stride) {
        if (i == 0) {
            rec[0] = rec[1] = out_power[0] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const size_t s = heap[i] < m ? heap[i] : 0;
        const uint8_t th = dir[2 * s], ph = dir[2 * s + 1];
        const float sintheta = tables[256 + th], costheta = tables[th], cosphi = tables[512 + ph], sinphi = tables[768 + ph];
        rec[2 * (size_t)i] = make_float4(pos[3 * s], pos[3 * s + 1], pos[3 * s + 2], __int_as_float(plane[i]));
        rec[2 * (size_t)i + 1] = make_float4(sintheta * cosphi, sintheta * sinphi, costheta, 0.0f);       // PhotonMap.cpp:66-71
        out_power[i] = make_float4(power[3 * s], power[3 * s + 1], power[3 * s + 2], 0.0f);
        out_dir[2 * (size_t)(i - 1)] = th; out_dir[2 * (size_t)(i - 1) + 1] = ph;
    }
}

// sub[6 j ...] = (lo, hi) of the subtree of node j; the children's level is done.  Operand order as mr_photon_map_balance
// has it (std::min / std::max keep their first argument when the two compare equal, which is what tells -0 from +0).
__global__ __launch_bounds__(kBlock) void build_subtree_kernel(const float4 *rec, uint32_t first, uint32_t last, uint32_t m, float *sub) {
    const uint32_t j = first + blockIdx.x * kBlock + threadIdx.x;
    if (j > last) return;
    const float4 a = rec[2 * (size_t)j];
    const float pj[3] = {a.x, a.y, a.z};
    for (int c = 0; c < 3; c++) {
        float lo = pj[c], hi = pj[c];
        for (size_t ch = 2 * (size_t)j; ch <= 2 * (size_t)j + 1 && ch <= m; ch++) {
            const float l = sub[6 * ch + c], h = sub[6 * ch + 3 + c];
            lo = l < lo ? l : lo;
            hi = hi < h ? h : hi;
        }
        sub[6 * (size_t)j + c] = lo; sub[6 * (size_t)j + 3 + c] = hi;
    }
}

struct BoxLayers { int32_t layers, base[4]; uint32_t total; };

__global__ __launch_bounds__(kBlock) void build_boxes_kernel(const float4 *rec, const float *sub, uint32_t m, BoxLayers bl, float4 *boxes) {
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id >= (bl.total ? bl.total : 1u)) return;
    const float inf = INFINITY;
    int L = 0;
    uint32_t base = 0;
#pragma unroll
    for (int l = 1; l < 4; l++)
        if (l < bl.layers && id >= (uint32_t)bl.base[l]) { L = l; base = (uint32_t)bl.base[l]; }
    const unsigned long long r = bl.layers ? (1ull << (6 * L)) + (id - base) : (unsigned long long)m + 1ull;
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    float4 *b = &boxes[4 * (size_t)id];
    if (r > m) {
        b[0] = b[2] = make_float4(inf, inf, inf, 0.f);
        b[1] = b[3] = make_float4(-inf, -inf, -inf, 0.f);
        return;
    }
    for (int l = 0; l < 6; l++)
        for (unsigned long long o = 0; o < (1ull << l); o++) {
            const unsigned long long j = (r << l) + o;
            if (j > m) break;
            const float4 a = rec[2 * j];
            const float pj[3] = {a.x, a.y, a.z};
            for (int c = 0; c < 3; c++) { lo[c] = pj[c] < lo[c] ? pj[c] : lo[c]; hi[c] = hi[c] < pj[c] ? pj[c] : hi[c]; }
        }
    b[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
    b[1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    b[2] = make_float4(sub[6 * r], sub[6 * r + 1], sub[6 * r + 2], 0.f);
    b[3] = make_float4(sub[6 * r + 3], sub[6 * r + 4], sub[6 * r + 5], 0.f);
}

inline unsigned blocks_of(unsigned long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// exclusive scan of data[0 .. n) into out (in place allowed), through `sums`
mr_status scan(const uint32_t *in, uint32_t *out, uint32_t *sums, uint32_t n, hipStream_t stream) {
    const unsigned nb = (n + kScanTile - 1) / kScanTile;
    if (nb <= 1) {
        hipLaunchKernelGGL(build_scan_kernel<true>, dim3(1), dim3(kBlock), 0, stream, in, out, (uint32_t *)nullptr, n);
        MR_HIP_CHECK(hipGetLastError());
        return MR_OK;
    }
    hipLaunchKernelGGL(build_scan_kernel<false>, dim3(nb), dim3(kBlock), 0, stream, in, out, sums, n);
    MR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(build_scan_sums_kernel, dim3(1), dim3(kBlock), 0, stream, sums, nb);
    MR_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(build_scan_kernel<true>, dim3(nb), dim3(kBlock), 0, stream, in, out, sums, n);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

// ---- workspace ----------------------------------------------------------------------------------------------------------------
struct PhotonBuildWork {
    uint32_t m = 0, tiles = 0;
    float *pos = nullptr, *power = nullptr, *sub = nullptr;
    uint8_t *dir = nullptr;
    float4 *deferred = nullptr;
    PhotonBuildStatus *status = nullptr;
    uint32_t *keys[2] = {nullptr, nullptr}, *lists[2] = {nullptr, nullptr}, *pseg[2] = {nullptr, nullptr};
    uint32_t *hist = nullptr, *marks = nullptr, *scan = nullptr, *sums = nullptr, *heap = nullptr;
    int32_t *plane = nullptr;
    BuildNode *nodes = nullptr;
    float *tables = nullptr;
};

namespace {
// one walk over the layout serves the size (base == nullptr) and the pointers
size_t carve(PhotonBuildWork &w, uint32_t m, char *base) {
    size_t at = 0;
    auto take = [&](auto *&p, size_t count) {
        using T = std::remove_reference_t<decltype(*p)>;
        p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += align256(count * sizeof(T));
    };
    const size_t n = m ? m : 1;
    w.m = m;
    w.tiles = (uint32_t)((n + kRadixTile - 1) / kRadixTile);
    const size_t hist = 3 * 256 * (size_t)w.tiles, longest = hist > 3 * n ? hist : 3 * n;
    take(w.status, 1);
    take(w.tables, 1024);
    take(w.pos, 3 * n); take(w.power, 3 * n); take(w.dir, 2 * n); take(w.deferred, n);
    take(w.keys[0], 3 * n); take(w.keys[1], 3 * n); take(w.lists[0], 3 * n); take(w.lists[1], 3 * n);
    take(w.pseg[0], n); take(w.pseg[1], n);
    take(w.hist, hist); take(w.marks, 3 * n); take(w.scan, 3 * n);
    take(w.sums, (longest + kScanTile - 1) / kScanTile + 1);
    take(w.heap, n + 1); take(w.plane, n + 1);
    take(w.nodes, n + 2);
    take(w.sub, 6 * (n + 2));
    return at;
}
}  // namespace

mr_status photon_build_begin(uint32_t m, const float *tables1024, PhotonBuildWork **out, hipStream_t stream) {
    *out = nullptr;
    PhotonBuildWork *w = new (std::nothrow) PhotonBuildWork();
    if (!w) return fail(MR_ERR_NOMEM, "out of host memory");
    const size_t bytes = carve(*w, m, nullptr);
    char *base = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&base), bytes);
    if (e != hipSuccess) { delete w; return fail(MR_ERR_NOMEM, "mr_photon_map_build_device: %zu bytes of device workspace: %s", bytes, hipGetErrorString(e)); }
    carve(*w, m, base);
    *out = w;
    PhotonBuildStatus st;
    const float big = 1e8f;                                          // Photon_map's initial box (PhotonMap.cpp:36-38)
    for (int c = 0; c < 3; c++) { st.lo[c] = order_key(big); st.hi[c] = order_key(-big); }
    st.nonfinite = 0; st.deferred = 0;
    MR_HIP_CHECK(hipMemcpyAsync(w->status, &st, sizeof(st), hipMemcpyHostToDevice, stream));
    MR_HIP_CHECK(hipMemcpyAsync(w->tables, tables1024, 1024 * sizeof(float), hipMemcpyHostToDevice, stream));
    MR_HIP_CHECK(hipStreamSynchronize(stream));
    return MR_OK;
}

void photon_build_end(PhotonBuildWork *w) {
    if (!w) return;
    (void)hipFree(w->status);                                        // the base of the one allocation
    delete w;
}

float4 *photon_build_deferred(PhotonBuildWork *w) { return w->deferred; }

mr_status launch_photon_build_store(PhotonBuildWork *w, const mr_photon_record *d_records, float scale, PhotonBuildStatus *status, float lo[3], float hi[3],
                                    hipStream_t stream) {
    if (w->m)
        hipLaunchKernelGGL(build_store_kernel, dim3(grid_for(w->m)), dim3(kBlock), 0, stream, reinterpret_cast<const float *>(d_records), w->m, scale,
                           w->pos, w->power, w->dir, w->deferred, w->status);
    MR_HIP_CHECK(hipGetLastError());
    MR_HIP_CHECK(hipMemcpyAsync(status, w->status, sizeof(*status), hipMemcpyDeviceToHost, stream));
    MR_HIP_CHECK(hipStreamSynchronize(stream));
    for (int c = 0; c < 3; c++) { lo[c] = key_float(status->lo[c]); hi[c] = key_float(status->hi[c]); }
    return MR_OK;
}

mr_status launch_photon_build_fix(PhotonBuildWork *w, uint32_t count, hipStream_t stream) {
    if (!count) return MR_OK;
    hipLaunchKernelGGL(build_fix_kernel, dim3(grid_for(count)), dim3(kBlock), 0, stream, w->deferred, count, w->m, w->dir);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

mr_status launch_photon_build_tree(PhotonBuildWork *w, hipStream_t stream) {
    const uint32_t m = w->m;
    if (m == 0) return MR_OK;
    MR_HIP_CHECK(hipMemsetAsync(w->heap, 0, ((size_t)m + 1) * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(build_init_kernel, dim3(grid_for(m)), dim3(kBlock), 0, stream, w->pos, m, w->status, w->keys[0], w->lists[0], w->pseg[0], w->nodes);
    MR_HIP_CHECK(hipGetLastError());
    if (m > 1) {
        for (int pass = 0; pass < 4; pass++) {                        // ends in buffer 0
            const int in = pass & 1, out = in ^ 1;
            hipLaunchKernelGGL(radix_hist_kernel, dim3(w->tiles, 3), dim3(64), 0, stream, w->keys[in], m, 8u * pass, w->tiles, w->hist);
            MR_HIP_CHECK(hipGetLastError());
            mr_status st = scan(w->hist, w->hist, w->sums, 3u * 256u * w->tiles, stream);
            if (st != MR_OK) return st;
            hipLaunchKernelGGL(radix_scatter_kernel, dim3(w->tiles, 3), dim3(64), 0, stream, w->keys[in], w->lists[in], m, 8u * pass, w->tiles, w->hist,
                               w->keys[out], w->lists[out]);
            MR_HIP_CHECK(hipGetLastError());
        }
    }
    int cur = 0;
    for (uint64_t first = 1; first <= m; first <<= 1) {
        const uint32_t last = (uint32_t)(2 * first - 1 < m ? 2 * first - 1 : m);
        hipLaunchKernelGGL(build_node_kernel, dim3(blocks_of(last - first + 1)), dim3(kBlock), 0, stream, w->nodes, (uint32_t)first, last, m, w->pos,
                           w->lists[cur], w->heap, w->plane);
        MR_HIP_CHECK(hipGetLastError());
        if (2 * first > m) break;                                     // no level below
        hipLaunchKernelGGL(build_mark_kernel, dim3(grid_for(3ull * m)), dim3(kBlock), 0, stream, w->nodes, m, w->pos, w->lists[cur], w->pseg[cur], w->marks);
        MR_HIP_CHECK(hipGetLastError());
        mr_status st = scan(w->marks, w->scan, w->sums, 3u * m, stream);
        if (st != MR_OK) return st;
        hipLaunchKernelGGL(build_scatter_kernel, dim3(grid_for(3ull * m)), dim3(kBlock), 0, stream, w->nodes, m, w->lists[cur], w->pseg[cur], w->marks,
                           w->scan, w->lists[cur ^ 1], w->pseg[cur ^ 1]);
        MR_HIP_CHECK(hipGetLastError());
        cur ^= 1;
    }
    return MR_OK;
}

mr_status launch_photon_build_pack(PhotonBuildWork *w, PhotonMapDev &dev, uint8_t *d_dir, hipStream_t stream) {
    const uint32_t m = w->m;
    hipLaunchKernelGGL(build_pack_kernel, dim3(grid_for((unsigned long long)m + 1)), dim3(kBlock), 0, stream, m, w->heap, w->plane, w->pos, w->power, w->dir,
                       w->tables, dev.rec, dev.power, d_dir);
    MR_HIP_CHECK(hipGetLastError());
    uint64_t top = 1;
    while (2 * top <= m) top <<= 1;                                   // first node of the deepest level
    for (uint64_t first = top; first >= 1 && m; first >>= 1) {
        const uint32_t last = (uint32_t)(2 * first - 1 < m ? 2 * first - 1 : m);
        hipLaunchKernelGGL(build_subtree_kernel, dim3(blocks_of(last - first + 1)), dim3(kBlock), 0, stream, dev.rec, (uint32_t)first, last, m, w->sub);
        MR_HIP_CHECK(hipGetLastError());
    }
    BoxLayers bl = {};
    bl.layers = dev.layers;
    for (int l = 0; l < 4; l++) bl.base[l] = dev.layer_base[l];
    const size_t total = photon_map_layout(dev, m);                    // what the caller laid dev out with
    bl.total = (uint32_t)total;
    hipLaunchKernelGGL(build_boxes_kernel, dim3(blocks_of(total ? total : 1)), dim3(kBlock), 0, stream, dev.rec, w->sub, m, bl, dev.boxes);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
