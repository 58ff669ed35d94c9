// mr_photon_walk.hip -- Scene::tracePhotons / traceCausticPhotons for one DirectionalAreaLight (Scene.cpp:351-472) with
// Scene::tracePhoton (Scene.cpp:529-655) per emitted photon, on the device:
//
//   photon_walk_kernel      one lane owns one photon for its whole life: emission (sampleDisc, Utility.h:82-95) -> Scene::trace
//                           -> the roulette over the hit material's kd / ks / kt averages -> store / absorb / the next segment
//                           (Ray::random, Ray::reflect, the Fresnel draw, Ray::refract).  Origin, direction, power, emission
//                           index and depth stay in registers between bounces; the traversal is trace_ray (mr_traverse.h) with
//                           the default exact arithmetic, so every hit is the record mr_trace returns for the same segment.
//                           Lanes whose photon has died re-arm from the round's emission counter between whole segments:
//                           wave64 ballot + prefix sum, one atomic per wave.  Everything a photon does is keyed by its
//                           emission index (random numbers, record slots), never by the lane that walks it.
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
#include "mr_recursion.h"
#include "mr_traverse.h"

namespace mr {
namespace {

using namespace rec;

constexpr uint32_t kNoPhoton = 0xFFFFFFFFu;
constexpr int kDiscAttempts = 64;             // sampleDisc's rejection loop, bounded: (1 - pi/4)^64 ~ 1e-43, then the centre

struct WalkArgs {
    TraceParams tp;
    MeshMat m;
    float pos[3], dir[3], t1[3], t2[3], power[3], radius;
    uint32_t hdir, hevent, hdisc;             // pcg32 of the seed in its three domains (directions, events, disc)
    uint32_t caustic, max_depth;
    uint32_t first, count;                    // the round: emissions first ... first + count - 1
    float4 *slots;                            // count * max_depth records of 3 float4
    uint32_t *words;                          // count packed words
    unsigned *next;                           // the round's emission counter (zeroed by the host)
};

// state word of a lane: depth (bits 0-7), stores (8-15), first bounce specular (16)
__device__ __forceinline__ float avg3(const float *c) { return ((c[0] + c[1]) + c[2]) / 3.0f; }      // Vector3::average

template <int VAR>
__global__ __launch_bounds__(kTraceBlock) void photon_walk_kernel(WalkArgs a) {
    extern __shared__ int s_stack[];                  // [stack_depth][kTraceBlock]
    const int tid = threadIdx.x, lane = tid & 63;
    Stats st = {0ull, 0ull};

    uint32_t my = kNoPhoton, state = 0;               // local emission index of the lane's photon
    float o[3] = {0.f, 0.f, 0.f}, d[3] = {1.f, 1.f, 1.f}, pw[3] = {0.f, 0.f, 0.f};
    bool exhausted = false;                           // wave-uniform: the counter has passed the round's end

    while (true) {
        // ---- re-arm the idle lanes with the next emissions
        const unsigned long long idle = __ballot(my == kNoPhoton);
        if (idle && !exhausted) {
            const unsigned n_idle = (unsigned)__popcll(idle);
            unsigned base = 0;
            if (lane == 0) base = atomicAdd(a.next, n_idle);
            base = __shfl(base, 0, 64);
            const unsigned cand = base + (unsigned)__popcll(idle & ((1ull << lane) - 1ull));
            if (my == kNoPhoton && cand < a.count) {
                my = cand;
                state = 0;
                // DirectionalAreaLight::samplePhotonOrigin (DirectionalAreaLight.h:20-24)
                const uint32_t hd = pcg32(a.hdisc ^ (a.first + cand));
                float x = 0.0f, y = 0.0f;
                for (int k = 0; k < kDiscAttempts; k++) {
                    const uint32_t hk = pcg32(hd + (uint32_t)k);
                    const float xr = (2 * unit01(pcg32(hk)) - 1) * a.radius, yr = (2 * unit01(pcg32(hk ^ 0x68bc21ebu)) - 1) * a.radius;
                    if (!(xr * xr + yr * yr > a.radius * a.radius)) { x = xr; y = yr; break; }
                }
                for (int c = 0; c < 3; c++) {
                    const float p = a.pos[c] + (x * a.t1[c] + y * a.t2[c]);
                    d[c] = a.dir[c]; pw[c] = a.power[c];
                    o[c] = p + kEps * d[c];                                          // Scene.cpp:535
                }
            }
            exhausted = base + n_idle >= a.count;
        }
        const bool live = my != kNoPhoton;
        if (!__any(live)) break;

        // ---- Scene::trace(hit, ray, 0, MIRO_TMAX) (Scene.cpp:539)
        const mr_hit h = trace_hit<true, false, false, VAR>(a.tp, make_float4(o[0], o[1], o[2], 0.0f), make_float4(d[0], d[1], d[2], 1e12f), 1e12f,
                                                            live, s_stack, tid, st);
        if (live) {
            state += 1u;                                                                 // ++depth (:538)
            const uint32_t depth = state & 255u;
            bool alive = false;
            if (h.prim != MR_MISS) {
                const float *mt = material_of(a.m, h.prim);
                const uint32_t e = a.first + my;
                const uint32_t hev = pcg32(a.hevent ^ e) + depth * 2u;
                const float rnd = unit01(pcg32(pcg32(hev)));
                const float p0 = avg3(mt), p1 = p0 + avg3(mt + 3), p2 = p1 + avg3(mt + 6);      // :551-553
                if (!(rnd > p2)) {
                    ChildGen<true> g;
                    g.mt = mt;
                    surface_point_od(a.m, o[0], o[1], o[2], d[0], d[1], d[2], h.t, h.prim, h.beta, h.gamma, g.P, g.N);
                    for (int c = 0; c < 3; c++) { g.d[c] = d[c]; g.w0[c] = 1.0f; }
                    g.Rs = 1.0f;
                    float org[3], nd[3], wgt[3];
                    if (rnd < p0) {                                                      // diffuse (:564-609)
                        bool go = true;
                        if (depth > 1u && ((state >> 8) & 255u) < a.max_depth) {      // (the second test always holds: at most one store per hit)
                            const uint32_t stores = (state >> 8) & 255u;
                            float4 *rec = a.slots + 3 * ((size_t)my * a.max_depth + stores);
                            rec[0] = make_float4(g.P[0], g.P[1], g.P[2], d[0]);
                            rec[1] = make_float4(d[1], d[2], pw[0], pw[1]);
                            rec[2] = make_float4(pw[2], __uint_as_float(e), __uint_as_float(depth), __uint_as_float((state >> 16) & 1u));
                            state += 1u << 8;
                        } else if (a.caustic) {
                            go = false;                                                  // :597-598
                        }
                        if (go) {
                            g.hray = pcg32(a.hdir ^ e) + depth * 4u;
                            g.make(3, org, nd, wgt);                                     // Ray::random: starts at P + epsilon * dir
                            const float inv = 1.0f / p0;
                            for (int c = 0; c < 3; c++) {
                                pw[c] = (mt[c] * pw[c]) * inv;                           // diffuseColor * power / prob[0] (:608)
                                d[c] = nd[c];
                                o[c] = org[c] + kEps * nd[c];                            // ... and tracePhoton offsets it again (:535)
                            }
                            alive = true;
                        }
                    } else if (rnd < p2 && !(!a.caustic && depth == 1u)) {               // mirror or transmit (:610-649)
                        ChildGen<false> s;
                        s.mt = mt;
                        for (int c = 0; c < 3; c++) { s.P[c] = g.P[c]; s.N[c] = g.N[c]; s.d[c] = d[c]; s.w0[c] = 1.0f; }
                        s.Rs = 1.0f;
                        int kind = 0;
                        if (!(rnd < p1)) {
                            bool emit[4];
                            g.plan(false, true, false, emit);                            // getReflectionCoefficient on miro_math.h
                            const float rnd2 = unit01(pcg32(pcg32(hev + 1u)));
                            kind = rnd2 < g.Rs ? 0 : 2;                                  // :637
                        }
                        s.make(kind, org, nd, wgt);
                        if (depth == 1u) state |= 1u << 16;
                        for (int c = 0; c < 3; c++) { d[c] = nd[c]; o[c] = g.P[c] + kEps * nd[c]; }      // tracePhoton(hit.P, dir, ...)
                        alive = true;
                    }
                }
            }
            if (alive && depth > a.max_depth) alive = false;                             // :532
            if (!alive) {
                a.words[my] = ((state >> 8) & 255u) | (depth << 8);
                my = kNoPhoton;
            }
        }
    }
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

template <int VAR>
mr_status launch_walk_t(const WalkArgs &a, hipStream_t stream) {
    auto kern = &photon_walk_kernel<VAR>;
    size_t lds = 0;
    unsigned grid = 1;
    mr_status st = stack_lds(kern, a.tp.stack_depth, kStackLdsShared, lds);
    // a resident grid: every wave keeps pulling emissions until the round is handed out
    if (st == MR_OK) st = resident_grid(kern, lds, ((unsigned long long)a.count + kTraceBlock - 1) / kTraceBlock, grid);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kTraceBlock), lds, stream, a);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace

mr_status launch_photon_round(const DeviceScene &ds, const PhotonWalkLight &lt, uint32_t seed, uint32_t caustic, uint32_t max_depth,
                              uint32_t first, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b, hipStream_t stream) {
    if (count == 0 || count > b.capacity) return fail(MR_ERR_INVALID, "photon round of %u emissions (buffers hold %u)", count, b.capacity);
    WalkArgs a;
    a.tp = scene_trace_params(ds);
    a.tp.n = count;
    a.m = mesh_of(ds);
    for (int c = 0; c < 3; c++) { a.pos[c] = lt.position[c]; a.dir[c] = lt.direction[c]; a.t1[c] = lt.t1[c]; a.t2[c] = lt.t2[c]; a.power[c] = lt.power[c]; }
    a.radius = lt.radius;
    a.hdir = pcg32(seed); a.hevent = pcg32(seed ^ kPhotonEventDomain); a.hdisc = pcg32(seed ^ kPhotonDiscDomain);
    a.caustic = caustic; a.max_depth = max_depth; a.first = first; a.count = count;
    a.slots = b.slots; a.words = b.words; a.next = b.next;
    MR_HIP_CHECK(hipMemsetAsync(b.next, 0, sizeof(unsigned), stream));
    // photons walk incoherently after their first bounce: the voting control flow of the default (exact) traversal
    mr_status st = (ds.n_planes || ds.n_spheres) ? launch_walk_t<kTraceVoteObj>(a, stream) : launch_walk_t<kTraceVote>(a, stream);
    if (st != MR_OK) return st;
    hipLaunchKernelGGL(photon_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, b.words, count, need, b.offsets, b.header);
    MR_HIP_CHECK(hipGetLastError());
    unsigned long long blocks = ((unsigned long long)count * max_depth + kBlock - 1) / kBlock;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(photon_compact_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, b.slots, b.words, b.offsets, count, max_depth,
                       b.header, b.compact);
    MR_HIP_CHECK(hipGetLastError());
    return MR_OK;
}

}  // namespace mr
