// mr_photon_trace.cpp -- host side of mr_trace_photons and mr_trace_photons_surface: Scene::tracePhotons /
// traceCausticPhotons for one DirectionalAreaLight (Scene.cpp:351-472).  The photons are walked on the device
// (mr_photon_walk.hip, or mr_photon_walk_surface.hip with the surface pass's colour and normal at every hit) in rounds of
// emissions; after each round the host reads one small header, copies the round's compacted records and pushes them
// through mr_photon_map_store, until the target is reached or max_emissions are spent; then scale_photon_power(1/emitted).
//
// The result does not depend on the round size: a round's header says how many of its emissions count (up to and including
// the one whose stores reach the target), and only their records -- in emission order -- are taken.
//
// Both entry points run trace_photons below; they differ in the round launcher they hand it (and in what they ask of the
// scene's texture table before).
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "mr_internal.h"

using namespace mr;

namespace {

constexpr float kPI = 3.1415926535897932384626433832795028841972f;   // Miro.h:10
constexpr uint32_t kRoundMin = 16384;
constexpr uint64_t kRoundRecords = 5ull << 20;                        // record slots per round (48 bytes each, twice)

struct Timing { double kernel_ms = 0, readback_ms = 0, store_ms = 0; };
thread_local Timing g_timing;

struct Buffers : PhotonRoundBuffers {
    ~Buffers() {
        (void)hipFree(slots); (void)hipFree(compact); (void)hipFree(words); (void)hipFree(offsets); (void)hipFree(next); (void)hipFree(header);
    }
};

mr_status allocate(Buffers &b, uint32_t capacity, uint32_t max_depth) {
    const size_t rec = (size_t)capacity * max_depth * 3 * sizeof(float4);
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b.slots), rec));
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b.compact), rec));
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b.words), (size_t)capacity * sizeof(uint32_t)));
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b.offsets), (size_t)capacity * sizeof(uint32_t)));
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b.next), sizeof(unsigned)));
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&b.header), sizeof(PhotonRoundHeader)));
    b.capacity = capacity;
    return MR_OK;
}

// Where a round's compacted records go -- the one thing mr_trace_photons_resident does differently.
//   begin(desc, max_depth)                 before the first round
//   copy(compact, n, at, stream)           enqueue the copy of the round's n records, the call's records [at, at + n)
//   store(map)                             after that copy and the stream's synchronisation: hand them to the map
//   finish(map, emitted, stored, stream)   after the last round
// HostStore: to the host and through mr_photon_map_store, then scale_photon_power(1 / emitted); the caller balances.
struct HostStore {
    static constexpr bool kHost = true;
    std::vector<mr_photon_record> recs;
    std::vector<float> power, pos, dir;
    mr_status begin(const mr_photon_trace_desc *, uint32_t) { return MR_OK; }
    mr_status copy(const float4 *compact, uint64_t n, uint64_t, hipStream_t stream) {
        recs.resize(n);
        if (n) MR_HIP_CHECK(hipMemcpyAsync(recs.data(), compact, n * sizeof(mr_photon_record), hipMemcpyDeviceToHost, stream));
        return MR_OK;
    }
    mr_status store(mr_photon_map *map) {
        power.resize(3 * recs.size()); pos.resize(3 * recs.size()); dir.resize(3 * recs.size());
        for (size_t i = 0; i < recs.size(); i++)
            for (int c = 0; c < 3; c++) { power[3 * i + c] = recs[i].power[c]; pos[3 * i + c] = recs[i].pos[c]; dir[3 * i + c] = recs[i].dir[c]; }
        for (size_t at = 0; at < recs.size(); at += 1u << 30) {       // mr_photon_map_store counts in 32 bits
            const size_t n = recs.size() - at < (1u << 30) ? recs.size() - at : (1u << 30);
            mr_status st = mr_photon_map_store(map, (uint32_t)n, power.data() + 3 * at, pos.data() + 3 * at, dir.data() + 3 * at);
            if (st != MR_OK) return st;
        }
        return MR_OK;
    }
    mr_status finish(mr_photon_map *map, uint64_t emitted, uint64_t, hipStream_t) {
        return emitted ? mr_photon_map_scale(map, 1.0f / (float)emitted) : MR_OK;      // Scene.cpp:402
    }
};
// DeviceAppend: device to device onto a library-owned buffer of target + max_depth records (the last emission's records all
// count), then mr_photon_map_build_device with the same scale; the map ends balanced and resident.
struct DeviceAppend {
    static constexpr bool kHost = false;
    mr_photon_record *d_all = nullptr;
    uint64_t capacity = 0;
    mr_photon_build_result *build = nullptr;
    ~DeviceAppend() { (void)hipFree(d_all); }
    mr_status begin(const mr_photon_trace_desc *desc, uint32_t max_depth) {
        capacity = (uint64_t)desc->target + max_depth;
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_all), capacity * sizeof(mr_photon_record)));
        return MR_OK;
    }
    mr_status copy(const float4 *compact, uint64_t n, uint64_t at, hipStream_t stream) {
        if (at + n > capacity) return fail(MR_ERR_HIP, "mr_trace_photons_resident: %llu records overflow the buffer of %llu", (unsigned long long)(at + n), (unsigned long long)capacity);
        if (n) MR_HIP_CHECK(hipMemcpyAsync(d_all + at, compact, n * sizeof(mr_photon_record), hipMemcpyDeviceToDevice, stream));
        return MR_OK;
    }
    mr_status store(mr_photon_map *) { return MR_OK; }
    mr_status finish(mr_photon_map *map, uint64_t emitted, uint64_t stored, hipStream_t stream) {
        return mr_photon_map_build_device(map, d_all, stored, emitted ? 1.0f / (float)emitted : 1.0f, build, stream);
    }
};

// launch(light, max_depth, first, count, need, buffers): one round's walk and bookkeeping kernels on `stream`
template <typename Policy, typename Launch>
mr_status trace_photons(const char *who, bool surface, mr_scene *s, mr_photon_map *map, const mr_photon_trace_desc *desc,
                        mr_photon_trace_result *result, mr_photon_record *d_records, uint64_t records_capacity, hipStream_t stream, Policy &&policy,
                        Launch &&launch) {
    if (!s || !map || !desc) return fail(MR_ERR_INVALID, "%s: NULL scene, map or desc", who);
    if (desc->max_emissions == 0) return fail(MR_ERR_INVALID, "%s: max_emissions is 0 (the hard stop is required)", who);
    const mr_disc_light &lt = desc->light;
    if (!(lt.radius > 0.0f) || !std::isfinite(lt.radius)) return fail(MR_ERR_INVALID, "%s: the light's radius must be positive", who);
    if (lt.normal[0] == 0.0f && lt.normal[1] == 0.0f && lt.normal[2] == 0.0f) return fail(MR_ERR_INVALID, "%s: the light's normal is zero", who);
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(lt.normal[c]) || !std::isfinite(lt.position[c])) return fail(MR_ERR_INVALID, "%s: the light's position and normal must be finite", who);
    if (desc->max_depth > kPhotonMaxDepth) return fail(MR_ERR_INVALID, "%s: max_depth is at most %u", who, kPhotonMaxDepth);
    for (int k = 0; k < 6; k++)
        if (desc->reserved[k] != 0) return fail(MR_ERR_INVALID, "mr_photon_trace_desc.reserved must be 0");
    if (reinterpret_cast<uintptr_t>(d_records) & 3) return fail(MR_ERR_INVALID, "%s: d_records must be 4-byte aligned", who);
    if (s->device != photon_map_device(map)) return fail(MR_ERR_INVALID, "%s: scene on device %d, photon map on device %d", who, s->device, photon_map_device(map));
    if (!s->built) return fail(MR_ERR_STATE, "mr_bvh_build has not been called on this scene");
    if (!s->on_device) return fail(MR_ERR_STATE, "scene was built host_only: nothing is resident on a device and there is no CPU fallback");
    if (!surface && !s->tex.blob.empty())    // the roulette reads diffuse2D (Scene.cpp:545-551); the plain walk has no texture lookup
        return fail(MR_ERR_STATE, "mr_trace_photons: the scene has a texture table (mr_scene_set_textures) and the plain photon walk's roulette "
                                  "has no texture lookup; call mr_trace_photons_surface, whose walk looks textures up, or trace photons "
                                  "before setting textures, or clear them (n_textures = 0)");
    if (photon_map_balanced(map)) return fail(MR_ERR_STATE, "photon map is immutable after mr_photon_map_balance");
    if (!policy.kHost && photon_map_stored(map) > 0)
        return fail(MR_ERR_STATE, "%s: the map already holds %u photons; this call builds ONE empty map (trace several lights into one map with "
                                  "mr_trace_photons and mr_photon_map_balance)", who, photon_map_stored(map));
    g_timing = Timing();

    const uint32_t max_depth = desc->max_depth ? desc->max_depth : 5u;          // TRACE_DEPTH_PHOTONS (Miro.h:14)
    PhotonWalkLight wl;
    {
        tangents_of(lt.normal, wl.t1, wl.t2);                                    // getTangents (Utility.h:25-31)
        float k = kPI * lt.radius * lt.radius;                                   // Scene.cpp:384
        if (desc->caustic) k = k / 10.f;                                         // :446
        for (int c = 0; c < 3; c++) {
            wl.position[c] = lt.position[c]; wl.direction[c] = lt.normal[c];
            wl.power[c] = (lt.color[c] * lt.wattage) * k;
        }
        wl.radius = lt.radius;
    }

    mr_photon_trace_result res = {0, 0, 0, 0};
    if (desc->target > 0 || !policy.kHost) MR_HIP_CHECK(hipSetDevice(s->device));
    if (desc->target > 0) {
        uint64_t limit = kRoundRecords / max_depth;
        if (limit > (1u << 20)) limit = 1u << 20;
        // the first round: one emission per wanted photon (a photon stores less than once per emission in most rooms)
        uint64_t round = desc->round_emissions ? desc->round_emissions : (desc->target > kRoundMin ? desc->target : kRoundMin);
        if (round > limit) round = limit;
        if (round > desc->max_emissions) round = desc->max_emissions;
        Buffers b;
        mr_status st = allocate(b, (uint32_t)round, max_depth);
        if (st != MR_OK) return st;
        st = policy.begin(desc, max_depth);
        if (st != MR_OK) return st;
        bool reached = false;
        while (!reached && res.emitted < desc->max_emissions) {
            uint64_t count = round;
            if (!desc->round_emissions && res.rounds > 0) {
                // later rounds from the measured yield, with an eighth to spare; none stored yet: the largest round
                count = res.stored ? (uint64_t)((double)(desc->target - res.stored) * (double)res.emitted / (double)res.stored * 1.125) + 1024 : b.capacity;
                if (count < kRoundMin) count = kRoundMin;
            }
            if (count > b.capacity) count = b.capacity;
            if (count > desc->max_emissions - res.emitted) count = desc->max_emissions - res.emitted;
            auto t0 = std::chrono::steady_clock::now();
            st = launch(wl, max_depth, (uint32_t)res.emitted, (uint32_t)count, (unsigned long long)(desc->target - res.stored), b);
            if (st != MR_OK) return st;
            PhotonRoundHeader hdr;
            MR_HIP_CHECK(hipMemcpyAsync(&hdr, b.header, sizeof(hdr), hipMemcpyDeviceToHost, stream));
            MR_HIP_CHECK(hipStreamSynchronize(stream));
            g_timing.kernel_ms += ms_since(t0);
            if (hdr.emitted > count || hdr.stored > (uint64_t)count * max_depth)
                return fail(MR_ERR_HIP, "%s: inconsistent round header (%u emissions of %llu)", who, hdr.emitted, (unsigned long long)count);

            t0 = std::chrono::steady_clock::now();
            st = policy.copy(b.compact, hdr.stored, res.stored, stream);
            if (st != MR_OK) return st;
            if (d_records && res.stored < records_capacity && hdr.stored) {
                const uint64_t room = records_capacity - res.stored, n = hdr.stored < room ? hdr.stored : room;
                MR_HIP_CHECK(hipMemcpyAsync(d_records + res.stored, b.compact, n * sizeof(mr_photon_record), hipMemcpyDeviceToDevice, stream));
            }
            MR_HIP_CHECK(hipStreamSynchronize(stream));
            if (policy.kHost) g_timing.readback_ms += ms_since(t0);

            t0 = std::chrono::steady_clock::now();
            st = policy.store(map);
            if (st != MR_OK) return st;
            if (policy.kHost) g_timing.store_ms += ms_since(t0);

            res.emitted += hdr.emitted; res.stored += hdr.stored; res.segments += hdr.segments; res.rounds++;
            reached = hdr.reached != 0;
        }
    }
    if (desc->target > 0 || !policy.kHost) {
        mr_status st2 = policy.finish(map, res.emitted, res.stored, stream);
        if (st2 != MR_OK) return st2;
    }
    if (result) *result = res;
    return MR_OK;
}

// the two walks behind one policy
template <typename Policy>
mr_status trace_plain(const char *who, mr_scene *s, mr_photon_map *map, const mr_photon_trace_desc *desc, mr_photon_trace_result *result,
                      mr_photon_record *d_records, uint64_t records_capacity, hipStream_t stream, Policy &&policy) {
    return trace_photons(who, false, s, map, desc, result, d_records, records_capacity, stream, policy,
                         [&](const PhotonWalkLight &wl, uint32_t max_depth, uint32_t first, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b) {
                             return launch_photon_round(s->dev, wl, desc->seed, desc->caustic ? 1u : 0u, max_depth, first, count, need, b, stream);
                         });
}

template <typename Policy>
mr_status trace_surface(const char *who, mr_scene *s, mr_photon_map *map, const mr_photon_trace_desc *desc, mr_photon_trace_result *result,
                        mr_photon_record *d_records, uint64_t records_capacity, hipStream_t stream, Policy &&policy) {
    bool have_table = false;                 // the table is uploaded / refreshed by the first round, as mr_hit_surface does it
    TexParams tex;
    return trace_photons(who, true, s, map, desc, result, d_records, records_capacity, stream, policy,
                         [&](const PhotonWalkLight &wl, uint32_t max_depth, uint32_t first, uint32_t count, unsigned long long need, const PhotonRoundBuffers &b) {
                             if (!have_table) {
                                 tex.recs = nullptr; tex.texels = nullptr; tex.mat_tex = nullptr; tex.texcoords = s->dev.texcoords; tex.ti = s->dev.ti;
                                 mr_status st = s->tex.blob.empty() ? MR_OK : texture_params(s, stream, tex);
                                 if (st != MR_OK) return st;
                                 have_table = true;
                             }
                             return launch_photon_round_surface(s->dev, tex, wl, desc->seed, desc->caustic ? 1u : 0u, max_depth, first, count, need, b, stream);
                         });
}

}  // namespace

extern "C" {

mr_status mr_trace_photons(mr_scene *s, mr_photon_map *map, const mr_photon_trace_desc *desc, mr_photon_trace_result *result,
                           mr_photon_record *d_records, uint64_t records_capacity, void *stream_) {
    return trace_plain("mr_trace_photons", s, map, desc, result, d_records, records_capacity, static_cast<hipStream_t>(stream_), HostStore());
}

mr_status mr_trace_photons_surface(mr_scene *s, mr_photon_map *map, const mr_photon_trace_desc *desc, mr_photon_trace_result *result,
                                   mr_photon_record *d_records, uint64_t records_capacity, void *stream_) {
    return trace_surface("mr_trace_photons_surface", s, map, desc, result, d_records, records_capacity, static_cast<hipStream_t>(stream_), HostStore());
}

mr_status mr_trace_photons_resident(mr_scene *s, mr_photon_map *map, const mr_photon_trace_desc *desc, uint32_t surface,
                                    mr_photon_trace_result *result, mr_photon_build_result *build, mr_photon_record *d_records,
                                    uint64_t records_capacity, void *stream_) {
    if (build) *build = mr_photon_build_result();
    if (surface > 1) return fail(MR_ERR_INVALID, "mr_trace_photons_resident: surface is 0 (the walk of mr_trace_photons) or 1 (of mr_trace_photons_surface)");
    DeviceAppend policy;
    policy.build = build;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return surface ? trace_surface("mr_trace_photons_resident", s, map, desc, result, d_records, records_capacity, stream, policy)
                   : trace_plain("mr_trace_photons_resident", s, map, desc, result, d_records, records_capacity, stream, policy);
}

mr_status mr_trace_photons_timing(double *kernel_ms, double *readback_ms, double *store_ms) {
    if (kernel_ms) *kernel_ms = g_timing.kernel_ms;
    if (readback_ms) *readback_ms = g_timing.readback_ms;
    if (store_ms) *store_ms = g_timing.store_ms;
    return MR_OK;
}

}  // extern "C"
