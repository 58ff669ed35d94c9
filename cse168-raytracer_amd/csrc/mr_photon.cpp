// mr_photon.cpp -- host side of the photon map (config 5 of BASELINE.json): the reference's Photon_map
// (PhotonMap.h:42-105; Jensen's kd-tree as vendored and modified by the reference) behind the C ABI:
//   mr_photon_map_store    Photon_map::store              PhotonMap.cpp:255-289  (direction quantised to 2 bytes)
//   mr_photon_map_scale    Photon_map::scale_photon_power PhotonMap.cpp:298-306
//   mr_photon_map_balance  Photon_map::balance            PhotonMap.cpp:314-359,409-476 (left-balanced kd-tree in
//                          heap order; split axis = longest extent of the running bounding box) + upload
//   mr_irradiance_estimate Photon_map::irradiance_estimate PhotonMap.cpp:81-145 -> csrc/mr_photon.hip
// Own structure: photons live in SoA vectors; the balance works on an index permutation with std::nth_element
// under a total order (coordinate, then storage index), which yields the unique left-balanced tree; the device
// gets three float4 planes in heap order (position+axis, de-quantised direction, power).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "mr_internal.h"
#include "mr_photon_tree.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

using namespace mr;

namespace {

struct DirTables {
    float costheta[256], sintheta[256], cosphi[256], sinphi[256];
    DirTables() {
        for (int i = 0; i < 256; i++) {                            // PhotonMap.cpp:47-53
            const double angle = double(i) * (1.0 / 256.0) * M_PI;
            costheta[i] = (float)cos(angle);
            sintheta[i] = (float)sin(angle);
            cosphi[i] = (float)cos(2.0 * angle);
            sinphi[i] = (float)sin(2.0 * angle);
        }
    }
};
const DirTables &tables() { static DirTables t; return t; }

// the two direction bytes of Photon_map::store (PhotonMap.cpp:268-283): the one place they are computed, for
// mr_photon_map_store and for the photons mr_photon_map_build_device defers to the host
inline void direction_bytes(float dx, float dy, float dz, uint8_t &theta_out, uint8_t &phi_out) {
    theta_out = theta_byte(int(acos(dz) * (256.0 / M_PI)));
    phi_out = phi_byte(int(atan2(dy, dx) * (256.0 / (2.0 * M_PI))));
}

}  // namespace

struct mr_photon_map {
    int32_t device = 0;
    uint32_t max_photons = 0;
    // storage order (1-based in the reference; 0-based here)
    std::vector<float> pos, power;           // xyz triples
    std::vector<uint8_t> theta, phi;
    uint32_t prev_scale = 0;
    float bbox_min[3] = {1e8f, 1e8f, 1e8f}, bbox_max[3] = {-1e8f, -1e8f, -1e8f};
    // heap order after balance: heap[i] = storage index of the photon at kd-tree node i+1, with its split axis
    std::vector<uint32_t> heap;
    std::vector<int16_t> plane;
    bool balanced = false, on_device = false;
    PhotonMapDev dev;
    unsigned long long *d_stats = nullptr;   // work counters of the estimates (mr_photon_map_count_stats), else NULL
    std::atomic<uint32_t> next_counter{0};   // which of dev.work_counters the next estimate launch takes
    // a map built by mr_photon_map_build_device lives on the device alone: the vectors above stay empty, dev holds the planes and
    // d_dir the quantised directions in heap order (theta, phi per photon), which mr_photon_map_export reads back
    bool device_built = false;
    uint32_t device_stored = 0;
    uint8_t *d_dir = nullptr;
    uint32_t count() const { return device_built ? device_stored : (uint32_t)theta.size(); }
};

namespace {

struct Balancer {
    mr_photon_map &m;
    std::vector<uint32_t> org;      // permutation being partitioned, 1-based segment positions
    float bmin[3], bmax[3];

    explicit Balancer(mr_photon_map &pm) : m(pm) {
        org.resize(m.count() + 1);
        for (uint32_t p = 1; p < org.size(); p++) org[p] = p - 1;      // storage index p-1 for p >= 1 (slot 0 unused)
        memcpy(bmin, m.bbox_min, sizeof(bmin));
        memcpy(bmax, m.bbox_max, sizeof(bmax));
    }

    void segment(int index, int start, int end) {
        const int median = left_balanced_median(start, end);
        const int axis = split_axis(bmin, bmax);
        const float *pos = m.pos.data();
        std::nth_element(org.begin() + start, org.begin() + median, org.begin() + end + 1,
                         [pos, axis](uint32_t a, uint32_t b) {
                             const float pa = pos[3 * (size_t)a + axis], pb = pos[3 * (size_t)b + axis];
                             return pa != pb ? pa < pb : a < b;
                         });
        m.heap[index - 1] = org[median];
        m.plane[index - 1] = (int16_t)axis;
        const float split = pos[3 * (size_t)org[median] + axis];
        if (median > start) {
            if (start < median - 1) {
                const float keep = bmax[axis];
                bmax[axis] = split;
                segment(2 * index, start, median - 1);
                bmax[axis] = keep;
            } else {
                m.heap[2 * index - 1] = org[start];
            }
        }
        if (median < end) {
            if (median + 1 < end) {
                const float keep = bmin[axis];
                bmin[axis] = split;
                segment(2 * index + 1, median + 1, end);
                bmin[axis] = keep;
            } else {
                m.heap[2 * index] = org[end];
            }
        }
    }
};

void release(mr_photon_map *m) {
    (void)hipFree(m->dev.rec); (void)hipFree(m->dev.power); (void)hipFree(m->dev.boxes); (void)hipFree(m->dev.work_counters); (void)hipFree(m->d_stats); (void)hipFree(m->d_dir);
    m->dev = PhotonMapDev();
    m->d_stats = nullptr;
    m->d_dir = nullptr;
    m->on_device = false;
}

// The device planes of a balanced map of n photons, from their allocation to the end of the call that fills them: commit()
// swaps them into the map; the destructor frees what the holder then holds -- the new planes of a call that failed, or the
// planes the map had before.  The hand-out counters are allocated once per map, by the first holder that finds none.
struct Planes {
    PhotonMapDev dev;
    uint8_t *d_dir = nullptr;
    size_t box_records = 0;                   // float4 in dev.boxes
    ~Planes() { (void)hipFree(dev.rec); (void)hipFree(dev.power); (void)hipFree(dev.boxes); (void)hipFree(dev.work_counters); (void)hipFree(d_dir); }
    mr_status allocate(const mr_photon_map *m, uint32_t n, bool with_dir) {
        box_records = 4 * std::max<size_t>(photon_map_layout(dev, n), 1);
        const size_t bytes = ((size_t)n + 1) * sizeof(float4);      // 1-based, slot 0 unused
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&dev.rec), 2 * bytes));
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&dev.power), bytes));
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&dev.boxes), box_records * sizeof(float4)));
        if (with_dir) MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d_dir), std::max<size_t>(2 * (size_t)n, 4)));
        if (!m->dev.work_counters) {
            MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&dev.work_counters), kPhotonWorkCounters * sizeof(unsigned)));
            MR_HIP_CHECK(hipMemset(dev.work_counters, 0, kPhotonWorkCounters * sizeof(unsigned)));
        }
        return MR_OK;
    }
    void commit(mr_photon_map *m) {
        if (m->dev.work_counters) std::swap(dev.work_counters, m->dev.work_counters);      // the map keeps its own
        std::swap(dev, m->dev);
        std::swap(d_dir, m->d_dir);
        m->on_device = true;
    }
};

// one k-NN estimate on a resident map: the launch takes the next of the map's hand-out counters and the map's statistics
mr_status estimate(mr_photon_map *m, const float *d_pos, const float *d_normal, unsigned long long n_queries, float max_dist, uint32_t nphotons,
                   float *d_irrad, int32_t *d_found, float *d_r2, hipStream_t stream) {
    unsigned *counter = m->dev.work_counters + (m->next_counter.fetch_add(1) % kPhotonWorkCounters);
    return launch_irradiance(m->dev, counter, d_pos, d_normal, n_queries, max_dist, nphotons, d_irrad, d_found, d_r2, m->d_stats, stream);
}

// What mr_final_gather and mr_gather_level do between their own checks and their own accumulate step.  d_scratch: laid out by
// gather_scratch (mr_internal.h); d_irr[i]: where map i's estimate is, NULL without that map.
mr_status gather_estimates(mr_scene *s, mr_photon_map *const maps[2], const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                           uint64_t n, float max_dist, uint32_t nphotons, float *d_scratch, uint64_t *d_counts, hipStream_t stream,
                           float *d_irr[2]) {
    MR_HIP_CHECK(hipSetDevice(s->device));
    const GatherScratch sc = gather_scratch(d_scratch, n, maps[0] != nullptr, maps[1] != nullptr);
    mr_status st = launch_gather_level_queries(s->dev, d_rays, d_hits, d_normal, n, sc.pos, sc.nrm, reinterpret_cast<unsigned long long *>(d_counts), stream);
    if (st != MR_OK) return st;
    for (int i = 0; i < 2; i++) {
        d_irr[i] = sc.irr[i];
        if (!maps[i]) continue;
        st = estimate(maps[i], sc.pos, sc.nrm, n, max_dist, nphotons, d_irr[i], nullptr, nullptr, stream);
        if (st != MR_OK) return st;
    }
    return MR_OK;
}

}  // namespace

namespace mr {
int32_t photon_map_device(const mr_photon_map *m) { return m->device; }
bool photon_map_balanced(const mr_photon_map *m) { return m->balanced; }
uint32_t photon_map_stored(const mr_photon_map *m) { return m->count(); }
bool photon_map_resident(const mr_photon_map *m) { return m->balanced && m->on_device; }
mr_status photon_map_estimate_queued(mr_photon_map *m, const float *d_pos, const float *d_normal, const unsigned long long *d_n,
                                     unsigned long long bound, float max_dist, uint32_t nphotons, float *d_irrad, hipStream_t stream) {
    unsigned *counter = m->dev.work_counters + (m->next_counter.fetch_add(1) % kPhotonWorkCounters);
    return launch_irradiance_queued(m->dev, counter, d_pos, d_normal, d_n, bound, max_dist, nphotons, d_irrad, m->d_stats, stream);
}
}  // namespace mr

extern "C" {

mr_status mr_photon_map_create(int32_t device, uint32_t max_photons, mr_photon_map **out) {
    if (!out) return fail(MR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (device < 0) return fail(MR_ERR_INVALID, "device %d is negative", device);
    mr_photon_map *m = new (std::nothrow) mr_photon_map();
    if (!m) return fail(MR_ERR_NOMEM, "out of host memory");
    m->device = device;
    m->max_photons = max_photons;
    *out = m;
    return MR_OK;
}

mr_status mr_photon_map_destroy(mr_photon_map *m) {
    if (!m) return MR_OK;
    if (m->on_device) { (void)hipSetDevice(m->device); release(m); }
    delete m;
    return MR_OK;
}

mr_status mr_photon_map_store(mr_photon_map *m, uint32_t n, const float *power, const float *pos, const float *dir) {
    if (!m || (n && (!power || !pos || !dir))) return fail(MR_ERR_INVALID, "NULL argument");
    if (m->balanced) return fail(MR_ERR_STATE, "photon map is immutable after mr_photon_map_balance");
    for (uint32_t i = 0; i < n; i++) {
        if (m->count() >= m->max_photons) break;                    // PhotonMap.cpp:260-261: silently full
        for (int k = 0; k < 3; k++) {
            const float p = pos[3 * (size_t)i + k];
            m->pos.push_back(p);
            if (p < m->bbox_min[k]) m->bbox_min[k] = p;
            if (p > m->bbox_max[k]) m->bbox_max[k] = p;
            m->power.push_back(power[3 * (size_t)i + k]);
        }
        uint8_t theta, phi;
        direction_bytes(dir[3 * (size_t)i], dir[3 * (size_t)i + 1], dir[3 * (size_t)i + 2], theta, phi);
        m->theta.push_back(theta);
        m->phi.push_back(phi);
    }
    return MR_OK;
}

mr_status mr_photon_map_scale(mr_photon_map *m, float scale) {
    if (!m) return fail(MR_ERR_INVALID, "photon map is NULL");
    if (m->balanced) return fail(MR_ERR_STATE, "photon map is immutable after mr_photon_map_balance");
    // the reference's loop runs from prev_scale (1-based, initially 1) to stored: it re-scales the last photon of
    // the previous batch (PhotonMap.cpp:301-305); kept
    const uint32_t from = m->prev_scale == 0 ? 0 : m->prev_scale - 1;
    for (uint32_t i = from; i < m->count(); i++)
        for (int k = 0; k < 3; k++) m->power[3 * (size_t)i + k] *= scale;
    m->prev_scale = m->count();
    return MR_OK;
}

mr_status mr_photon_map_balance(mr_photon_map *m, uint32_t host_only) {
    if (!m) return fail(MR_ERR_INVALID, "photon map is NULL");
    if (m->device_built) return MR_OK;       // mr_photon_map_build_device left it balanced and resident
    const uint32_t n = m->count();
    m->heap.assign(n, 0);
    m->plane.assign(n, 0);
    if (n > 1) {
        Balancer b(*m);
        b.segment(1, 1, (int)n);
    } else if (n == 1) {
        m->heap[0] = 0;
    }
    m->balanced = true;
    if (host_only) return MR_OK;
    mr_status st = select_device(m->device);
    if (st != MR_OK) return st;
    if (m->on_device) release(m);
    Planes planes;                            // the map takes them once every upload has succeeded
    st = planes.allocate(m, n, false);
    if (st != MR_OK) return st;
    // heap-ordered planes, 1-based (slot 0 unused) so that children of i are 2i, 2i+1
    std::vector<float4> a(n + 1), d(n + 1), p(n + 1);
    const DirTables &t = tables();
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t s = m->heap[i];
        float w;
        const int32_t pl = m->plane[i];
        memcpy(&w, &pl, 4);
        a[i + 1] = make_float4(m->pos[3 * (size_t)s], m->pos[3 * (size_t)s + 1], m->pos[3 * (size_t)s + 2], w);
        const uint8_t th = m->theta[s], ph = m->phi[s];
        d[i + 1] = make_float4(t.sintheta[th] * t.cosphi[ph], t.sintheta[th] * t.sinphi[ph], t.costheta[th], 0.0f);   // :66-71
        p[i + 1] = make_float4(m->power[3 * (size_t)s], m->power[3 * (size_t)s + 1], m->power[3 * (size_t)s + 2], 0.0f);
    }
    a[0] = d[0] = p[0] = make_float4(0, 0, 0, 0);
    const size_t bytes = (size_t)(n + 1) * sizeof(float4);
    std::vector<float4> rec(2 * (size_t)(n + 1));
    for (uint32_t i = 0; i <= n; i++) { rec[2 * (size_t)i] = a[i]; rec[2 * (size_t)i + 1] = d[i]; }
    MR_HIP_CHECK(hipMemcpy(planes.dev.rec, rec.data(), 2 * bytes, hipMemcpyHostToDevice));
    MR_HIP_CHECK(hipMemcpy(planes.dev.power, p.data(), bytes, hipMemcpyHostToDevice));
    // block boxes: bounds of every subtree (bottom-up over the heap), then per block root its own six levels and its subtree
    {
        const float inf = INFINITY;
        std::vector<float> slo(3 * (size_t)(n + 1), inf), shi(3 * (size_t)(n + 1), -inf);
        for (uint32_t j = n; j >= 1; j--) {
            const float pj[3] = {a[j].x, a[j].y, a[j].z};
            for (int c = 0; c < 3; c++) {
                float lo = pj[c], hi = pj[c];
                for (uint32_t ch = 2 * j; ch <= 2 * j + 1 && ch <= n; ch++) {
                    lo = std::min(lo, slo[3 * (size_t)ch + c]);
                    hi = std::max(hi, shi[3 * (size_t)ch + c]);
                }
                slo[3 * (size_t)j + c] = lo; shi[3 * (size_t)j + c] = hi;
            }
        }
        const int layers = planes.dev.layers;
        std::vector<float4> boxes(planes.box_records, make_float4(inf, inf, inf, 0.f));
        for (size_t i = 0; i < boxes.size(); i += 2) boxes[i + 1] = make_float4(-inf, -inf, -inf, 0.f);
        uint64_t first = 1;
        for (int L = 0; L < layers; L++, first <<= 6) {
            for (uint64_t r = first; r < 2 * first && r <= n; r++) {
                float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
                for (int l = 0; l < 6; l++)
                    for (uint64_t o = 0; o < (1ull << l); o++) {
                        const uint64_t j = (r << l) + o;
                        if (j > n) break;
                        const float pj[3] = {a[j].x, a[j].y, a[j].z};
                        for (int c = 0; c < 3; c++) { lo[c] = std::min(lo[c], pj[c]); hi[c] = std::max(hi[c], pj[c]); }
                    }
                float4 *b = &boxes[4 * ((size_t)planes.dev.layer_base[L] + (size_t)(r - first))];
                b[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
                b[1] = make_float4(hi[0], hi[1], hi[2], 0.f);
                b[2] = make_float4(slo[3 * r], slo[3 * r + 1], slo[3 * r + 2], 0.f);
                b[3] = make_float4(shi[3 * r], shi[3 * r + 1], shi[3 * r + 2], 0.f);
            }
        }
        MR_HIP_CHECK(hipMemcpy(planes.dev.boxes, boxes.data(), boxes.size() * sizeof(float4), hipMemcpyHostToDevice));
    }
    planes.commit(m);
    return MR_OK;
}

mr_status mr_photon_map_build_device(mr_photon_map *m, const mr_photon_record *d_records, uint64_t n, float scale,
                                     mr_photon_build_result *result, void *stream_v) {
    if (result) *result = mr_photon_build_result();
    if (!m) return fail(MR_ERR_INVALID, "mr_photon_map_build_device: photon map is NULL");
    if (n && !d_records) return fail(MR_ERR_INVALID, "mr_photon_map_build_device: records is NULL with n = %llu", (unsigned long long)n);
    if (reinterpret_cast<uintptr_t>(d_records) & 3) return fail(MR_ERR_INVALID, "mr_photon_map_build_device: records must be 4-byte aligned");
    if (n > (1ull << 24))
        return fail(MR_ERR_INVALID, "mr_photon_map_build_device: n = %llu is above 2^24; store larger maps through the host path "
                                    "(mr_photon_map_store, mr_photon_map_scale, mr_photon_map_balance)", (unsigned long long)n);
    if (m->balanced) return fail(MR_ERR_STATE, "photon map is immutable after mr_photon_map_balance");
    if (m->count() > 0) return fail(MR_ERR_STATE, "mr_photon_map_build_device: the map already holds %u photons; it builds an empty map", m->count());
    mr_status st = select_device(m->device);
    if (st != MR_OK) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const uint32_t taken = (uint32_t)(n < m->max_photons ? n : m->max_photons);       // PhotonMap.cpp:260-261: silently full
    mr_photon_build_result res = mr_photon_build_result();
    res.stored = taken; res.dropped = n - taken;

    struct Work {                                   // the workspace
        PhotonBuildWork *w = nullptr;
        ~Work() { photon_build_end(w); }
    } work;
    const DirTables &t = tables();
    static_assert(sizeof(DirTables) == 1024 * sizeof(float), "the four tables travel as one block");
    st = photon_build_begin(taken, t.costheta, &work.w, stream);
    if (st != MR_OK) return st;

    // store: powers, box, direction bytes (the host's for the deferred photons), the non-finite flag
    auto t0 = std::chrono::steady_clock::now();
    PhotonBuildStatus status;
    float lo[3], hi[3];
    st = launch_photon_build_store(work.w, d_records, scale, &status, lo, hi, stream);
    if (st != MR_OK) return st;
    if (status.nonfinite) return fail(MR_ERR_INVALID, "mr_photon_map_build_device: a photon position is not finite; the map is left empty");
    if (status.deferred > taken) return fail(MR_ERR_HIP, "mr_photon_map_build_device: inconsistent deferred count %u of %u", status.deferred, taken);
    if (status.deferred) {
        std::vector<float4> list(status.deferred);
        float4 *d_list = photon_build_deferred(work.w);
        MR_HIP_CHECK(hipMemcpyAsync(list.data(), d_list, list.size() * sizeof(float4), hipMemcpyDeviceToHost, stream));
        MR_HIP_CHECK(hipStreamSynchronize(stream));
        for (float4 &d : list) {
            uint8_t theta, phi;
            direction_bytes(d.y, d.z, d.w, theta, phi);
            const uint32_t b = (uint32_t)theta | ((uint32_t)phi << 8);
            memcpy(&d.y, &b, 4);
        }
        MR_HIP_CHECK(hipMemcpyAsync(d_list, list.data(), list.size() * sizeof(float4), hipMemcpyHostToDevice, stream));
        st = launch_photon_build_fix(work.w, status.deferred, stream);
        if (st != MR_OK) return st;
        MR_HIP_CHECK(hipStreamSynchronize(stream));                 // `list` leaves scope
    }
    res.deferred = status.deferred;
    res.store_ms = ms_since(t0);

    // balance: three sorted lists, then one heap level per step
    t0 = std::chrono::steady_clock::now();
    st = launch_photon_build_tree(work.w, stream);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipStreamSynchronize(stream));
    res.balance_ms = ms_since(t0);

    // pack: the planes in heap order and the block boxes, laid out as mr_photon_map_balance lays them out
    t0 = std::chrono::steady_clock::now();
    Planes planes;                                  // the map takes them once the build has succeeded
    st = planes.allocate(m, taken, true);
    if (st != MR_OK) return st;
    st = launch_photon_build_pack(work.w, planes.dev, planes.d_dir, stream);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipStreamSynchronize(stream));
    res.pack_ms = ms_since(t0);

    planes.commit(m);
    memcpy(m->bbox_min, lo, sizeof(lo));
    memcpy(m->bbox_max, hi, sizeof(hi));
    m->prev_scale = taken;
    m->device_built = true;
    m->device_stored = taken;
    m->balanced = true;
    if (result) *result = res;
    return MR_OK;
}

mr_status mr_photon_map_count(const mr_photon_map *m, uint32_t *stored) {
    if (!m || !stored) return fail(MR_ERR_INVALID, "NULL argument");
    *stored = m->count();
    return MR_OK;
}

mr_status mr_photon_map_export(const mr_photon_map *m, float *pos, int32_t *plane, uint8_t *theta_phi, float *power) {
    if (!m) return fail(MR_ERR_INVALID, "photon map is NULL");
    if (!m->balanced) return fail(MR_ERR_STATE, "mr_photon_map_balance has not been called");
    if (m->device_built) {                    // the device arrays are all there is: read them back
        const uint32_t n = m->count();
        if (n == 0) return MR_OK;
        std::vector<float4> rec(2 * (size_t)(n + 1)), pw((size_t)n + 1);
        std::vector<uint8_t> tp(2 * (size_t)n);
        MR_HIP_CHECK(hipSetDevice(m->device));
        MR_HIP_CHECK(hipDeviceSynchronize());
        MR_HIP_CHECK(hipMemcpy(rec.data(), m->dev.rec, rec.size() * sizeof(float4), hipMemcpyDeviceToHost));
        MR_HIP_CHECK(hipMemcpy(pw.data(), m->dev.power, pw.size() * sizeof(float4), hipMemcpyDeviceToHost));
        MR_HIP_CHECK(hipMemcpy(tp.data(), m->d_dir, tp.size(), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; i++) {
            const float4 a = rec[2 * (size_t)(i + 1)], p = pw[(size_t)i + 1];
            if (pos) { pos[3 * (size_t)i] = a.x; pos[3 * (size_t)i + 1] = a.y; pos[3 * (size_t)i + 2] = a.z; }
            if (power) { power[3 * (size_t)i] = p.x; power[3 * (size_t)i + 1] = p.y; power[3 * (size_t)i + 2] = p.z; }
            if (plane) memcpy(&plane[i], &a.w, 4);
        }
        if (theta_phi) memcpy(theta_phi, tp.data(), tp.size());
        return MR_OK;
    }
    for (uint32_t i = 0; i < m->count(); i++) {
        const uint32_t s = m->heap[i];
        for (int k = 0; k < 3; k++) {
            if (pos) pos[3 * (size_t)i + k] = m->pos[3 * (size_t)s + k];
            if (power) power[3 * (size_t)i + k] = m->power[3 * (size_t)s + k];
        }
        if (plane) plane[i] = m->plane[i];
        if (theta_phi) { theta_phi[2 * (size_t)i] = m->theta[s]; theta_phi[2 * (size_t)i + 1] = m->phi[s]; }
    }
    return MR_OK;
}

mr_status mr_irradiance_estimate(mr_photon_map *m, const float *d_pos, const float *d_normal, uint64_t n_queries,
                                 float max_dist, uint32_t nphotons, float *d_irrad, int32_t *d_found, float *d_r2,
                                 void *stream) {
    if (!m) return fail(MR_ERR_INVALID, "photon map is NULL");
    if (!m->balanced) return fail(MR_ERR_STATE, "mr_photon_map_balance has not been called");
    if (!m->on_device) return fail(MR_ERR_STATE, "photon map was balanced host_only: nothing is resident on a device and there is no CPU fallback");
    if (n_queries == 0) return MR_OK;
    if (!d_pos || !d_normal || !d_irrad) return fail(MR_ERR_INVALID, "NULL argument");
    if (nphotons == 0 || nphotons > kKnnMaxK) return fail(MR_ERR_INVALID, "nphotons must be in [1, %d]", kKnnMaxK);
    MR_HIP_CHECK(hipSetDevice(m->device));
    return estimate(m, d_pos, d_normal, n_queries, max_dist, nphotons, d_irrad, d_found, d_r2, static_cast<hipStream_t>(stream));
}

mr_status mr_photon_map_count_stats(mr_photon_map *m, int32_t enable) {
    if (!m) return fail(MR_ERR_INVALID, "photon map is NULL");
    if (!m->on_device) return fail(MR_ERR_STATE, "photon map is not resident on a device");
    MR_HIP_CHECK(hipSetDevice(m->device));
    if (enable && !m->d_stats) {
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&m->d_stats), kPhotonStats * sizeof(unsigned long long)));
        MR_HIP_CHECK(hipMemset(m->d_stats, 0, kPhotonStats * sizeof(unsigned long long)));
    } else if (!enable && m->d_stats) {
        MR_HIP_CHECK(hipDeviceSynchronize());
        (void)hipFree(m->d_stats);
        m->d_stats = nullptr;
    }
    return MR_OK;
}

mr_status mr_photon_map_get_stats(mr_photon_map *m, uint64_t out[12], int32_t reset) {
    if (!m || !out) return fail(MR_ERR_INVALID, "NULL argument");
    if (!m->d_stats) return fail(MR_ERR_STATE, "mr_photon_map_count_stats has not been enabled on this map");
    MR_HIP_CHECK(hipSetDevice(m->device));
    MR_HIP_CHECK(hipDeviceSynchronize());
    unsigned long long h[kPhotonStats];
    MR_HIP_CHECK(hipMemcpy(h, m->d_stats, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < kPhotonStats; i++) out[i] = h[i];
    if (reset) MR_HIP_CHECK(hipMemset(m->d_stats, 0, sizeof(h)));
    return MR_OK;
}

mr_status mr_final_gather(mr_scene *s, mr_photon_map *global_map, mr_photon_map *caustic_map, const mr_ray *d_rays,
                          const mr_hit *d_hits, uint64_t n, float max_dist, uint32_t nphotons, uint32_t spp,
                          float *d_scratch, float *d_rgb, void *stream_v) {
    if (!s || !s->built || !s->on_device) return fail(MR_ERR_STATE, "scene is not resident on a device");
    if (!d_rays || !d_hits || !d_scratch || !d_rgb) return fail(MR_ERR_INVALID, "NULL argument");
    if (spp == 0 || n % spp != 0) return fail(MR_ERR_INVALID, "n (%llu) must be a multiple of spp (%u)", (unsigned long long)n, spp);
    if (nphotons == 0 || nphotons > kKnnMaxK) return fail(MR_ERR_INVALID, "nphotons must be in [1, %d]", kKnnMaxK);
    mr_photon_map *maps[2] = {global_map, caustic_map};
    for (mr_photon_map *m : maps) {
        if (!m) continue;
        if (!m->balanced || !m->on_device) return fail(MR_ERR_STATE, "photon map is not balanced and resident on a device");
        if (m->device != s->device) return fail(MR_ERR_INVALID, "photon map lives on device %d, the scene on %d", m->device, s->device);
    }
    if (n == 0) return MR_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    float *d_irr[2];
    mr_status st = gather_estimates(s, maps, d_rays, d_hits, nullptr, n, max_dist, nphotons, d_scratch, nullptr, stream, d_irr);
    if (st != MR_OK) return st;
    return launch_gather_accumulate(d_irr[0], d_irr[1], n, spp, d_rgb, stream);
}

mr_status mr_gather_level(mr_scene *s, mr_photon_map *global_map, mr_photon_map *caustic_map, const mr_ray *d_rays,
                          const mr_hit *d_hits, const float *d_normal, const float *d_weights, const uint32_t *d_pixels, uint64_t n,
                          float max_dist, uint32_t nphotons, uint32_t spp, float *d_scratch, float *d_rgb, float *d_ray_rgb,
                          uint64_t *d_counts, void *stream_v) {
    if (!s || !d_rays || !d_hits || !d_scratch || (!d_rgb && !d_ray_rgb)) return fail(MR_ERR_INVALID, "mr_gather_level: NULL argument");
    if (spp == 0) return fail(MR_ERR_INVALID, "mr_gather_level: spp is 0");
    if (n / spp > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "mr_gather_level: too many pixels");
    if (nphotons == 0 || nphotons > kKnnMaxK) return fail(MR_ERR_INVALID, "mr_gather_level: nphotons must be in [1, %d]", kKnnMaxK);
    if ((reinterpret_cast<uintptr_t>(d_rays) & 15) || (reinterpret_cast<uintptr_t>(d_hits) & 15) || (reinterpret_cast<uintptr_t>(d_counts) & 7) ||
        (reinterpret_cast<uintptr_t>(d_rgb) & 3) || (reinterpret_cast<uintptr_t>(d_ray_rgb) & 3) || (reinterpret_cast<uintptr_t>(d_weights) & 3) ||
        (reinterpret_cast<uintptr_t>(d_pixels) & 3) || (reinterpret_cast<uintptr_t>(d_normal) & 3) || (reinterpret_cast<uintptr_t>(d_scratch) & 3))
        return fail(MR_ERR_INVALID, "mr_gather_level: ray / hit buffers must be 16-byte aligned, float buffers 4-byte, counters 8-byte aligned");
    mr_photon_map *maps[2] = {global_map, caustic_map};
    for (mr_photon_map *m : maps)
        if (m && m->device != s->device) return fail(MR_ERR_INVALID, "mr_gather_level: photon map lives on device %d, the scene on %d", m->device, s->device);
    if (!s->built) return fail(MR_ERR_STATE, "mr_gather_level: mr_bvh_build has not been called on this scene");
    if (!s->on_device) return fail(MR_ERR_STATE, "mr_gather_level: scene was built host_only: nothing is resident on a device and there is no CPU fallback");
    for (mr_photon_map *m : maps)
        if (m && (!m->balanced || !m->on_device)) return fail(MR_ERR_STATE, "mr_gather_level: photon map is not balanced and resident on a device");
    if (s->tex.procedural && !d_normal)
        return fail(MR_ERR_STATE, "mr_gather_level: the scene's texture table holds a procedural texture (STONE, STEM, PETAL, LEAF or FLOWER_CENTER), "
                                  "whose normal comes from the surface pass: call mr_hit_surface, then mr_gather_level with its normal buffer");
    if (n == 0) return MR_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    float *d_irr[2];
    mr_status st = gather_estimates(s, maps, d_rays, d_hits, d_normal, n, max_dist, nphotons, d_scratch, d_counts, stream, d_irr);
    if (st != MR_OK) return st;
    if (!d_irr[0] && !d_irr[1] && !d_ray_rgb) return MR_OK;      // no map: nothing to add
    return launch_gather_level_accumulate(d_irr[0], d_irr[1], d_weights, d_pixels, n, spp, d_rgb, d_ray_rgb, stream);
}

}  // extern "C"
