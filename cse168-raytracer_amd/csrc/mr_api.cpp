// mr_api.cpp -- the extern "C" boundary declared in include/miro_hip.h.
// Scene assembly runs on the host, BVH::build on the host (mr_build.cpp) or, opt-in, on the device (mr_bvh_build.hip);
// mr_bvh_build flattens the tree into the device layout of mr_internal.h and uploads it once; mr_trace only moves
// rays/hits and launches.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "mr_internal.h"
#include "mr_launch.h"
#include "mr_tile.h"

namespace mr {

static thread_local char g_err[512] = "";

mr_status fail(mr_status code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

mr_status select_device(int32_t device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(MR_ERR_HIP, "no HIP device available (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device >= count) return fail(MR_ERR_INVALID, "device %d out of range [0,%d)", device, count);
    MR_HIP_CHECK(hipSetDevice(device));
    return MR_OK;
}

namespace {

template <typename T>
mr_status upload(T *&dst, const T *src, size_t count, uint64_t &bytes) {
    const size_t sz = (count ? count : 1) * sizeof(T);
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&dst), sz));
    if (count) MR_HIP_CHECK(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    bytes += sz;
    return MR_OK;
}

void release_device(mr_scene *s) {
    DeviceScene &d = s->dev;
    (void)hipFree(d.nodes); (void)hipFree(d.tris); (void)hipFree(d.tri_prim); (void)hipFree(d.leaf_cnt_ext);
    (void)hipFree(d.v); (void)hipFree(d.n); (void)hipFree(d.vi); (void)hipFree(d.ni);
    (void)hipFree(d.materials); (void)hipFree(d.prim_material);
    (void)hipFree(d.spheres); (void)hipFree(d.planes);
    (void)hipFree(d.texcoords); (void)hipFree(d.ti);
    d = DeviceScene();
    (void)hipFree(s->d_stats); s->d_stats = nullptr;
    (void)hipFree(s->d_work_counters); s->d_work_counters = nullptr;
    for (EyeTables &t : s->eye_tables.set) {
        (void)hipFree(t.d);
        if (t.ready) (void)hipEventDestroy(static_cast<hipEvent_t>(t.ready));
        t = EyeTables();
    }
    s->eye_tables.calls = 0;
    (void)hipFree(s->d_stage_rays); (void)hipFree(s->d_stage_hits);
    s->d_stage_rays = s->d_stage_hits = nullptr;
    s->stage_cap = 0;
    for (void *e : s->stage_events) (void)hipEventDestroy(static_cast<hipEvent_t>(e));
    s->stage_events.clear();
    if (s->copy_in) (void)hipStreamDestroy(static_cast<hipStream_t>(s->copy_in));
    if (s->copy_out) (void)hipStreamDestroy(static_cast<hipStream_t>(s->copy_out));
    s->copy_in = s->copy_out = nullptr;
    (void)hipFree(s->d_occluded);
    s->d_occluded = nullptr;
    s->occluded_cap = 0;
    (void)hipFree(s->d_light_scale);
    s->d_light_scale = nullptr;
    s->light_scale_cap = 0;
    (void)hipFree(s->d_env);
    s->d_env = nullptr;
    s->env_dirty = s->env.W != 0;          // the image outlives the device records: the next shade call uploads it again
    (void)hipFree(s->d_tex);
    s->d_tex = nullptr;
    s->tex_dirty = !s->tex.blob.empty();   // and so does the texture table
    (void)hipFree(s->d_finish_state);
    s->d_finish_state = nullptr;
}

inline int32_t leaf_ref(uint32_t first, uint32_t count) {
    const uint32_t c = count < (uint32_t)kLeafCountMask ? count : (uint32_t)kLeafCountMask;
    return (int32_t)~((first << kLeafCountBits) | c);
}

mr_status upload_materials(mr_scene *s);
mr_status upload_texcoords(mr_scene *s);

// Storage order of the inner nodes (MR_LAYOUT_*): the list of host node indices in the order their records are stored;
// -1 = an unused padding record.  Node identity, references and visiting order do not depend on it.
std::vector<int32_t> node_storage_order(const HostTree &t, uint32_t mode) {
    std::vector<int32_t> order;
    const auto inner = [&](int32_t n) { return n >= 0 && !t.nodes[(size_t)n].is_leaf; };
    if (t.nodes.empty() || t.nodes[0].is_leaf) return order;
    if (mode == MR_LAYOUT_PAIRS) {
        // pre-order; a node that has an inner child and would start in the second half of a line although it is not the
        // partner of the record before it moves to the next line: (node, first inner child) always share 128 bytes
        struct Item { int32_t node; bool partner; };
        std::vector<Item> stack{{0, false}};
        while (!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            const HostNode &nd = t.nodes[(size_t)it.node];
            const int32_t first = inner(nd.a) ? nd.a : (inner(nd.b) ? nd.b : -1);
            const int32_t other = (first == nd.a && inner(nd.b)) ? nd.b : -1;
            if (!it.partner && (order.size() & 1) && first >= 0) order.push_back(-1);
            const bool even = (order.size() & 1) == 0;
            order.push_back(it.node);
            if (other >= 0) stack.push_back({other, false});
            if (first >= 0) stack.push_back({first, even});
        }
        return order;
    }
    if (mode == MR_LAYOUT_TREELETS) {
        constexpr int kTop = 12, kTreelet = 3;
        std::vector<int32_t> frontier{0}, roots;
        for (int level = 0; level < kTop && !frontier.empty(); level++) {        // breadth-first top
            std::vector<int32_t> next;
            for (int32_t n : frontier) {
                order.push_back(n);
                for (int32_t c : {t.nodes[(size_t)n].a, t.nodes[(size_t)n].b})
                    if (inner(c)) next.push_back(c);
            }
            frontier.swap(next);
        }
        roots = frontier;
        // below: a treelet = the inner nodes of up to kTreelet levels under its root, breadth-first and contiguous; the
        // treelets under it follow depth-first
        std::vector<int32_t> stack(roots.rbegin(), roots.rend());
        while (!stack.empty()) {
            const int32_t root = stack.back();
            stack.pop_back();
            std::vector<int32_t> level{root}, below;
            for (int l = 0; l < kTreelet && !level.empty(); l++) {
                std::vector<int32_t> next;
                for (int32_t n : level) {
                    order.push_back(n);
                    for (int32_t c : {t.nodes[(size_t)n].a, t.nodes[(size_t)n].b})
                        if (inner(c)) next.push_back(c);
                }
                level.swap(next);
            }
            for (auto it = level.rbegin(); it != level.rend(); ++it) stack.push_back(*it);
        }
        return order;
    }
    for (size_t i = 0; i < t.nodes.size(); i++)
        if (!t.nodes[i].is_leaf) order.push_back((int32_t)i);
    return order;
}

// host tree -> device records
mr_status flatten_and_upload(mr_scene *s, uint32_t layout) {
    const HostTree &t = s->tree;
    const HostMesh &m = s->mesh;
    DeviceScene &d = s->dev;
    const uint32_t nt = m.n_triangles();
    if (nt >= (1u << (31 - kLeafCountBits)))
        return fail(MR_ERR_INVALID, "scene has %u triangles; the leaf reference encoding holds < %u", nt,
                    1u << (31 - kLeafCountBits));

    // inner nodes get their record index from the storage order (depth-first pre-order by default)
    const std::vector<int32_t> order = node_storage_order(t, layout & 15u);
    std::vector<int32_t> inner_id(t.nodes.size(), -1);
    const uint32_t n_inner = (uint32_t)order.size();
    for (uint32_t k = 0; k < n_inner; k++)
        if (order[k] >= 0) inner_id[(size_t)order[k]] = (int32_t)k;
    for (size_t i = 0; i < t.nodes.size(); i++)
        if (!t.nodes[i].is_leaf && inner_id[i] < 0) return fail(MR_ERR_STATE, "node %zu missing from the storage order", i);

    // leaves: where each one's triangles start in the record array.  MR_LAYOUT_ALIGN_LEAVES puts up to seven unused
    // 48-byte records in front of a leaf when that lowers the number of 128-byte lines its triangles touch.
    std::vector<uint32_t> leaf_first(t.nodes.size(), 0);
    uint32_t n_rec = 0;
    {
        std::vector<uint32_t> leaves;
        for (size_t i = 0; i < t.nodes.size(); i++)
            if (t.nodes[i].is_leaf) leaves.push_back((uint32_t)i);
        std::sort(leaves.begin(), leaves.end(), [&](uint32_t x, uint32_t y) { return t.nodes[x].a < t.nodes[y].a; });
        for (uint32_t li : leaves) {
            const uint32_t cnt = (uint32_t)t.nodes[li].b;
            if ((layout & MR_LAYOUT_ALIGN_LEAVES) && cnt > 0 && cnt <= 8) {
                const auto lines = [&](uint32_t first) { return (first * 48u + cnt * 48u - 1u) / 128u - (first * 48u) / 128u + 1u; };
                uint32_t best = 0;
                for (uint32_t pad = 1; pad < 8; pad++)
                    if (lines(n_rec + pad) < lines(n_rec + best)) best = pad;
                n_rec += best;
            }
            leaf_first[li] = n_rec;
            n_rec += cnt;
        }
    }
    if (n_rec >= (1u << (31 - kLeafCountBits))) return fail(MR_ERR_INVALID, "padded triangle array exceeds the leaf reference encoding");
    auto ref_of = [&](int32_t node) -> int32_t {
        const HostNode &nd = t.nodes[(size_t)node];
        return nd.is_leaf ? leaf_ref(leaf_first[(size_t)node], (uint32_t)nd.b) : inner_id[(size_t)node];
    };

    std::vector<float4> nodes((size_t)n_inner * 4, make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t i = 0; i < t.nodes.size(); i++) {
        const HostNode &nd = t.nodes[i];
        if (nd.is_leaf) continue;
        const HostNode &c0 = t.nodes[(size_t)nd.a], &c1 = t.nodes[(size_t)nd.b];
        float4 *q = &nodes[(size_t)inner_id[i] * 4];
        q[0] = make_float4(c0.lo[0], c0.hi[0], c0.lo[1], c0.hi[1]);
        q[1] = make_float4(c1.lo[0], c1.hi[0], c1.lo[1], c1.hi[1]);
        q[2] = make_float4(c0.lo[2], c0.hi[2], c1.lo[2], c1.hi[2]);
        // refs[2] = 1 marks an "irregular" node: some child corner is not finite (empty leaves keep [inf,-inf]) or lies
        // outside 0 / [2^-36, 2^60] in magnitude; the default trace then divides like the reference instead of using the
        // correction step (mr_kernels.hip: exact_quot)
        int32_t irregular = 0;
        for (const HostNode *c : {&c0, &c1})
            for (int k = 0; k < 3; k++)
                for (float v : {c->lo[k], c->hi[k]}) {
                    const float m = fabsf(v);
                    if (!(m == 0.0f || (m >= 0x1p-36f && m <= 0x1p60f))) irregular = 1;
                }
        int32_t refs[4] = {ref_of(nd.a), ref_of(nd.b), irregular, 0};
        memcpy(&q[3], refs, sizeof(refs));
    }

    // triangles pre-gathered in leaf order: A, B-A, C-A, (B-A)x(C-A)  (Triangle.cpp:143-151)
    std::vector<float4> tris((size_t)n_rec * 3, make_float4(0.f, 0.f, 0.f, 0.f));
    std::vector<uint32_t> cnt_ext(n_rec, 0), rec_prim(n_rec, MR_MISS);
    for (size_t li = 0; li < t.nodes.size(); li++) {
        const HostNode &leaf = t.nodes[li];
        if (!leaf.is_leaf) continue;
        for (int32_t j = 0; j < leaf.b; j++) {
            const uint32_t k = leaf_first[li] + (uint32_t)j;
            const uint32_t prim = t.leaf_prims[(size_t)leaf.a + (size_t)j];
            rec_prim[k] = prim;
            if (m.is_sphere(prim)) {
                const float *sp = &m.spheres[4 * (size_t)m.vi[3 * (size_t)prim + 1]];
                uint32_t tag = kSphereTag;
                float tagf;
                memcpy(&tagf, &tag, sizeof(tagf));
                tris[3 * (size_t)k + 0] = make_float4(sp[0], sp[1], sp[2], sp[3]);
                tris[3 * (size_t)k + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
                tris[3 * (size_t)k + 2] = make_float4(0.f, 0.f, 0.f, tagf);
                continue;
            }
            const float *A = &m.v[3 * (size_t)m.vi[3 * prim]];
            const float *B = &m.v[3 * (size_t)m.vi[3 * prim + 1]];
            const float *C = &m.v[3 * (size_t)m.vi[3 * prim + 2]];
            const float bx = B[0] - A[0], by = B[1] - A[1], bz = B[2] - A[2];
            const float cx = C[0] - A[0], cy = C[1] - A[1], cz = C[2] - A[2];
            const float nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
            tris[3 * (size_t)k + 0] = make_float4(A[0], A[1], A[2], bx);
            tris[3 * (size_t)k + 1] = make_float4(by, bz, cx, cy);
            tris[3 * (size_t)k + 2] = make_float4(cz, nx, ny, nz);
        }
        if (leaf.b >= kLeafCountMask && leaf.b > 0) cnt_ext[(size_t)leaf_first[li]] = (uint32_t)leaf.b;
    }

    d.bytes = 0;
    mr_status st;
    if ((st = upload(d.nodes, nodes.data(), nodes.size(), d.bytes)) != MR_OK) return st;
    if ((st = upload(d.tris, tris.data(), tris.size(), d.bytes)) != MR_OK) return st;
    if ((st = upload(d.tri_prim, rec_prim.data(), rec_prim.size(), d.bytes)) != MR_OK) return st;
    if ((st = upload(d.leaf_cnt_ext, cnt_ext.data(), cnt_ext.size(), d.bytes)) != MR_OK) return st;
    if ((st = upload(d.v, m.v.data(), m.v.size(), d.bytes)) != MR_OK) return st;
    if ((st = upload(d.n, m.n.data(), m.n.size(), d.bytes)) != MR_OK) return st;
    if ((st = upload(d.vi, m.vi.data(), m.vi.size(), d.bytes)) != MR_OK) return st;
    if ((st = upload(d.ni, m.ni.data(), m.ni.size(), d.bytes)) != MR_OK) return st;
    d.n_spheres = m.n_spheres();
    d.n_planes = m.n_planes();
    if (d.n_spheres) {
        std::vector<float4> sp(d.n_spheres);
        for (uint32_t i = 0; i < d.n_spheres; i++)
            sp[i] = make_float4(m.spheres[4 * i], m.spheres[4 * i + 1], m.spheres[4 * i + 2], m.spheres[4 * i + 3]);
        if ((st = upload(d.spheres, sp.data(), sp.size(), d.bytes)) != MR_OK) return st;
    }
    if (d.n_planes) {
        std::vector<float4> pl(2 * (size_t)d.n_planes);
        for (uint32_t i = 0; i < d.n_planes; i++) {
            float matf;
            memcpy(&matf, &m.plane_material[i], sizeof(matf));
            pl[2 * i] = make_float4(m.planes[6 * i], m.planes[6 * i + 1], m.planes[6 * i + 2], matf);
            pl[2 * i + 1] = make_float4(m.planes[6 * i + 3], m.planes[6 * i + 4], m.planes[6 * i + 5], 0.f);
        }
        if ((st = upload(d.planes, pl.data(), pl.size(), d.bytes)) != MR_OK) return st;
    }
    const HostNode &root = t.nodes[0];
    memcpy(d.root_lo, root.lo, sizeof(d.root_lo));
    memcpy(d.root_hi, root.hi, sizeof(d.root_hi));
    d.root_ref = ref_of(0);
    d.n_inner = n_inner;
    d.n_tris = n_rec;
    d.stack_depth = t.max_depth + 1;   // pending far children (one per inner node on a root-to-leaf path, <= max_depth) + the kDone sentinel
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&s->d_stats), 2 * sizeof(unsigned long long)));
    MR_HIP_CHECK(hipMemset(s->d_stats, 0, 2 * sizeof(unsigned long long)));
    // two rings: [0, kWorkCounters) for the persistent trace kernels (zeroed before each launch), [kWorkCounters, 2 kWorkCounters) for
    // the tails of large frames (zero here, re-armed by the launch's last reader: mr_frame.hip)
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&s->d_work_counters), 2 * kWorkCounters * sizeof(unsigned long long)));
    MR_HIP_CHECK(hipMemset(s->d_work_counters, 0, 2 * kWorkCounters * sizeof(unsigned long long)));
    if ((st = upload_texcoords(s)) != MR_OK) return st;
    return upload_materials(s);
}

// the texture coordinates and their three indices per object (mr_uv.h); objects added behind the last one that has any get none
mr_status upload_texcoords(mr_scene *s) {
    DeviceScene &d = s->dev;
    const HostMesh &m = s->mesh;
    (void)hipFree(d.texcoords); (void)hipFree(d.ti);
    d.texcoords = nullptr; d.ti = nullptr;
    if (m.t.empty()) return MR_OK;
    if (m.ti.size() > m.vi.size()) return fail(MR_ERR_STATE, "texture-coordinate indices cover %zu objects, the scene holds %u", m.ti.size() / 3, m.n_triangles());
    std::vector<uint32_t> ti(m.ti);
    ti.resize(m.vi.size(), kNoTexcoord);
    uint64_t bytes = 0;
    mr_status st;
    if ((st = upload(d.texcoords, m.t.data(), m.t.size(), bytes)) != MR_OK) return st;
    return upload(d.ti, ti.data(), ti.size(), bytes);
}

// default: one white Lambert = Phong(Vector3(1)) (Lambert.h:9, Phong.h:10-14: shininess 1, index 1)
mr_status upload_materials(mr_scene *s) {
    DeviceScene &d = s->dev;
    // the kernels index prim_material[] with every object of the scene: a table set before later geometry was added
    // would be read out of bounds (mr_surface.h material_id)
    if (!s->prim_material.empty() && s->prim_material.size() != s->mesh.n_triangles())
        return fail(MR_ERR_STATE, "mr_scene_set_materials covered %zu objects, the scene now holds %u: set the materials "
                                  "again after the last object was added", s->prim_material.size(), s->mesh.n_triangles());
    (void)hipFree(d.materials); (void)hipFree(d.prim_material);
    d.materials = nullptr; d.prim_material = nullptr;
    d.user_materials = s->materials.empty() ? 0u : 1u;
    d.refractive = 0;
    for (size_t i = 0; i + 10 < s->materials.size(); i += 11)
        if (s->materials[i + 6] > 0.f || s->materials[i + 7] > 0.f || s->materials[i + 8] > 0.f) d.refractive = 1;
    static const float white[11] = {1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1};
    const float *src = s->materials.empty() ? white : s->materials.data();
    const size_t nfl = s->materials.empty() ? 11 : s->materials.size();
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d.materials), nfl * sizeof(float)));
    MR_HIP_CHECK(hipMemcpy(d.materials, src, nfl * sizeof(float), hipMemcpyHostToDevice));
    if (!s->prim_material.empty()) {
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d.prim_material), s->prim_material.size() * sizeof(uint32_t)));
        MR_HIP_CHECK(hipMemcpy(d.prim_material, s->prim_material.data(), s->prim_material.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return MR_OK;
}

mr_status ensure_stage(mr_scene *s, uint64_t n) {
    if (n <= s->stage_cap) return MR_OK;
    (void)hipFree(s->d_stage_rays); (void)hipFree(s->d_stage_hits);
    s->d_stage_rays = s->d_stage_hits = nullptr;
    s->stage_cap = 0;
    MR_HIP_CHECK(hipMalloc(&s->d_stage_rays, n * sizeof(mr_ray)));
    MR_HIP_CHECK(hipMalloc(&s->d_stage_hits, n * sizeof(mr_hit)));
    s->stage_cap = n;
    return MR_OK;
}

// copy streams and 2 events per chunk for the pipelined host-pointer trace
mr_status ensure_copy_pipeline(mr_scene *s, uint64_t n_chunks) {
    if (!s->copy_in) {
        hipStream_t a = nullptr;
        MR_HIP_CHECK(hipStreamCreateWithFlags(&a, hipStreamNonBlocking));
        s->copy_in = a;
    }
    if (!s->copy_out) {
        hipStream_t b = nullptr;
        MR_HIP_CHECK(hipStreamCreateWithFlags(&b, hipStreamNonBlocking));
        s->copy_out = b;
    }
    while (s->stage_events.size() < 2 * n_chunks) {
        hipEvent_t e = nullptr;
        MR_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        s->stage_events.push_back(e);
    }
    return MR_OK;
}

mr_status require_built(const mr_scene *s) {
    if (!s) return fail(MR_ERR_INVALID, "scene is NULL");
    if (!s->built) return fail(MR_ERR_STATE, "mr_bvh_build has not been called on this scene");
    return MR_OK;
}

mr_status require_device(const mr_scene *s) {
    mr_status st = require_built(s);
    if (st != MR_OK) return st;
    if (!s->on_device)
        return fail(MR_ERR_STATE, "scene was built host_only: nothing is resident on a device and there is no CPU fallback");
    return MR_OK;
}

}  // namespace

// the texture table on the device, uploaded on `stream` by the first shading call after a change; `p`: as the kernels take it
// (declared in mr_internal.h: mr_trace_photons_surface in mr_photon_trace.cpp takes it too)
mr_status texture_params(mr_scene *s, hipStream_t stream, TexParams &p) {
    const HostTextures &t = s->tex;
    if (s->tex_dirty) {
        (void)hipFree(s->d_tex);
        s->d_tex = nullptr;
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&s->d_tex), t.blob.size() * sizeof(float4)));
        MR_HIP_CHECK(hipMemcpyAsync(s->d_tex, t.blob.data(), t.blob.size() * sizeof(float4), hipMemcpyHostToDevice, stream));
        s->tex_dirty = false;
    }
    p.recs = s->d_tex;
    p.texels = s->d_tex + t.texel_base;
    p.mat_tex = reinterpret_cast<const uint32_t *>(s->d_tex + t.mat_base);
    p.texcoords = s->dev.texcoords;
    p.ti = s->dev.ti;
    return MR_OK;
}

namespace {

// what the entry points that shade without the texture lookup answer on a scene with a texture table
mr_status refuse_textured(const mr_scene *s, const char *who) {
    if (s->tex.blob.empty()) return MR_OK;
    return fail(MR_ERR_STATE, "%s: the scene has a texture table (mr_scene_set_textures) and this call shades without the lookup; "
                              "use the batched calls mr_trace -> mr_shade_lights, or mr_gen_shadow_rays -> mr_trace_indirect -> "
                              "mr_shade_accumulate", who);
}

// what mr_scene_set_lights and mr_shade_square_lights ask of light i of a list: reserved words 0; finite position, colour and
// wattage; with `normal` (a light that has one) a finite normal that is not zero
mr_status check_light(const char *who, uint32_t i, const uint32_t reserved[4], const float position[3], const float color[3], float wattage,
                      const float *normal) {
    for (int k = 0; k < 4; k++)
        if (reserved[k] != 0) return fail(MR_ERR_INVALID, "%s: light %u: reserved must be 0", who, i);
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(position[c]) || !std::isfinite(color[c])) return fail(MR_ERR_INVALID, "%s: light %u: position and color must be finite", who, i);
    if (!std::isfinite(wattage)) return fail(MR_ERR_INVALID, "%s: light %u: wattage must be finite", who, i);
    if (!normal) return MR_OK;
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(normal[c])) return fail(MR_ERR_INVALID, "%s: light %u: the normal must be finite", who, i);
    if (normal[0] == 0.0f && normal[1] == 0.0f && normal[2] == 0.0f) return fail(MR_ERR_INVALID, "%s: light %u: the normal is zero", who, i);
    return MR_OK;
}

// what the entry points that compute a hit's colour or normal themselves answer on a scene with a procedural texture
mr_status refuse_procedural(const mr_scene *s, const char *who, const char *instead) {
    if (!s->tex.procedural) return MR_OK;
    return fail(MR_ERR_STATE, "%s: the scene's texture table holds a procedural texture (STONE, STEM, PETAL, LEAF or FLOWER_CENTER), whose "
                              "colour and normal come from the surface pass: call mr_hit_surface, then %s", who, instead);
}

// LoadedTexture::LoadedTexture (Texture.cpp:30-92) for a FIT_RGBF image of W x H pixels: m_maxIntensity and the low-res image,
// written behind the image's own records in e.rec
void build_environment_image(HostEnvironment &e, const float *px) {
    const int w = (int)e.W, h = (int)e.H;
    const int lrw = (int)e.lw, lrh = (int)e.lh;
    e.rec.assign(4 * ((size_t)w * h + (size_t)lrw * lrh), 0.0f);
    float max_intensity = -1e15;                                               // :34
    for (int i = 0; i < h; i++)                                                // :41-50
        for (int j = 0; j < w; j++) {
            const float *p = px + 3 * ((size_t)i * w + j);
            float *r = &e.rec[4 * ((size_t)i * w + j)];
            for (int k = 0; k < 3; k++) {
                if (max_intensity < p[k]) max_intensity = p[k];
                r[k] = p[k];
            }
        }
    e.max_intensity = max_intensity;
    const float PI = 3.1415926535897932384626433832795028841972f;               // Miro.h:10
    float *low = &e.rec[4 * (size_t)w * h];
    for (int i = 0; i < lrh; i++)                                              // :63-91
        for (int j = 0; j < lrw; j++) {
            long double acc[3] = {0.0, 0.0, 0.0};
            const int midX = (w / lrw) * j + (w / lrw) / 2;
            const int midY = (h / lrh) * i + (h / lrh) / 2;
            for (int ii = (h / lrh) * i; ii < (h / lrh) * i + (h / lrh) && ii < h; ii++)
                for (int jj = (w / lrw) * j; jj < (w / lrw) * j + (w / lrw) && jj < w; jj++) {
                    const float *p = px + 3 * ((size_t)ii * w + jj);
                    const float x = jj - midX, y = ii - midY;
                    const float sigma = 1;
                    const long double g = 1.0 / (2.0 * PI * sigma) * std::exp(-(x * x + y * y) / (2 * sigma));   // :80, exp(float)
                    acc[0] += g * p[0];
                    acc[1] += g * p[1];
                    acc[2] += g * p[2];
                }
            float *r = low + 4 * ((size_t)i * lrw + j);
            r[0] = (float)acc[0];                                              // setPixel, FIT_RGBF (:118-124): red = value[0],
            r[1] = (float)acc[2];                                              // green = value[2],
            r[2] = (float)acc[1];                                              // blue = value[1]
        }
}

// one of the addresses `p` is no multiple of `align`, a power of two (NULL is aligned: an optional buffer passes)
template <typename... P>
bool misaligned(uintptr_t align, const P *...p) {
    return ((reinterpret_cast<uintptr_t>(p) | ...) & (align - 1)) != 0;
}

}  // namespace
}  // namespace mr

using namespace mr;

extern "C" {

const char *mr_last_error(void) { return g_err; }
const char *mr_version(void) { return "miro_hip 0.2 (gfx950)"; }

mr_status mr_scene_create(int32_t device, mr_scene **out) {
    if (!out) return fail(MR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (device < 0) return fail(MR_ERR_INVALID, "device %d is negative", device);
    mr_scene *s = new (std::nothrow) mr_scene();
    if (!s) return fail(MR_ERR_NOMEM, "out of host memory");
    s->device = device;
    *out = s;
    return MR_OK;
}

mr_status mr_scene_destroy(mr_scene *s) {
    if (!s) return MR_OK;
    if (s->on_device) {
        (void)hipSetDevice(s->device);
        release_device(s);
    }
    delete s;
    return MR_OK;
}

mr_status mr_scene_add_mesh(mr_scene *s, const mr_mesh_desc *mesh) {
    if (!s || !mesh) return fail(MR_ERR_INVALID, "NULL argument");
    if (s->built) return fail(MR_ERR_STATE, "scene is immutable after mr_bvh_build");
    if ((mesh->n_vertices && !mesh->vertices) || (mesh->n_normals && !mesh->normals) ||
        (mesh->n_triangles && (!mesh->vidx || !mesh->nidx)))
        return fail(MR_ERR_INVALID, "mesh descriptor has NULL arrays");
    for (uint32_t i = 0; i < 3 * mesh->n_triangles; i++) {
        if (mesh->vidx[i] >= mesh->n_vertices) return fail(MR_ERR_INVALID, "vertex index %u out of range", mesh->vidx[i]);
        if (mesh->nidx[i] >= mesh->n_normals) return fail(MR_ERR_INVALID, "normal index %u out of range", mesh->nidx[i]);
    }
    HostMesh &m = s->mesh;
    const uint32_t vb = m.n_vertices(), nb = m.n_normals();
    m.v.insert(m.v.end(), mesh->vertices, mesh->vertices + 3 * (size_t)mesh->n_vertices);
    m.n.insert(m.n.end(), mesh->normals, mesh->normals + 3 * (size_t)mesh->n_normals);
    for (uint32_t i = 0; i < 3 * mesh->n_triangles; i++) {
        m.vi.push_back(mesh->vidx[i] + vb);
        m.ni.push_back(mesh->nidx[i] + nb);
    }
    return MR_OK;
}

mr_status mr_scene_add_obj(mr_scene *s, const char *path, const float *ctm16, uint32_t *n_triangles_out) {
    if (!s || !path) return fail(MR_ERR_INVALID, "NULL argument");
    if (s->built) return fail(MR_ERR_STATE, "scene is immutable after mr_bvh_build");
    return load_obj(path, ctm16, s->mesh, n_triangles_out);
}

mr_status mr_scene_add_triangle(mr_scene *s, const float v[9], const float n[9]) {
    static const uint32_t idx[3] = {0, 1, 2};
    mr_mesh_desc d;
    d.vertices = v; d.n_vertices = 3;
    d.normals = n;  d.n_normals = 3;
    d.vidx = idx; d.nidx = idx; d.n_triangles = 1;
    return mr_scene_add_mesh(s, &d);
}

mr_status mr_scene_add_sphere(mr_scene *s, const float center[3], float radius, uint32_t *prim_out) {
    if (!s || !center) return fail(MR_ERR_INVALID, "NULL argument");
    if (s->built) return fail(MR_ERR_STATE, "scene is immutable after mr_bvh_build");
    HostMesh &m = s->mesh;
    const uint32_t slot[3] = {kSphereSlot, m.n_spheres(), 0u};
    if (prim_out) *prim_out = m.n_triangles();
    m.vi.insert(m.vi.end(), slot, slot + 3);
    m.ni.insert(m.ni.end(), slot, slot + 3);
    m.spheres.insert(m.spheres.end(), center, center + 3);
    m.spheres.push_back(radius);
    return MR_OK;
}

mr_status mr_scene_add_plane(mr_scene *s, const float normal[3], const float origin[3], uint32_t material,
                             uint32_t *index_out) {
    if (!s || !normal || !origin) return fail(MR_ERR_INVALID, "NULL argument");
    if (s->built) return fail(MR_ERR_STATE, "scene is immutable after mr_bvh_build");
    HostMesh &m = s->mesh;
    if (index_out) *index_out = m.n_planes();
    m.planes.insert(m.planes.end(), normal, normal + 3);
    m.planes.insert(m.planes.end(), origin, origin + 3);
    m.plane_material.push_back(material);
    return MR_OK;
}

// where the calling thread's last mr_bvh_build spent its time (mr_bvh_build_timing)
struct BuildTiming { uint32_t builder_used = MR_BUILD_REFERENCE; double prims_ms = 0.0, levels_ms = 0.0, finish_ms = 0.0, upload_ms = 0.0; };
static thread_local BuildTiming g_build_timing;

mr_status mr_bvh_build(mr_scene *s, const mr_build_opts *opts) {
    if (!s) return fail(MR_ERR_INVALID, "scene is NULL");
    uint32_t leaf = 4, builder = MR_BUILD_REFERENCE;
    const bool host_only = opts && opts->host_only;
    if (opts) {
        builder = opts->builder;
        if (builder != MR_BUILD_REFERENCE && builder != MR_BUILD_REFERENCE_DEVICE) return fail(MR_ERR_INVALID, "unknown builder %u", builder);
        if (builder == MR_BUILD_REFERENCE_DEVICE && host_only)
            return fail(MR_ERR_INVALID, "builder MR_BUILD_REFERENCE_DEVICE builds on a device: host_only must be 0 with it");
        if (opts->leaf_size) leaf = opts->leaf_size;
    }
    if (!host_only) {
        mr_status st = select_device(s->device);
        if (st != MR_OK) return st;
    }
    if (s->on_device) release_device(s);
    s->built = false;
    s->on_device = false;
    BuildTiming timing;
    mr_status st = MR_OK;
    bool on_host = builder == MR_BUILD_REFERENCE;
    if (!on_host) {
        BvhBuildPhases ph;
        st = build_reference_tree_device(s->mesh, leaf, s->tree, ph, on_host);      // on_host: a non-finite coordinate
        if (st != MR_OK) return st;
        timing.builder_used = MR_BUILD_REFERENCE_DEVICE;
        timing.prims_ms = ph.prims_ms; timing.levels_ms = ph.levels_ms; timing.finish_ms = ph.finish_ms;
    }
    if (on_host) {
        const auto t0 = std::chrono::steady_clock::now();
        st = build_reference_tree(s->mesh, leaf, s->tree);
        if (st != MR_OK) return st;
        timing.builder_used = MR_BUILD_REFERENCE;
        timing.levels_ms = ms_since(t0);
    }
    g_build_timing = timing;
    s->built = true;
    if (host_only) return MR_OK;
    const uint32_t layout = opts ? opts->layout : 0u;
    if ((layout & 15u) > MR_LAYOUT_TREELETS || (layout & ~(uint32_t)(15u | MR_LAYOUT_ALIGN_LEAVES)))
        return fail(MR_ERR_INVALID, "unknown layout %u", layout);
    const auto t0 = std::chrono::steady_clock::now();
    st = flatten_and_upload(s, layout);
    if (st != MR_OK) { release_device(s); return st; }
    g_build_timing.upload_ms = ms_since(t0);
    s->on_device = true;
    return MR_OK;
}

mr_status mr_bvh_build_timing(uint32_t *builder_used, double *prims_ms, double *levels_ms, double *finish_ms, double *upload_ms) {
    if (builder_used) *builder_used = g_build_timing.builder_used;
    if (prims_ms) *prims_ms = g_build_timing.prims_ms;
    if (levels_ms) *levels_ms = g_build_timing.levels_ms;
    if (finish_ms) *finish_ms = g_build_timing.finish_ms;
    if (upload_ms) *upload_ms = g_build_timing.upload_ms;
    return MR_OK;
}

mr_status mr_scene_get_info(const mr_scene *s, mr_scene_info *info) {
    if (!s || !info) return fail(MR_ERR_INVALID, "NULL argument");
    memset(info, 0, sizeof(*info));
    info->n_vertices = s->mesh.n_vertices();
    info->n_normals = s->mesh.n_normals();
    info->n_triangles = s->mesh.n_triangles();
    info->built = s->built ? 1u : 0u;
    info->device = s->device;
    if (s->built) {
        info->n_nodes = (uint32_t)s->tree.nodes.size();
        info->n_leaves = s->tree.n_leaves;
        info->max_depth = s->tree.max_depth;
        info->leaf_size = s->tree.leaf_size;
        info->device_bytes = s->dev.bytes;
    }
    return MR_OK;
}

mr_status mr_scene_get_mesh(const mr_scene *s, mr_mesh_desc *out) {
    if (!s || !out) return fail(MR_ERR_INVALID, "NULL argument");
    out->vertices = s->mesh.v.data(); out->n_vertices = s->mesh.n_vertices();
    out->normals = s->mesh.n.data();  out->n_normals = s->mesh.n_normals();
    out->vidx = s->mesh.vi.data();    out->nidx = s->mesh.ni.data();
    out->n_triangles = s->mesh.n_triangles();
    return MR_OK;
}

mr_status mr_scene_export_tree(const mr_scene *s, float *corners6, int32_t *meta3, uint32_t *leaf_prims) {
    mr_status st = require_built(s);
    if (st != MR_OK) return st;
    const HostTree &t = s->tree;
    for (size_t i = 0; i < t.nodes.size(); i++) {
        if (corners6) {
            memcpy(corners6 + 6 * i, t.nodes[i].lo, 3 * sizeof(float));
            memcpy(corners6 + 6 * i + 3, t.nodes[i].hi, 3 * sizeof(float));
        }
        if (meta3) {
            meta3[3 * i] = t.nodes[i].is_leaf;
            meta3[3 * i + 1] = t.nodes[i].a;
            meta3[3 * i + 2] = t.nodes[i].b;
        }
    }
    if (leaf_prims) memcpy(leaf_prims, t.leaf_prims.data(), t.leaf_prims.size() * sizeof(uint32_t));
    return MR_OK;
}

mr_status mr_trace(mr_scene *s, const mr_ray *rays, uint64_t n, mr_hit *hits, uint32_t flags, void *stream_v) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (n == 0) return MR_OK;
    if (!rays || !hits) return fail(MR_ERR_INVALID, "rays/hits is NULL");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    MR_HIP_CHECK(hipSetDevice(s->device));
    const bool rays_dev = flags & MR_RAYS_ON_DEVICE, hits_dev = flags & MR_HITS_ON_DEVICE;
    if ((rays_dev && misaligned(16, rays)) || (hits_dev && misaligned(16, hits)))
        return fail(MR_ERR_INVALID, "device ray/hit buffers must be 16-byte aligned");
    const mr_ray *d_rays = rays;
    mr_hit *d_hits = hits;
    // host buffers go through the scene's staging buffers: one such call at a time (the call is synchronous anyway)
    std::unique_lock<std::mutex> staged(s->stage_mutex, std::defer_lock);
    if (!rays_dev || !hits_dev) {
        staged.lock();
        if ((st = ensure_stage(s, n)) != MR_OK) return st;
        // batches above kStageChunk are uploaded chunk by chunk on the copy stream below; smaller ones in one piece here
        if (!rays_dev) {
            if (n <= kStageChunk)
                MR_HIP_CHECK(hipMemcpyAsync(s->d_stage_rays, rays, n * sizeof(mr_ray), hipMemcpyHostToDevice, stream));
            d_rays = static_cast<const mr_ray *>(s->d_stage_rays);
        }
        if (!hits_dev) d_hits = static_cast<mr_hit *>(s->d_stage_hits);
    }
    TraceParams p = scene_trace_params(s->dev);
    p.rays = d_rays; p.hits = d_hits; p.n = n; p.stats = s->d_stats;
    p.work_counter = s->d_work_counters + (s->next_counter.fetch_add(1) % kWorkCounters);
    if (staged.owns_lock() && n > kStageChunk) {
        // host buffers, large batch: chunk k+1 uploads and chunk k-1 downloads while chunk k is traced (full overlap when
        // the caller's buffers are pinned -- mr_host_alloc --, since only then are the copies asynchronous to this thread)
        const uint64_t n_chunks = (n + kStageChunk - 1) / kStageChunk;
        if ((st = ensure_copy_pipeline(s, n_chunks)) != MR_OK) return st;
        // (alternating the uploads between two copy streams changes nothing: one queue already fills the link, 27 GB/s up)
        hipStream_t in = static_cast<hipStream_t>(s->copy_in), out = static_cast<hipStream_t>(s->copy_out);
        // one chunk; on any failure the three streams are drained before stage_mutex is released, so that the next
        // caller never shares the staging buffers with copies still in flight
        auto chunk = [&](uint64_t k) -> mr_status {
            const uint64_t off = k * kStageChunk, m = n - off < kStageChunk ? n - off : kStageChunk;
            hipEvent_t up = static_cast<hipEvent_t>(s->stage_events[2 * k]), done = static_cast<hipEvent_t>(s->stage_events[2 * k + 1]);
            if (!rays_dev) {
                MR_HIP_CHECK(hipMemcpyAsync(static_cast<mr_ray *>(s->d_stage_rays) + off, rays + off, m * sizeof(mr_ray), hipMemcpyHostToDevice, in));
                MR_HIP_CHECK(hipEventRecord(up, in));
                MR_HIP_CHECK(hipStreamWaitEvent(stream, up, 0));
            }
            p.rays = d_rays + off; p.hits = d_hits + off; p.n = m;
            const mr_status lst = launch_trace(p, flags, stream);
            if (lst != MR_OK) return lst;
            if (!hits_dev) {
                MR_HIP_CHECK(hipEventRecord(done, stream));
                MR_HIP_CHECK(hipStreamWaitEvent(out, done, 0));
                MR_HIP_CHECK(hipMemcpyAsync(hits + off, d_hits + off, m * sizeof(mr_hit), hipMemcpyDeviceToHost, out));
            }
            return MR_OK;
        };
        for (uint64_t k = 0; k < n_chunks && st == MR_OK; k++) st = chunk(k);
        const hipError_t e_in = hipStreamSynchronize(in), e_run = hipStreamSynchronize(stream), e_out = hipStreamSynchronize(out);
        if (st != MR_OK) return st;           // the failing call's message is the one mr_last_error() keeps
        MR_HIP_CHECK(e_in); MR_HIP_CHECK(e_run); MR_HIP_CHECK(e_out);
        return MR_OK;
    }
    if ((st = launch_trace(p, flags, stream)) != MR_OK) return st;
    if (!hits_dev) {
        MR_HIP_CHECK(hipMemcpyAsync(hits, d_hits, n * sizeof(mr_hit), hipMemcpyDeviceToHost, stream));
        MR_HIP_CHECK(hipStreamSynchronize(stream));
    } else if (!rays_dev) {
        MR_HIP_CHECK(hipStreamSynchronize(stream));   // the staged host rays may be reused by the caller
    }
    return MR_OK;
}

mr_status mr_host_alloc(void **ptr, uint64_t bytes) {
    if (!ptr) return fail(MR_ERR_INVALID, "ptr is NULL");
    *ptr = nullptr;
    if (bytes == 0) return MR_OK;
    MR_HIP_CHECK(hipHostMalloc(ptr, bytes, hipHostMallocPortable));
    return MR_OK;
}

mr_status mr_host_free(void *ptr) {
    if (ptr) MR_HIP_CHECK(hipHostFree(ptr));
    return MR_OK;
}

mr_status mr_trace_indirect(mr_scene *s, const mr_ray *d_rays, const uint64_t *d_count, uint64_t max_rays,
                            mr_hit *d_hits, uint32_t flags, void *stream_v) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (max_rays == 0) return MR_OK;
    if (!d_rays || !d_hits || !d_count) return fail(MR_ERR_INVALID, "NULL argument");
    if (misaligned(16, d_rays, d_hits) || misaligned(8, d_count))
        return fail(MR_ERR_INVALID, "device ray/hit buffers must be 16-byte aligned, the count 8-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    TraceParams p = scene_trace_params(s->dev);
    p.rays = d_rays; p.hits = d_hits; p.n = max_rays; p.stats = s->d_stats;
    p.n_dev = reinterpret_cast<const unsigned long long *>(d_count);
    p.work_counter = s->d_work_counters + (s->next_counter.fetch_add(1) % kWorkCounters);
    return launch_trace(p, flags, static_cast<hipStream_t>(stream_v));
}

mr_status mr_order_by_octant(mr_scene *s, const mr_ray *d_rays, const uint8_t *d_octants, uint64_t n, uint32_t chunk_log2,
                             uint32_t *d_order, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (n == 0) return MR_OK;
    if ((!d_rays && !d_octants) || !d_order) return fail(MR_ERR_INVALID, "NULL argument");
    if (misaligned(16, d_rays) || misaligned(4, d_order))
        return fail(MR_ERR_INVALID, "the ray buffer must be 16-byte aligned, the order buffer 4-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_octant_order(d_rays, d_octants, n, chunk_log2 ? chunk_log2 : 14u, d_order, static_cast<hipStream_t>(stream));
}

mr_status mr_trace_grouped(mr_scene *s, const mr_ray *d_rays, const uint8_t *d_octants, uint64_t n, mr_hit *d_hits, uint32_t *d_order,
                           uint32_t chunk_log2, uint32_t flags, void *stream_v) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (n == 0) return MR_OK;
    if (!d_rays || !d_hits || !d_order) return fail(MR_ERR_INVALID, "NULL argument");
    if (misaligned(16, d_rays, d_hits) || misaligned(4, d_order))
        return fail(MR_ERR_INVALID, "device ray/hit buffers must be 16-byte aligned, the order buffer 4-byte aligned");
    if (flags & (MR_MATH_FAST | MR_COUNT_STATS))
        return fail(MR_ERR_INVALID, "mr_trace_grouped: flags may hold MR_TRACE_ANY, MR_MATH_PRODUCT, MR_TRACE_INCOHERENT only");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    MR_HIP_CHECK(hipSetDevice(s->device));
    if (!(chunk_log2 & MR_ORDER_GIVEN)) {
        if (chunk_log2 == 0) chunk_log2 = 14;
        st = launch_octant_order(d_rays, d_octants, n, chunk_log2, d_order, stream);
        if (st != MR_OK) return st;
    }
    TraceParams p = scene_trace_params(s->dev);
    p.rays = d_rays; p.hits = d_hits; p.n = n; p.stats = s->d_stats;
    p.order = d_order;
    return launch_trace(p, flags & ~(uint32_t)(MR_RAYS_ON_DEVICE | MR_HITS_ON_DEVICE | MR_TRACE_PERSISTENT), stream);
}

mr_status mr_trace_get_stats(mr_scene *s, uint64_t *box_tests, uint64_t *tri_tests, int32_t reset) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    unsigned long long h[2] = {0, 0};
    MR_HIP_CHECK(hipDeviceSynchronize());
    MR_HIP_CHECK(hipMemcpy(h, s->d_stats, sizeof(h), hipMemcpyDeviceToHost));
    if (box_tests) *box_tests = h[0];
    if (tri_tests) *tri_tests = h[1];
    if (reset) MR_HIP_CHECK(hipMemset(s->d_stats, 0, sizeof(h)));
    return MR_OK;
}

mr_status mr_gen_eye_rays(mr_scene *s, const mr_camera *cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1,
                          uint32_t spp, uint32_t jitter, uint32_t seed, mr_ray *d_rays, void *stream) {
    if (!s || !cam || !d_rays) return fail(MR_ERR_INVALID, "NULL argument");
    if (W == 0 || H == 0 || spp == 0 || y1 < y0 || y1 > H) return fail(MR_ERR_INVALID, "bad image window");
    if (misaligned(16, d_rays)) return fail(MR_ERR_INVALID, "d_rays must be 16-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_eye_rays(*cam, W, H, y0, y1, spp, jitter, seed, false, d_rays, static_cast<hipStream_t>(stream));
}

mr_status mr_gen_eye_rays_tiled(mr_scene *s, const mr_camera *cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1,
                                uint32_t spp, uint32_t jitter, uint32_t seed, mr_ray *d_rays, void *stream) {
    if (!s || !cam || !d_rays) return fail(MR_ERR_INVALID, "NULL argument");
    if (W == 0 || H == 0 || spp == 0 || y1 < y0 || y1 > H) return fail(MR_ERR_INVALID, "bad image window");
    if ((uint64_t)W * (y1 - y0) > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "window of more than 2^32-1 pixels");
    if (misaligned(16, d_rays)) return fail(MR_ERR_INVALID, "d_rays must be 16-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_eye_rays(*cam, W, H, y0, y1, spp, jitter, seed, true, d_rays, static_cast<hipStream_t>(stream));
}

mr_status mr_tile_pixel_map(uint32_t W, uint32_t rows, uint32_t spp, uint32_t *pixel_of_slot) {
    if (!pixel_of_slot && (uint64_t)W * rows) return fail(MR_ERR_INVALID, "pixel_of_slot is NULL");
    if ((uint64_t)W * rows > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "window of more than 2^32-1 pixels");
    const mr::TileShape t = mr::tile_shape(spp);
    const uint32_t n = W * rows;
    for (uint32_t p = 0; p < n; p++) {
        uint32_t x, yl;
        mr::tile_decode(p, W, rows, t, x, yl);
        pixel_of_slot[p] = yl * W + x;
    }
    return MR_OK;
}

mr_status mr_gen_shadow_rays(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n, const float light[3],
                             mr_ray *d_out, uint32_t *d_src, uint64_t *d_count, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_hits || !d_out || !d_count || !light) return fail(MR_ERR_INVALID, "NULL argument");
    if (n > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "at most 2^32-1 rays per shadow batch");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_shadow_rays(s->dev, d_rays, d_hits, n, light, d_out, d_src,
                              reinterpret_cast<unsigned long long *>(d_count), static_cast<hipStream_t>(stream));
}

mr_status mr_shade_direct(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n, const mr_hit *d_shadow_hits,
                          const uint32_t *d_shadow_src, const uint64_t *d_shadow_count, const mr_light *light,
                          const float diffuse[3], uint32_t spp, float *d_rgb, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_rays || !d_hits || !d_shadow_hits || !d_shadow_src || !d_shadow_count || !light || !diffuse || !d_rgb)
        return fail(MR_ERR_INVALID, "NULL argument");
    if (spp == 0 || n % spp != 0) return fail(MR_ERR_INVALID, "n (%llu) must be a multiple of spp (%u)", (unsigned long long)n, spp);
    // this call shades a uniform material and knows occluders as a flag per ray (opaque occluders, see the header): in a
    // scene with a refractive material the light behind such an occluder is attenuated, not removed (Phong.cpp:99-113) --
    // mr_shade_accumulate (batched) and mr_render_direct / mr_trace_level (one launch) implement that
    if ((st = refuse_textured(s, "mr_shade_direct")) != MR_OK) return st;
    if (s->dev.refractive)
        return fail(MR_ERR_STATE, "mr_shade_direct: the scene has a refractive material; use mr_shade_accumulate, mr_render_direct "
                                  "or mr_trace_level, which let light through refractive occluders as Phong.cpp:99-113 does");
    MR_HIP_CHECK(hipSetDevice(s->device));
    if (n > s->occluded_cap) {     // grow-only scratch; size it with a first call outside any graph capture
        (void)hipFree(s->d_occluded);
        s->d_occluded = nullptr;
        s->occluded_cap = 0;
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&s->d_occluded), n));
        s->occluded_cap = n;
    }
    return launch_shade(s->dev, d_rays, d_hits, n, d_shadow_hits, d_shadow_src,
                        reinterpret_cast<const unsigned long long *>(d_shadow_count), s->d_occluded, *light, diffuse, spp,
                        d_rgb, static_cast<hipStream_t>(stream));
}

mr_status mr_band_locate(uint32_t H, uint32_t band_rows, uint32_t world, uint32_t y, uint32_t *rank, uint32_t *local_row) {
    if (band_rows == 0 || world == 0 || y >= H) return fail(MR_ERR_INVALID, "mr_band_locate: row %u of %u, bands of %u over %u ranks", y, H, band_rows, world);
    const uint32_t band = y / band_rows;
    if (rank) *rank = band % world;
    if (local_row) *local_row = (band / world) * band_rows + y % band_rows;
    return MR_OK;
}

mr_status mr_band_rows_of(uint32_t H, uint32_t band_rows, uint32_t rank, uint32_t world, uint32_t *rows) {
    if (band_rows == 0 || world == 0 || rank >= world || !rows) return fail(MR_ERR_INVALID, "mr_band_rows_of: bad arguments");
    uint32_t n = 0;
    const uint32_t nb = (H + band_rows - 1) / band_rows;
    for (uint32_t b = rank; b < nb; b += world) n += (b + 1) * band_rows <= H ? band_rows : H - b * band_rows;
    *rows = n;
    return MR_OK;
}

mr_status mr_deinterleave_bands(mr_scene *s, const float *d_recv, float *d_full, uint32_t W, uint32_t H, uint32_t band_rows,
                                uint32_t world, uint32_t shard_rows, uint32_t floats_per_pixel, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_recv || !d_full) return fail(MR_ERR_INVALID, "NULL argument");
    if (band_rows == 0 || world == 0 || floats_per_pixel == 0) return fail(MR_ERR_INVALID, "mr_deinterleave_bands: bad band description");
    for (uint32_t r = 0; r < world; r++) {
        uint32_t rows = 0;
        mr_band_rows_of(H, band_rows, r, world, &rows);
        if (rows > shard_rows) return fail(MR_ERR_INVALID, "rank %u owns %u rows, the shards hold %u", r, rows, shard_rows);
    }
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_deinterleave(d_recv, d_full, W, H, band_rows, world, shard_rows, floats_per_pixel, static_cast<hipStream_t>(stream));
}

mr_status mr_render_direct(mr_scene *s, const mr_frame_desc *frame, float *d_rgb, mr_hit *d_hits, mr_hit *d_shadow_hits,
                           uint64_t *d_counts, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!frame || !d_rgb) return fail(MR_ERR_INVALID, "NULL argument");
    if ((st = refuse_textured(s, "mr_render_direct")) != MR_OK) return st;
    if (frame->W == 0 || frame->H == 0) return fail(MR_ERR_INVALID, "empty image");
    if (misaligned(16, d_hits, d_shadow_hits) || misaligned(8, d_counts) || misaligned(4, d_rgb))
        return fail(MR_ERR_INVALID, "hit buffers must be 16-byte aligned, counters 8-byte aligned");
    mr_frame_desc fd = *frame;
    if (fd.band_world <= 1) { fd.band_world = 1; fd.band_rank = 0; if (fd.band_rows == 0) fd.band_rows = 1; }
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_frame(s->dev, fd, d_rgb, d_hits, d_shadow_hits, reinterpret_cast<unsigned long long *>(d_counts),
                        s->d_work_counters + kWorkCounters + (s->next_counter.fetch_add(1) % kWorkCounters), s->eye_tables,
                        static_cast<hipStream_t>(stream));
}

mr_status mr_scene_set_materials(mr_scene *s, const mr_material *mats, uint32_t n_mats, const uint32_t *prim_material) {
    if (!s || !mats || n_mats == 0) return fail(MR_ERR_INVALID, "NULL argument or no materials");
    if (!s->tex.blob.empty())
        return fail(MR_ERR_STATE, "mr_scene_set_materials: the scene's texture table names materials by index; clear it first "
                                  "(mr_scene_set_textures with n_textures = 0) and set it again afterwards");
    const uint32_t nt = s->mesh.n_triangles();
    if (prim_material)
        for (uint32_t i = 0; i < nt; i++)
            if (prim_material[i] >= n_mats) return fail(MR_ERR_INVALID, "triangle %u has material %u of %u", i, prim_material[i], n_mats);
    for (uint32_t i = 0; i < s->mesh.n_planes(); i++)
        if (s->mesh.plane_material[i] >= n_mats)
            return fail(MR_ERR_INVALID, "plane %u has material %u of %u", i, s->mesh.plane_material[i], n_mats);
    s->materials.resize(11 * (size_t)n_mats);
    for (uint32_t i = 0; i < n_mats; i++) {
        float *o = &s->materials[11 * (size_t)i];
        // energy balance of the Phong constructor (Phong.cpp:12-33)
        for (int c = 0; c < 3; c++) {
            const float ks = mats[i].specular[c];
            const float kt = fmaxf(fminf(mats[i].transmission[c], 1.0f - ks), 0.f);
            const float kd = fmaxf(fminf(mats[i].diffuse[c], 1.0f - ks - kt), 0.f);
            o[c] = kd; o[3 + c] = ks; o[6 + c] = kt;
        }
        o[9] = mats[i].shininess;
        o[10] = mats[i].refract_index;
    }
    if (prim_material) s->prim_material.assign(prim_material, prim_material + nt);
    else s->prim_material.clear();
    if (s->on_device) {
        MR_HIP_CHECK(hipSetDevice(s->device));
        MR_HIP_CHECK(hipDeviceSynchronize());
        return upload_materials(s);
    }
    return MR_OK;
}

// the scene's per-ray light-scale buffer, grown to n floats
static mr_status reserve_light_scale(mr_scene *s, uint64_t n) {
    if (n <= s->light_scale_cap) return MR_OK;
    (void)hipFree(s->d_light_scale);
    s->d_light_scale = nullptr;
    s->light_scale_cap = 0;
    MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&s->d_light_scale), n * sizeof(float)));
    s->light_scale_cap = n;
    return MR_OK;
}

// what mr_shade_accumulate and mr_shade_accumulate_surface ask first, in this order.  surface_null: one of the buffers that the
// _surface call takes besides is NULL
static mr_status check_shade_accumulate(const char *who, mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, bool surface_null,
                                        const mr_ray *d_shadow_rays, const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src,
                                        const uint64_t *d_shadow_count, const mr_light *light, uint32_t spp, const float *d_rgb) {
    const mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_rays || !d_hits || surface_null || !d_shadow_rays || !d_shadow_hits || !d_shadow_src || !d_shadow_count || !light || !d_rgb)
        return fail(MR_ERR_INVALID, "%s: NULL argument", who);
    if (spp == 0) return fail(MR_ERR_INVALID, "%s: spp is 0", who);
    return MR_OK;
}

mr_status mr_shade_accumulate(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                              const uint32_t *d_pixels, uint64_t n, const mr_ray *d_shadow_rays, const mr_hit *d_shadow_hits,
                              const uint32_t *d_shadow_src, const uint64_t *d_shadow_count, const mr_light *light, uint32_t spp,
                              float *d_rgb, void *stream) {
    mr_status st = check_shade_accumulate("mr_shade_accumulate", s, d_rays, d_hits, false, d_shadow_rays, d_shadow_hits, d_shadow_src,
                                          d_shadow_count, light, spp, d_rgb);
    if (st != MR_OK) return st;
    if ((st = refuse_procedural(s, "mr_shade_accumulate", "mr_shade_accumulate_surface")) != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    if ((st = reserve_light_scale(s, n)) != MR_OK) return st;
    TexParams tex;
    const bool textured = !s->tex.blob.empty();
    if (textured && (st = texture_params(s, static_cast<hipStream_t>(stream), tex)) != MR_OK) return st;
    return launch_shade_accumulate(s->dev, d_rays, d_hits, d_weights, d_pixels, n, d_shadow_rays, d_shadow_hits, d_shadow_src,
                                   reinterpret_cast<const unsigned long long *>(d_shadow_count), s->d_light_scale, *light, spp,
                                   d_rgb, textured ? &tex : nullptr, static_cast<hipStream_t>(stream));
}

// What mr_gen_secondary_rays and mr_gen_secondary_rays_surface ask, in this order.  surface: the _surface call, which takes
// d_normal besides and reads every hit's N from it, so that a reflective STONE material is no reason to refuse.
static mr_status check_gen_secondary_rays(const char *who, bool surface, mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits,
                                          const float *d_normal, uint64_t n, uint32_t spp, const mr_ray *d_out_rays,
                                          const float *d_out_weights, const uint32_t *d_out_pixels, const uint64_t *d_count,
                                          uint64_t out_capacity) {
    const mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_rays || !d_hits || !d_out_rays || !d_out_weights || !d_out_pixels || !d_count) return fail(MR_ERR_INVALID, "NULL argument");
    if (spp == 0) return fail(MR_ERR_INVALID, "spp is 0");
    if (n / spp > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "too many pixels");
    if (out_capacity == 0 && n > 0) return fail(MR_ERR_INVALID, "%s: out_capacity is 0 (room for 3n rays always suffices)", who);
    if (surface && !d_normal) return fail(MR_ERR_INVALID, "%s: d_normal is NULL", who);
    if (surface && misaligned(4, d_normal)) return fail(MR_ERR_INVALID, "%s: d_normal must be 4-byte aligned", who);
    if (!surface && s->tex.bumped_specular)                   // Ray::reflect bounces about N, which this call does not bump
        return fail(MR_ERR_STATE, "%s: a material of the scene names a STONE texture and has a non-zero ks (its mirror child bounces "
                                  "about the bump-mapped normal, which this call does not have; mr_gen_secondary_rays_surface reads "
                                  "mr_hit_surface's normal)", who);
    return MR_OK;
}

mr_status mr_gen_secondary_rays(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                                const uint32_t *d_pixels, uint64_t n, uint32_t spp, mr_ray *d_out_rays, float *d_out_weights,
                                uint32_t *d_out_pixels, uint64_t *d_count, uint64_t out_capacity, uint8_t *d_out_octants, void *stream) {
    const mr_status st = check_gen_secondary_rays("mr_gen_secondary_rays", false, s, d_rays, d_hits, nullptr, n, spp, d_out_rays,
                                                  d_out_weights, d_out_pixels, d_count, out_capacity);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_secondary_rays(s->dev, d_rays, d_hits, d_weights, d_pixels, n, spp, d_out_rays, d_out_weights, d_out_pixels,
                                 reinterpret_cast<unsigned long long *>(d_count), out_capacity, d_out_octants, static_cast<hipStream_t>(stream));
}

// ... about the normal Scene::trace hands on (include/miro_hip_bump.h, mr_bump_surface.hip)
mr_status mr_gen_secondary_rays_surface(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_normal,
                                        const float *d_weights, const uint32_t *d_pixels, uint64_t n, uint32_t spp, mr_ray *d_out_rays,
                                        float *d_out_weights, uint32_t *d_out_pixels, uint64_t *d_count, uint64_t out_capacity,
                                        uint8_t *d_out_octants, void *stream) {
    const mr_status st = check_gen_secondary_rays("mr_gen_secondary_rays_surface", true, s, d_rays, d_hits, d_normal, n, spp, d_out_rays,
                                                  d_out_weights, d_out_pixels, d_count, out_capacity);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_secondary_rays_surface(s->dev, d_rays, d_hits, d_normal, d_weights, d_pixels, n, spp, d_out_rays, d_out_weights,
                                         d_out_pixels, reinterpret_cast<unsigned long long *>(d_count), out_capacity, d_out_octants,
                                         static_cast<hipStream_t>(stream));
}

// What mr_gen_path_rays and mr_gen_path_rays_surface ask, in this order.  surface: the _surface call, which takes d_color /
// d_normal besides and reads every hit's N from the second, so that a procedural texture is no reason to refuse.
static mr_status check_gen_path_rays(const char *who, bool surface, mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits,
                                     const float *d_color, const float *d_normal, uint64_t n, uint32_t spp, uint32_t kinds,
                                     const mr_ray *d_out_rays, const float *d_out_weights, const uint32_t *d_out_pixels,
                                     const uint64_t *d_count, uint64_t out_capacity) {
    const mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_rays || !d_hits || !d_out_rays || !d_out_weights || !d_out_pixels || !d_count) return fail(MR_ERR_INVALID, "NULL argument");
    if (surface && !d_color) return fail(MR_ERR_INVALID, "%s: d_color is NULL", who);
    if (surface && !d_normal) return fail(MR_ERR_INVALID, "%s: d_normal is NULL", who);
    if (surface && misaligned(4, d_color)) return fail(MR_ERR_INVALID, "%s: d_color must be 4-byte aligned", who);
    if (surface && misaligned(4, d_normal)) return fail(MR_ERR_INVALID, "%s: d_normal must be 4-byte aligned", who);
    if (spp == 0) return fail(MR_ERR_INVALID, "spp is 0");
    if (n / spp > 0xFFFFFFFFull || n > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "too many rays for 32-bit ray ids");
    if (kinds == 0 || (kinds & ~7u)) return fail(MR_ERR_INVALID, "kinds must be a combination of MR_PATH_MIRROR | MR_PATH_REFRACT | MR_PATH_DIFFUSE");
    if (out_capacity == 0 && n > 0) return fail(MR_ERR_INVALID, "%s: out_capacity is 0 (room for 4n rays always suffices)", who);
    if (!surface && (kinds & 4u) && s->tex.procedural)        // MR_PATH_DIFFUSE: Ray::random bounces about N, which this call does not bump
        return fail(MR_ERR_STATE, "%s: MR_PATH_DIFFUSE on a scene whose texture table holds a procedural texture (STONE, STEM, "
                                  "PETAL, LEAF or FLOWER_CENTER; Ray::random bounces about the un-bumped N here; mr_gen_path_rays_surface "
                                  "reads mr_hit_surface's normal and colour)", who);
    if (!surface && (kinds & 1u) && s->tex.bumped_specular)   // MR_PATH_MIRROR: the lobe lies about Ray::reflect's direction, likewise
        return fail(MR_ERR_STATE, "%s: MR_PATH_MIRROR on a scene with a material that names a STONE texture and has a non-zero ks (its "
                                  "mirror child bounces about the bump-mapped normal, which this call does not have; "
                                  "mr_gen_path_rays_surface reads mr_hit_surface's normal and colour)", who);
    return MR_OK;
}

mr_status mr_gen_path_rays(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights,
                           const uint32_t *d_pixels, const uint32_t *d_ids, uint64_t n, uint32_t spp, uint32_t seed,
                           uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                           uint32_t *d_out_ids, uint64_t *d_count, uint64_t out_capacity, uint8_t *d_out_octants, void *stream) {
    const mr_status st = check_gen_path_rays("mr_gen_path_rays", false, s, d_rays, d_hits, nullptr, nullptr, n, spp, kinds, d_out_rays,
                                             d_out_weights, d_out_pixels, d_count, out_capacity);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_path_rays(s->dev, d_rays, d_hits, d_weights, d_pixels, d_ids, n, spp, seed, bounce, kinds, d_out_rays,
                            d_out_weights, d_out_pixels, d_out_ids, reinterpret_cast<unsigned long long *>(d_count), out_capacity,
                            d_out_octants, static_cast<hipStream_t>(stream));
}

mr_status mr_gen_path_rays_surface(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color, const float *d_normal,
                                   const float *d_weights, const uint32_t *d_pixels, const uint32_t *d_ids, uint64_t n, uint32_t spp,
                                   uint32_t seed, uint32_t bounce, uint32_t kinds, mr_ray *d_out_rays, float *d_out_weights,
                                   uint32_t *d_out_pixels, uint32_t *d_out_ids, uint64_t *d_count, uint64_t out_capacity,
                                   uint8_t *d_out_octants, void *stream) {
    const mr_status st = check_gen_path_rays("mr_gen_path_rays_surface", true, s, d_rays, d_hits, d_color, d_normal, n, spp, kinds,
                                             d_out_rays, d_out_weights, d_out_pixels, d_count, out_capacity);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_path_rays_surface(s->dev, d_rays, d_hits, d_color, d_normal, d_weights, d_pixels, d_ids, n, spp, seed, bounce, kinds,
                                    d_out_rays, d_out_weights, d_out_pixels, d_out_ids, reinterpret_cast<unsigned long long *>(d_count),
                                    out_capacity, d_out_octants, static_cast<hipStream_t>(stream));
}

mr_status mr_trace_level(mr_scene *s, const mr_level_desc *level, const mr_ray *d_rays, const float *d_weights,
                         const uint32_t *d_pixels, const uint32_t *d_ids, uint64_t n, float *d_rgb, mr_ray *d_out_rays,
                         float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids, uint64_t *d_out_count,
                         uint64_t *d_counts, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!level || !d_rays || !d_rgb) return fail(MR_ERR_INVALID, "NULL argument");
    if ((st = refuse_textured(s, "mr_trace_level")) != MR_OK) return st;
    if (level->children > MR_LEVEL_PATH) return fail(MR_ERR_INVALID, "mr_trace_level: children must be MR_LEVEL_LAST, _SPECULAR or _PATH");
    if (level->children != MR_LEVEL_LAST && (!d_out_rays || !d_out_weights || !d_out_pixels || !d_out_count))
        return fail(MR_ERR_INVALID, "mr_trace_level: a level with children needs the output queue");
    if (level->children != MR_LEVEL_LAST && n > 0 && level->out_capacity_lo == 0 && level->out_capacity_hi == 0)
        return fail(MR_ERR_INVALID, "mr_trace_level: out_capacity is 0 (room for %un rays always suffices)", level->children == MR_LEVEL_PATH ? 4u : 3u);
    if (level->spp == 0) return fail(MR_ERR_INVALID, "spp is 0");
    if (n > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "mr_trace_level: at most 2^32 - 1 rays per call");
    if (level->children == MR_LEVEL_PATH && (level->path_kinds == 0 || (level->path_kinds & ~7u)))
        return fail(MR_ERR_INVALID, "path_kinds must be a combination of MR_PATH_MIRROR | MR_PATH_REFRACT | MR_PATH_DIFFUSE");
    if (level->flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT))
        return fail(MR_ERR_INVALID, "mr_trace_level: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT only");
    if (misaligned(16, d_rays, d_out_rays) || misaligned(8, d_out_count, d_counts))
        return fail(MR_ERR_INVALID, "ray queues must be 16-byte aligned, counters 8-byte aligned");
    if (level->reserved != 0) return fail(MR_ERR_INVALID, "mr_level_desc.reserved must be 0");
    if (misaligned(4, level->d_order)) return fail(MR_ERR_INVALID, "mr_level_desc.d_order must be 4-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_level(s->dev, *level, d_rays, d_weights, d_pixels, d_ids, n, d_rgb, d_out_rays, d_out_weights, d_out_pixels,
                        d_out_ids, reinterpret_cast<unsigned long long *>(d_out_count),
                        reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
}

mr_status mr_scene_set_lights(mr_scene *s, const mr_light_desc *lights, uint32_t n_lights) {
    if (!s) return fail(MR_ERR_INVALID, "mr_scene_set_lights: NULL scene");
    if (n_lights > MR_MAX_LIGHTS) return fail(MR_ERR_INVALID, "mr_scene_set_lights: %u lights, at most %u", n_lights, (unsigned)MR_MAX_LIGHTS);
    if (n_lights > 0 && !lights) return fail(MR_ERR_INVALID, "mr_scene_set_lights: NULL list of %u lights", n_lights);
    std::vector<ShadeLight> list(n_lights);
    for (uint32_t i = 0; i < n_lights; i++) {
        const mr_light_desc &in = lights[i];
        if (in.kind != MR_LIGHT_POINT && in.kind != MR_LIGHT_DISC) return fail(MR_ERR_INVALID, "light %u: unknown kind %u", i, in.kind);
        const mr_status st = check_light("mr_scene_set_lights", i, in.reserved, in.position, in.color, in.wattage,
                                         in.kind == MR_LIGHT_DISC ? in.normal : nullptr);
        if (st != MR_OK) return st;
        ShadeLight &o = list[i];
        o = ShadeLight();
        o.kind = in.kind;
        for (int c = 0; c < 3; c++) { o.position[c] = in.position[c]; o.color[c] = in.color[c]; }
        o.wattage = in.wattage;
        if (in.kind == MR_LIGHT_DISC) {
            if (!(in.radius > 0.0f) || !std::isfinite(in.radius)) return fail(MR_ERR_INVALID, "light %u: a disc light's radius must be positive", i);
            for (int c = 0; c < 3; c++) o.normal[c] = in.normal[c];
            o.radius = in.radius;
        }
    }
    s->lights.swap(list);
    return MR_OK;
}

// what mr_shade_lights and mr_shade_lights_surface ask of the scene and of their arguments, in this order.  surface_null /
// surface_misaligned: one of the buffers that the _surface call takes besides is
static mr_status check_shade_lights(const char *who, mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, bool surface_null,
                                    bool surface_misaligned, uint64_t n, uint32_t spp, uint32_t flags, const float *d_rgb,
                                    const float *d_ray_rgb, const uint64_t *d_counts) {
    const mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (s->lights.empty()) return fail(MR_ERR_STATE, "%s: the scene has no lights (mr_scene_set_lights)", who);
    if (!d_rays || !d_hits || surface_null || (!d_rgb && !d_ray_rgb)) return fail(MR_ERR_INVALID, "%s: NULL argument", who);
    if (spp == 0) return fail(MR_ERR_INVALID, "%s: spp is 0", who);
    if (n / spp > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "%s: too many pixels", who);
    if (flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT | MR_TRACE_ANY))
        return fail(MR_ERR_INVALID, "%s: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT, MR_TRACE_ANY only", who);
    if ((flags & MR_TRACE_ANY) && s->dev.refractive)
        return fail(MR_ERR_STATE, "%s: MR_TRACE_ANY with a refractive material (the nearest occluder decides, Phong.cpp:99-113)", who);
    if (misaligned(16, d_rays, d_hits) || misaligned(8, d_counts) || misaligned(4, d_rgb, d_ray_rgb) || surface_misaligned)
        return fail(MR_ERR_INVALID, "%s: ray / hit buffers must be 16-byte aligned, float buffers 4-byte, counters 8-byte aligned", who);
    return MR_OK;
}

mr_status mr_shade_lights(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels,
                          uint64_t n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb, uint64_t *d_counts, void *stream) {
    mr_status st = check_shade_lights("mr_shade_lights", s, d_rays, d_hits, false, false, n, spp, flags, d_rgb, d_ray_rgb, d_counts);
    if (st != MR_OK) return st;
    if ((st = refuse_procedural(s, "mr_shade_lights", "mr_shade_lights_surface")) != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    if (!s->tex.blob.empty()) {
        TexParams tex;
        if ((st = texture_params(s, static_cast<hipStream_t>(stream), tex)) != MR_OK) return st;
        return launch_shade_lights_tex(s->dev, tex, s->lights.data(), (uint32_t)s->lights.size(), d_rays, d_hits, d_weights, d_pixels, n,
                                       spp, flags, d_rgb, d_ray_rgb, reinterpret_cast<unsigned long long *>(d_counts),
                                       static_cast<hipStream_t>(stream));
    }
    return launch_shade_lights(s->dev, s->lights.data(), (uint32_t)s->lights.size(), d_rays, d_hits, d_weights, d_pixels, n, spp,
                               flags, d_rgb, d_ray_rgb, reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
}

// the environment on the device, its texel records uploaded on `stream` by the first call after a change (e.rec stays until the
// next change); `p`: as the kernels take it.  For mr_shade_environment and mr_render_lights_environment, as texture_params is
// for the calls that read the texture table
static mr_status environment_params(mr_scene *s, hipStream_t stream, EnvParams &p) {
    const HostEnvironment &e = s->env;
    if (s->env_dirty) {
        (void)hipFree(s->d_env);
        s->d_env = nullptr;
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&s->d_env), e.rec.size() * sizeof(float)));
        MR_HIP_CHECK(hipMemcpyAsync(s->d_env, e.rec.data(), e.rec.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        s->env_dirty = false;
    }
    p = EnvParams{};
    if (e.W) {
        p.full = s->d_env; p.low = s->d_env + (size_t)e.W * e.H;
        p.W = e.W; p.H = e.H; p.lw = e.lw; p.lh = e.lh;
        p.max_intensity = e.max_intensity;
    }
    p.rot[0] = e.rot[0]; p.rot[1] = e.rot[1];
    for (int c = 0; c < 3; c++) p.bg[c] = e.bg[c];
    return MR_OK;
}

// the scene as the textured light-list kernels take it, after the call's state checks: its device made current, its texture table
// or none, with `environment` its environment (without: all zero), and its light list.  The two uploads happen only after a
// change (texture_params, environment_params) and must lie outside a stream capture
static mr_status lights_scene_params(mr_scene *s, bool environment, void *stream, LightScene &ls) {
    MR_HIP_CHECK(hipSetDevice(s->device));
    mr_status st = MR_OK;
    ls.ds = &s->dev;
    ls.lights = s->lights.data();
    ls.n_lights = (uint32_t)s->lights.size();
    ls.bumped_specular = s->tex.bumped_specular;
    TexParams &tex = ls.tex;
    tex.recs = nullptr; tex.texels = nullptr; tex.mat_tex = nullptr; tex.texcoords = s->dev.texcoords; tex.ti = s->dev.ti;
    if (!s->tex.blob.empty() && (st = texture_params(s, static_cast<hipStream_t>(stream), tex)) != MR_OK) return st;
    ls.env = EnvParams{};
    return environment ? environment_params(s, static_cast<hipStream_t>(stream), ls.env) : MR_OK;
}

// mr_render_direct's window over mr_shade_lights' light list, in one launch (mr_frame_lights.hip).  What the arguments alone can
// get wrong is answered first, before any device call and before the scene's state is read; then the scene's state.
// What mr_render_lights and mr_render_lights_surface ask of their arguments and of the scene, in this order; `fd`: the
// descriptor as the launchers take it (band_world >= 1).  surface_misaligned: one of the buffers that the _surface call takes
// besides is; refuse_table: the call shades without the lookup.
// (the two halves: what the arguments alone can get wrong; then the scene's state.  mr_render_level_lights puts its own
// argument checks between them)
// the frame's own part of them, which mr_render_recursion_photons_workspace asks without a scene: a non-empty image, `fd` as
// the launchers take it, check_frame_lights
static mr_status check_render_lights_frame(const char *who, const mr_frame_desc &frame, mr_frame_desc &fd) {
    if (frame.W == 0 || frame.H == 0) return fail(MR_ERR_INVALID, "%s: empty image", who);
    fd = frame;
    if (fd.band_world <= 1) { fd.band_world = 1; fd.band_rank = 0; if (fd.band_rows == 0) fd.band_rows = 1; }
    return check_frame_lights(who, fd);
}
static mr_status check_render_lights_args(const char *who, mr_scene *s, const mr_frame_desc *frame, mr_frame_desc &fd, const float *d_rgb,
                                          const mr_hit *d_hits, const float *d_sample_rgb, bool surface_misaligned, const uint64_t *d_counts) {
    if (!s || !frame || !d_rgb) return fail(MR_ERR_INVALID, "%s: NULL argument", who);
    const mr_status st = check_render_lights_frame(who, *frame, fd);
    if (st != MR_OK) return st;
    if (misaligned(16, d_hits) || misaligned(8, d_counts) || misaligned(4, d_rgb, d_sample_rgb) || surface_misaligned)
        return fail(MR_ERR_INVALID, "%s: the hit buffer must be 16-byte aligned, float buffers 4-byte, counters 8-byte aligned", who);
    return MR_OK;
}
static mr_status check_render_lights_state(const char *who, mr_scene *s, const mr_frame_desc &fd, bool refuse_table) {
    const mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (s->lights.empty()) return fail(MR_ERR_STATE, "%s: the scene has no lights (mr_scene_set_lights)", who);
    if (refuse_table && !s->tex.blob.empty())
        return fail(MR_ERR_STATE, "%s: the scene has a texture table (mr_scene_set_textures) and this call shades without "
                                  "the lookup; use the batched calls mr_trace -> mr_shade_lights, or mr_trace -> mr_hit_surface -> "
                                  "mr_shade_lights_surface", who);
    if ((fd.flags & MR_TRACE_ANY) && s->dev.refractive)
        return fail(MR_ERR_STATE, "%s: MR_TRACE_ANY with a refractive material (the nearest occluder decides, Phong.cpp:99-113)", who);
    return MR_OK;
}
static mr_status check_render_lights(const char *who, mr_scene *s, const mr_frame_desc *frame, mr_frame_desc &fd, const float *d_rgb,
                                     const mr_hit *d_hits, const float *d_sample_rgb, bool surface_misaligned, const uint64_t *d_counts,
                                     bool refuse_table) {
    const mr_status st = check_render_lights_args(who, s, frame, fd, d_rgb, d_hits, d_sample_rgb, surface_misaligned, d_counts);
    return st != MR_OK ? st : check_render_lights_state(who, s, fd, refuse_table);
}

mr_status mr_render_lights(mr_scene *s, const mr_frame_desc *frame, float *d_rgb, mr_hit *d_hits, float *d_sample_rgb,
                           uint64_t *d_counts, void *stream) {
    mr_frame_desc fd;
    const mr_status st = check_render_lights("mr_render_lights", s, frame, fd, d_rgb, d_hits, d_sample_rgb, false, d_counts, true);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_frame_lights(s->dev, s->lights.data(), (uint32_t)s->lights.size(), fd, d_rgb, d_hits, d_sample_rgb,
                               reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
}

// ... on any scene: with a texture table every hit's diffuse colour and normal are hit_color_normal's (mr_frame_lights_surface.hip).
// The first call after mr_scene_set_textures uploads the table (texture_params: an allocation and a copy) and must lie outside a
// stream capture; after it the call is one kernel on `stream`.
mr_status mr_render_lights_surface(mr_scene *s, const mr_frame_desc *frame, float *d_rgb, mr_hit *d_hits, float *d_sample_rgb,
                                   float *d_sample_color, float *d_sample_normal, uint64_t *d_counts, void *stream) {
    mr_frame_desc fd;
    mr_status st = check_render_lights("mr_render_lights_surface", s, frame, fd, d_rgb, d_hits, d_sample_rgb,
                                       misaligned(4, d_sample_color, d_sample_normal), d_counts, false);
    if (st != MR_OK) return st;
    LightScene ls;
    if ((st = lights_scene_params(s, false, stream, ls)) != MR_OK) return st;
    const FrameOutputs o = {d_rgb, d_hits, d_sample_rgb, d_sample_color, d_sample_normal, reinterpret_cast<unsigned long long *>(d_counts)};
    return launch_frame_lights_surface(ls, fd, o, static_cast<hipStream_t>(stream));
}

// Level 0 of the light-list frame with the environment, whichever call asks for it; the only caller of its three launchers.  A lens
// (optional) selects the thin-lens frame (mr_frame_lens.hip), with or without children; without a lens, ld.children ==
// MR_LEVEL_LAST is the plain frame (mr_frame_lights_env.hip), which reads neither `out` nor d_out_count, and a level with children
// the frame that emits them into `out` (mr_frame_level_lights.hip).  who: the entry point the lens frame's window messages name
static mr_status launch_level0_lights(const char *who, const LightScene &ls, const mr_frame_desc &fd, const mr_lens_desc *lens,
                                      const mr_frame_level_desc &ld, const FrameOutputs &o, const RayQueue &out,
                                      unsigned long long *d_out_count, hipStream_t stream) {
    if (lens) return launch_frame_lens(who, ls, fd, *lens, ld, o, out, d_out_count, stream);
    if (ld.children == MR_LEVEL_LAST) return launch_frame_lights_env(ls, fd, o, stream);
    return launch_frame_level_lights(ls, fd, ld, o, out, d_out_count, stream);
}

// ... and a live sample whose primary ray misses is worth the scene's environment (mr_frame_lights_env.hip).  The first call after
// mr_scene_set_environment with an image uploads it (environment_params: an allocation and a copy), as the first call after
// mr_scene_set_textures uploads the table; both must lie outside a stream capture.  After them the call is one kernel on `stream`.
mr_status mr_render_lights_environment(mr_scene *s, const mr_frame_desc *frame, float *d_rgb, mr_hit *d_hits, float *d_sample_rgb,
                                       float *d_sample_color, float *d_sample_normal, uint64_t *d_counts, void *stream) {
    mr_frame_desc fd;
    mr_status st = check_render_lights("mr_render_lights_environment", s, frame, fd, d_rgb, d_hits, d_sample_rgb,
                                       misaligned(4, d_sample_color, d_sample_normal), d_counts, false);
    if (st != MR_OK) return st;
    LightScene ls;
    if ((st = lights_scene_params(s, true, stream, ls)) != MR_OK) return st;
    const FrameOutputs o = {d_rgb, d_hits, d_sample_rgb, d_sample_color, d_sample_normal, reinterpret_cast<unsigned long long *>(d_counts)};
    mr_frame_level_desc last = {};
    last.children = MR_LEVEL_LAST;
    return launch_level0_lights("mr_render_lights_environment", ls, fd, nullptr, last, o, RayQueue{}, nullptr, static_cast<hipStream_t>(stream));
}

// what the three calls that emit children ask of the queue they fill, in this order: the queue and its capacity with children
// (fan: children at most per ray or sample, n of which the call runs), and n itself.  no_queue, no_room, too_many: the call's own
// three refusals, formats over (who), (who, fan) and (who)
static mr_status check_out_queue(const char *who, const char *no_queue, const char *no_room, const char *too_many, bool children,
                                 unsigned fan, uint32_t capacity_lo, uint32_t capacity_hi, uint64_t n, const mr_ray *d_out_rays,
                                 const float *d_out_weights, const uint32_t *d_out_pixels, const uint64_t *d_out_count) {
    if (children && (!d_out_rays || !d_out_weights || !d_out_pixels || !d_out_count)) return fail(MR_ERR_INVALID, no_queue, who);
    if (children && n > 0 && capacity_lo == 0 && capacity_hi == 0) return fail(MR_ERR_INVALID, no_room, who, fan);
    if (n > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, too_many, who);
    return MR_OK;
}

// what mr_trace_level_lights and mr_trace_level_lights_path ask of their queues after the descriptor's own words, in this order:
// check_out_queue, then the alignments.  more_misaligned: one of the buffers that the _path call takes besides is
static mr_status check_level_lights_queue(const char *who, bool children, unsigned fan, uint32_t capacity_lo, uint32_t capacity_hi,
                                          const mr_ray *d_rays, const float *d_weights, const uint32_t *d_pixels, uint64_t n,
                                          const float *d_rgb, const mr_hit *d_hits, const float *d_ray_rgb, const float *d_color,
                                          const float *d_normal, const mr_ray *d_out_rays, const float *d_out_weights,
                                          const uint32_t *d_out_pixels, const uint64_t *d_out_count, const uint64_t *d_counts,
                                          bool more_misaligned) {
    const mr_status st = check_out_queue(who, "%s: a level with children needs the output queue",
                                         "%s: out_capacity is 0 (room for %un rays always suffices)", "%s: at most 2^32 - 1 rays per call",
                                         children, fan, capacity_lo, capacity_hi, n, d_out_rays, d_out_weights, d_out_pixels, d_out_count);
    if (st != MR_OK) return st;
    if (misaligned(16, d_rays, d_out_rays, d_hits) || misaligned(8, d_out_count, d_counts) ||
        misaligned(4, d_weights, d_pixels, d_rgb, d_ray_rgb, d_color, d_normal, d_out_weights, d_out_pixels) || more_misaligned)
        return fail(MR_ERR_INVALID, "%s: ray queues and the hit buffer must be 16-byte aligned, counters 8-byte, float and index buffers "
                                    "4-byte aligned", who);
    return MR_OK;
}

// ... and of the scene, after the arguments: built on a device, with lights; then lights_scene_params
static mr_status level_lights_params(const char *who, mr_scene *s, bool environment, void *stream, LightScene &ls) {
    const mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (s->lights.empty()) return fail(MR_ERR_STATE, "%s: the scene has no lights (mr_scene_set_lights)", who);
    return lights_scene_params(s, environment, stream, ls);
}

// One level of the recursion over the light list on any scene, in one launch (mr_level_lights.hip).  What the arguments alone can
// get wrong is answered first, before any device call and before the scene's state is read; then the scene's state; then the two
// uploads of mr_render_lights_environment (texture table, environment image: outside a stream capture), each only after a change.
mr_status mr_trace_level_lights(mr_scene *s, const mr_level_lights_desc *level, const mr_ray *d_rays, const float *d_weights,
                                const uint32_t *d_pixels, uint64_t n, float *d_rgb, mr_hit *d_hits, float *d_ray_rgb, float *d_color,
                                float *d_normal, mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels,
                                uint64_t *d_out_count, uint64_t *d_counts, void *stream) {
    const char *who = "mr_trace_level_lights";
    if (!s || !level || !d_rays) return fail(MR_ERR_INVALID, "%s: NULL argument (scene, level and d_rays are required)", who);
    if (!d_rgb && !d_ray_rgb) return fail(MR_ERR_INVALID, "%s: NULL argument (d_rgb and d_ray_rgb are both NULL)", who);
    if (level->spp == 0) return fail(MR_ERR_INVALID, "%s: spp is 0", who);
    if (level->flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT))
        return fail(MR_ERR_INVALID, "%s: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT only", who);
    if (level->children == MR_LEVEL_PATH)
        return fail(MR_ERR_INVALID, "%s: children == MR_LEVEL_PATH: the path-traced generators stay batched, "
                                    "mr_gen_path_rays or mr_gen_path_rays_surface after a level with MR_LEVEL_LAST", who);
    if (level->children != MR_LEVEL_LAST && level->children != MR_LEVEL_SPECULAR)
        return fail(MR_ERR_INVALID, "%s: children must be MR_LEVEL_LAST or MR_LEVEL_SPECULAR", who);
    if (level->environment > 1) return fail(MR_ERR_INVALID, "%s: environment must be 0 or 1", who);
    for (int k = 0; k < 6; k++)
        if (level->reserved[k] != 0) return fail(MR_ERR_INVALID, "%s: mr_level_lights_desc.reserved must be 0", who);
    mr_status st = check_level_lights_queue(who, level->children != MR_LEVEL_LAST, 3u, level->out_capacity_lo, level->out_capacity_hi, d_rays,
                                            d_weights, d_pixels, n, d_rgb, d_hits, d_ray_rgb, d_color, d_normal, d_out_rays, d_out_weights,
                                            d_out_pixels, d_out_count, d_counts, false);
    if (st != MR_OK) return st;
    LightScene ls;
    if ((st = level_lights_params(who, s, level->environment != 0, stream, ls)) != MR_OK) return st;
    return launch_level_lights(ls, *level, d_rays, d_weights, d_pixels, n, d_rgb, d_hits, d_ray_rgb, d_color, d_normal, d_out_rays,
                               d_out_weights, d_out_pixels, reinterpret_cast<unsigned long long *>(d_out_count),
                               reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
}

// ... of a PATH_TRACING build (mr_level_lights_path.hip): the children of mr_gen_path_rays_surface, ids, the low-res byte.  The
// checks, their order and the uploads are mr_trace_level_lights', under this call's name; the two byte masks take any address.
mr_status mr_trace_level_lights_path(mr_scene *s, const mr_level_lights_path_desc *level, const mr_ray *d_rays, const float *d_weights,
                                     const uint32_t *d_pixels, const uint32_t *d_ids, uint64_t n, float *d_rgb, mr_hit *d_hits,
                                     float *d_ray_rgb, float *d_color, float *d_normal, mr_ray *d_out_rays, float *d_out_weights,
                                     uint32_t *d_out_pixels, uint32_t *d_out_ids, uint64_t *d_out_count, uint64_t *d_counts,
                                     void *stream) {
    const char *who = "mr_trace_level_lights_path";
    if (!s || !level || !d_rays) return fail(MR_ERR_INVALID, "%s: NULL argument (scene, level and d_rays are required)", who);
    if (!d_rgb && !d_ray_rgb) return fail(MR_ERR_INVALID, "%s: NULL argument (d_rgb and d_ray_rgb are both NULL)", who);
    if (level->spp == 0) return fail(MR_ERR_INVALID, "%s: spp is 0", who);
    if (level->flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT | MR_ENV_LOWRES))
        return fail(MR_ERR_INVALID, "%s: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT, MR_ENV_LOWRES only", who);
    if (level->children == MR_LEVEL_SPECULAR)
        return fail(MR_ERR_INVALID, "%s: children == MR_LEVEL_SPECULAR: the specular children are mr_trace_level_lights'", who);
    if (level->children != MR_LEVEL_LAST && level->children != MR_LEVEL_PATH)
        return fail(MR_ERR_INVALID, "%s: children must be MR_LEVEL_LAST or MR_LEVEL_PATH", who);
    if (level->environment > 1) return fail(MR_ERR_INVALID, "%s: environment must be 0 or 1", who);
    if (level->children == MR_LEVEL_PATH && (level->path_kinds == 0 || (level->path_kinds & ~7u)))
        return fail(MR_ERR_INVALID, "%s: path_kinds must be a combination of MR_PATH_MIRROR | MR_PATH_REFRACT | MR_PATH_DIFFUSE", who);
    for (int k = 0; k < 5; k++)
        if (level->reserved[k] != 0) return fail(MR_ERR_INVALID, "%s: mr_level_lights_path_desc.reserved must be 0", who);
    mr_status st = check_level_lights_queue(who, level->children != MR_LEVEL_LAST, 4u, level->out_capacity_lo, level->out_capacity_hi, d_rays,
                                            d_weights, d_pixels, n, d_rgb, d_hits, d_ray_rgb, d_color, d_normal, d_out_rays, d_out_weights,
                                            d_out_pixels, d_out_count, d_counts, misaligned(4, d_ids, d_out_ids));
    if (st != MR_OK) return st;
    LightScene ls;
    if ((st = level_lights_params(who, s, level->environment != 0, stream, ls)) != MR_OK) return st;
    return launch_level_lights_path(ls, *level, d_rays, d_weights, d_pixels, d_ids, n, d_rgb, d_hits, d_ray_rgb, d_color, d_normal,
                                    d_out_rays, d_out_weights, d_out_pixels, d_out_ids, reinterpret_cast<unsigned long long *>(d_out_count),
                                    reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
}

// what the three calls of include/miro_hip_lens.h ask after the list of their pinhole twin, in this order: the lens as
// mr_gen_eye_rays_lens checks it, then image order (that generator, which the calls are held to, makes no other)
static mr_status check_frame_lens(const char *who, const mr_lens_desc *lens, const mr_frame_desc &fd) {
    if (!lens) return fail(MR_ERR_INVALID, "%s: NULL lens", who);
    for (int k = 0; k < 6; k++)
        if (lens->reserved[k] != 0) return fail(MR_ERR_INVALID, "%s: mr_lens_desc.reserved must be 0", who);
    if (!std::isfinite(lens->aperture) || lens->aperture < 0.0f) return fail(MR_ERR_INVALID, "%s: aperture must be finite and >= 0", who);
    if (!std::isfinite(lens->focus_plane) || !(lens->focus_plane > 0.0f))
        return fail(MR_ERR_INVALID, "%s: focus_plane must be finite and > 0", who);
    if (fd.tiled)
        return fail(MR_ERR_INVALID, "%s: tiled sample order (the thin-lens rays are mr_gen_eye_rays_lens', in image order); use tiled = 0", who);
    return MR_OK;
}

// The level-0 frame that also emits the rays of level 1 (mr_frame_level_lights.hip).  The frame call's argument checks under this
// call's name, then the level calls' in their order, all before the scene's state is read; then the state and the uploads of
// mr_render_lights_environment.  MR_LEVEL_LAST is that frame itself.  with_lens: mr_render_level_lights_lens (mr_frame_lens.hip),
// whose lens checks follow the list and whose MR_LEVEL_LAST is its own kernel
static mr_status render_level_lights(const char *who, bool with_lens, mr_scene *s, const mr_frame_desc *frame, const mr_lens_desc *lens,
                                     const mr_frame_level_desc *level, float *d_rgb, mr_hit *d_hits, float *d_sample_rgb,
                                     float *d_sample_color, float *d_sample_normal, mr_ray *d_out_rays, float *d_out_weights,
                                     uint32_t *d_out_pixels, uint32_t *d_out_ids, uint64_t *d_out_count, uint64_t *d_counts, void *stream) {
    mr_frame_desc fd;
    mr_status st = check_render_lights_args(who, s, frame, fd, d_rgb, d_hits, d_sample_rgb,
                                            misaligned(4, d_sample_color, d_sample_normal), d_counts);
    if (st != MR_OK) return st;
    if (!level) return fail(MR_ERR_INVALID, "%s: NULL argument (level)", who);
    if (fd.flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT))
        return fail(MR_ERR_INVALID, "%s: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT only (the shadow rays are closest-hit, as in "
                                    "mr_trace_level_lights)", who);
    if (level->children != MR_LEVEL_LAST && level->children != MR_LEVEL_SPECULAR && level->children != MR_LEVEL_PATH)
        return fail(MR_ERR_INVALID, "%s: children must be MR_LEVEL_LAST, MR_LEVEL_SPECULAR or MR_LEVEL_PATH", who);
    if (level->environment > 1) return fail(MR_ERR_INVALID, "%s: environment must be 0 or 1", who);
    if (level->children == MR_LEVEL_PATH && (level->path_kinds == 0 || (level->path_kinds & ~7u)))
        return fail(MR_ERR_INVALID, "%s: path_kinds must be a combination of MR_PATH_MIRROR | MR_PATH_REFRACT | MR_PATH_DIFFUSE", who);
    for (int k = 0; k < 6; k++)
        if (level->reserved[k] != 0) return fail(MR_ERR_INVALID, "%s: mr_frame_level_desc.reserved must be 0", who);
    const bool children = level->children != MR_LEVEL_LAST;
    if (children) {
        unsigned long long n = 0;                              // (the window has passed check_frame_lights: this cannot fail here)
        if ((st = frame_level_lights_samples(who, fd, n)) != MR_OK) return st;
        st = check_out_queue(who, "%s: a frame with children needs the output queue",
                             "%s: out_capacity is 0 (room for %u rays per sample always suffices)",
                             "%s: at most 2^32 - 1 samples per call with children", true, level->children == MR_LEVEL_PATH ? 4u : 3u,
                             level->out_capacity_lo, level->out_capacity_hi, n, d_out_rays, d_out_weights, d_out_pixels, d_out_count);
        if (st != MR_OK) return st;
        if (misaligned(16, d_out_rays) || misaligned(8, d_out_count) || misaligned(4, d_out_weights, d_out_pixels, d_out_ids))
            return fail(MR_ERR_INVALID, "%s: the output rays must be 16-byte aligned, d_out_count 8-byte, weights, pixels and ids "
                                        "4-byte aligned", who);
    }
    if (with_lens && (st = check_frame_lens(who, lens, fd)) != MR_OK) return st;
    if ((st = check_render_lights_state(who, s, fd, false)) != MR_OK) return st;
    LightScene ls;
    if ((st = lights_scene_params(s, level->environment != 0, stream, ls)) != MR_OK) return st;
    const RayQueue out = {d_out_rays, d_out_weights, d_out_pixels, d_out_ids, level->d_out_lowres};
    const FrameOutputs o = {d_rgb, d_hits, d_sample_rgb, d_sample_color, d_sample_normal, reinterpret_cast<unsigned long long *>(d_counts)};
    return launch_level0_lights(who, ls, fd, with_lens ? lens : nullptr, *level, o, out, reinterpret_cast<unsigned long long *>(d_out_count),
                                static_cast<hipStream_t>(stream));
}
mr_status mr_render_level_lights(mr_scene *s, const mr_frame_desc *frame, const mr_frame_level_desc *level, float *d_rgb, mr_hit *d_hits,
                                 float *d_sample_rgb, float *d_sample_color, float *d_sample_normal, mr_ray *d_out_rays,
                                 float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids, uint64_t *d_out_count,
                                 uint64_t *d_counts, void *stream) {
    return render_level_lights("mr_render_level_lights", false, s, frame, nullptr, level, d_rgb, d_hits, d_sample_rgb, d_sample_color,
                               d_sample_normal, d_out_rays, d_out_weights, d_out_pixels, d_out_ids, d_out_count, d_counts, stream);
}
// ... through the thin lens (include/miro_hip_lens.h; Camera.cpp:135-160, Miro.h:18-19)
mr_status mr_render_level_lights_lens(mr_scene *s, const mr_frame_desc *frame, const mr_lens_desc *lens, const mr_frame_level_desc *level,
                                      float *d_rgb, mr_hit *d_hits, float *d_sample_rgb, float *d_sample_color, float *d_sample_normal,
                                      mr_ray *d_out_rays, float *d_out_weights, uint32_t *d_out_pixels, uint32_t *d_out_ids,
                                      uint64_t *d_out_count, uint64_t *d_counts, void *stream) {
    return render_level_lights("mr_render_level_lights_lens", true, s, frame, lens, level, d_rgb, d_hits, d_sample_rgb, d_sample_color,
                               d_sample_normal, d_out_rays, d_out_weights, d_out_pixels, d_out_ids, d_out_count, d_counts, stream);
}

// The workspace of mr_render_recursion: two queues of `cap` rays, each a run of arrays whose offsets are rounded up to 16 bytes
// (the ray queue's alignment, which serves every other array).  The offsets of ONE queue's rays, weights, pixels, ids and low-res
// bytes (ids / low: where the queue has none, the offset of its end) and its size in bytes
struct RecursionQueue { uint64_t rays, weights, pixels, ids, low, bytes; bool has_ids, has_low; };
static RecursionQueue recursion_queue_layout(uint64_t cap, bool path, bool low) {
    auto up = [](uint64_t v) { return (v + 15ull) & ~15ull; };
    RecursionQueue q;
    q.rays = 0;
    q.weights = up(q.rays + 32ull * cap);
    q.pixels = up(q.weights + 12ull * cap);
    q.ids = up(q.pixels + 4ull * cap);
    q.low = path ? up(q.ids + 4ull * cap) : q.ids;
    q.bytes = path && low ? up(q.low + cap) : q.low;
    q.has_ids = path; q.has_low = path && low;
    return q;
}
static RecursionQueue recursion_queue_layout(const mr_recursion_desc &rd) {
    return recursion_queue_layout(rd.queue_capacity_lo, rd.children == MR_LEVEL_PATH, rd.environment != 0);
}
// the two queues of a workspace laid out as `q`, array by array
static void recursion_queues(void *d_workspace, const RecursionQueue &q, RayQueue qs[2]) {
    for (int w = 0; w < 2; w++) {
        uint8_t *base = static_cast<uint8_t *>(d_workspace) + (uint64_t)w * q.bytes;
        qs[w].rays = reinterpret_cast<mr_ray *>(base + q.rays);
        qs[w].weights = reinterpret_cast<float *>(base + q.weights);
        qs[w].pixels = reinterpret_cast<uint32_t *>(base + q.pixels);
        qs[w].ids = q.has_ids ? reinterpret_cast<uint32_t *>(base + q.ids) : nullptr;
        qs[w].low = q.has_low ? base + q.low : nullptr;
    }
}
// what every call of the family asks of the descriptor alone, in this order
static mr_status check_recursion_desc(const char *who, const mr_recursion_desc *rd) {
    if (!rd) return fail(MR_ERR_INVALID, "%s: NULL argument (desc)", who);
    if (rd->depth > 64) return fail(MR_ERR_INVALID, "%s: depth must be 64 at most", who);
    if (rd->environment > 1) return fail(MR_ERR_INVALID, "%s: environment must be 0 or 1", who);
    for (int k = 0; k < 5; k++)
        if (rd->reserved[k] != 0) return fail(MR_ERR_INVALID, "%s: mr_recursion_desc.reserved must be 0", who);
    if (rd->depth == 0) return MR_OK;
    if (rd->children != MR_LEVEL_SPECULAR && rd->children != MR_LEVEL_PATH)
        return fail(MR_ERR_INVALID, "%s: children must be MR_LEVEL_SPECULAR or MR_LEVEL_PATH", who);
    if (rd->children == MR_LEVEL_PATH && (rd->path_kinds == 0 || (rd->path_kinds & ~7u)))
        return fail(MR_ERR_INVALID, "%s: path_kinds must be a combination of MR_PATH_MIRROR | MR_PATH_REFRACT | MR_PATH_DIFFUSE", who);
    if (rd->queue_capacity_lo == 0 && rd->queue_capacity_hi == 0)
        return fail(MR_ERR_INVALID, "%s: queue_capacity is 0 (room for %u rays per sample always suffices for level 1)", who,
                    rd->children == MR_LEVEL_PATH ? 4u : 3u);
    if (rd->queue_capacity_hi != 0)
        return fail(MR_ERR_INVALID, "%s: at most 2^32 - 1 rays per queue", who);
    return MR_OK;
}
// what mr_render_recursion and mr_render_recursion_photons ask first, in this order: the argument checks of
// mr_render_level_lights under the call's name, the counters, the flags, the descriptor.  fd: the frame as the launchers take it;
// samples: those of its window (which has passed check_frame_lights: counting them cannot fail)
// (counts_name: what the call names its counters, d_level_counts or d_pass_counts)
static mr_status check_recursion_args(const char *who, mr_scene *s, const mr_frame_desc *frame, const mr_recursion_desc *desc,
                                      const float *d_rgb, const uint64_t *d_level_counts, mr_frame_desc &fd, unsigned long long &samples,
                                      const char *counts_name = "d_level_counts") {
    mr_status st = check_render_lights_args(who, s, frame, fd, d_rgb, nullptr, nullptr, false, d_level_counts);
    if (st != MR_OK) return st;
    if (!d_level_counts) return fail(MR_ERR_INVALID, "%s: NULL argument (%s)", who, counts_name);
    if (fd.flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT))
        return fail(MR_ERR_INVALID, "%s: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT only (the shadow rays are closest-hit, as in "
                                    "mr_trace_level_lights)", who);
    if ((st = check_recursion_desc(who, desc)) != MR_OK) return st;
    return frame_level_lights_samples(who, fd, samples);
}

mr_status mr_render_recursion_workspace(const mr_recursion_desc *desc, uint64_t *bytes) {
    const char *who = "mr_render_recursion_workspace";
    if (!bytes) return fail(MR_ERR_INVALID, "%s: NULL argument (bytes)", who);
    const mr_status st = check_recursion_desc(who, desc);
    if (st != MR_OK) return st;
    *bytes = desc->depth == 0 ? 0ull : 2ull * recursion_queue_layout(*desc).bytes;
    return MR_OK;
}

// ---- the passes of a frame of S samples per pixel (include/miro_hip_passes.h).  The rule: from sample_begin, whole passes of
// frame_spp while they fit below sample_end, then the remainder as powers of two in descending order.  Writes the first
// `capacity` passes (base / spp: either may be NULL) and returns how many there are
static uint32_t passes_plan(uint32_t frame_spp, uint32_t begin, uint32_t end, uint32_t *base, uint32_t *spp, uint32_t capacity) {
    uint32_t n = 0;
    for (uint32_t at = begin, p; at < end; at += p, n++) {
        for (p = frame_spp; p > end - at;) p >>= 1;
        if (n < capacity && base) base[n] = at;
        if (n < capacity && spp) spp[n] = p;
    }
    return n;
}
// what the descriptor alone can get wrong, in this order; frame_spp: a power of two <= 64
static mr_status check_passes_desc(const char *who, const mr_passes_desc *pd, uint32_t frame_spp) {
    if (!pd) return fail(MR_ERR_INVALID, "%s: NULL argument (passes)", who);
    for (int k = 0; k < 5; k++)
        if (pd->reserved[k] != 0) return fail(MR_ERR_INVALID, "%s: mr_passes_desc.reserved must be 0", who);
    if (pd->spp_total == 0) return fail(MR_ERR_INVALID, "%s: spp_total must be at least 1", who);
    if (pd->sample_begin >= pd->sample_end || pd->sample_end > pd->spp_total)
        return fail(MR_ERR_INVALID, "%s: samples [%u, %u) are no non-empty range inside [0, spp_total = %u)", who, pd->sample_begin,
                    pd->sample_end, pd->spp_total);
    if (pd->sample_begin % frame_spp != 0)
        return fail(MR_ERR_INVALID, "%s: sample_begin (%u) must be a multiple of the frame's spp (%u)", who, pd->sample_begin, frame_spp);
    return MR_OK;
}
mr_status mr_render_passes_plan(uint32_t frame_spp, const mr_passes_desc *desc, uint32_t *n_passes, uint32_t *base, uint32_t *spp,
                                uint32_t capacity) {
    const char *who = "mr_render_passes_plan";
    if (!n_passes) return fail(MR_ERR_INVALID, "%s: NULL argument (n_passes)", who);
    if (frame_spp == 0 || frame_spp > 64 || (frame_spp & (frame_spp - 1)))
        return fail(MR_ERR_INVALID, "%s: spp must be a power of two <= 64 (got %u)", who, frame_spp);
    const mr_status st = check_passes_desc(who, desc, frame_spp);
    if (st != MR_OK) return st;
    *n_passes = passes_plan(frame_spp, desc->sample_begin, desc->sample_end, base, spp, capacity);
    return MR_OK;
}
// what the two passes calls ask after their parent call's list (and the lens checks), in this order; fd: the frame as the launchers
// take it, samples: those of its window
static mr_status check_passes(const char *who, const mr_frame_desc &fd, const mr_recursion_desc &rd, unsigned long long samples,
                              const mr_passes_desc *pd) {
    if (fd.tiled)
        return fail(MR_ERR_INVALID, "%s: tiled sample order (a sample's frame-wide index is pixel * spp_total + sample, in image "
                                    "order); use tiled = 0", who);
    const mr_status st = check_passes_desc(who, pd, fd.spp);
    if (st != MR_OK) return st;
    if (rd.depth >= 1 && samples / fd.spp * pd->spp_total > 0xFFFFFFFFull)
        return fail(MR_ERR_INVALID, "%s: at most 2^32 - 1 samples per frame with children (%llu pixels x spp_total %u: ray ids are "
                                    "32 bits)", who, samples / fd.spp, pd->spp_total);
    return MR_OK;
}
// The launches of a whole recursive frame on one stream, and nothing else: the kernel that zeroes the counters (`counts`:
// [depth + 1][8]); level 0, mr_render_level_lights' launcher (launch_level0_lights) with its children in queue 0 of the workspace (depth 0: the plain
// frame, no workspace); then one queued level kernel (mr_level_lights_queued.hip) per further level, from one queue into the
// other, whose length is the word the level before counted its children into.  d_hits / d_normal: optional, every level's per-ray
// records, each level overwriting the one before.  step(l, row, d_n, bound, in, pass) is enqueued after level l, 0 included -- row: the
// level's eight counters, d_n: the
// word that holds the level's length (level 0: the samples the frame counted), bound: what the host knows it cannot exceed (fan^l
// x samples, saturating at the capacity), in: the queue the level read (level 0: none, its rays start at the eye).  lens
// (optional): level 0 is the thin-lens frame's launcher (mr_frame_lens.hip), at depth 0 too; the further levels do not differ
// pass (optional): the call is one pass of a frame of pass->S samples per pixel (mr_render_recursion_passes): level 0 is
// mr_frame_passes.hip's kernel for either camera, the further levels divide by S, and `step` is handed the pass
static mr_status no_level_step(uint32_t, unsigned long long *, const unsigned long long *, unsigned long long, const RayQueue &, const FramePass *) { return MR_OK; }
extern "C++" template <typename STEP>                                                  // (the entry points around it have C linkage)
static mr_status enqueue_recursion(const LightScene &ls, const mr_frame_desc &fd, const mr_lens_desc *lens, const mr_recursion_desc &rd,
                                   unsigned long long samples, void *d_workspace, float *d_rgb, mr_hit *d_hits, float *d_normal, unsigned long long *counts,
                                   hipStream_t hs, STEP step, const FramePass *pass = nullptr) {
    mr_status st = launch_zero_words(counts, 8ull * (rd.depth + 1ull), hs);
    if (st != MR_OK) return st;
    const bool path = rd.children == MR_LEVEL_PATH;
    const uint64_t cap = rd.queue_capacity_lo;
    const unsigned fan = path ? 4u : 3u;
    RayQueue qs[2] = {};
    mr_frame_level_desc l0 = {};
    l0.children = MR_LEVEL_LAST; l0.environment = rd.environment;
    if (rd.depth > 0) {
        recursion_queues(d_workspace, recursion_queue_layout(rd), qs);
        l0.children = rd.children;
        l0.path_kinds = rd.path_kinds; l0.path_seed = rd.path_seed;
        l0.out_capacity_lo = rd.queue_capacity_lo; l0.out_capacity_hi = 0;
    }
    FrameOutputs o = {};
    o.rgb = d_rgb; o.hits = d_hits; o.sample_normal = d_normal; o.counts = counts;
    st = pass ? launch_frame_pass("mr_render_recursion_passes", ls, fd, lens, l0, *pass, o, qs[0], &counts[5], hs)
              : launch_level0_lights("mr_render_level_lights_lens", ls, fd, lens, l0, o, qs[0], &counts[5], hs);
    if (st != MR_OK || (st = step(0u, counts, &counts[0], samples, RayQueue{}, pass)) != MR_OK) return st;

    QueuedLevel lv = {};
    lv.spp = pass ? pass->S : fd.spp;
    lv.flags = (fd.flags & MR_MATH_PRODUCT) | MR_TRACE_INCOHERENT;                      // a bounce queue is compacted in wave order
    lv.path = path; lv.environment = rd.environment;
    lv.path_kinds = rd.path_kinds; lv.seed = rd.path_seed;
    lv.capacity = cap;
    unsigned long long bound = samples;
    for (uint32_t l = 1; l <= rd.depth; l++) {
        bound = bound > cap / fan ? cap : bound * fan;
        const RayQueue &in = qs[(l - 1) & 1], &out = qs[l & 1];
        unsigned long long *row = counts + 8ull * l;
        const unsigned long long *d_n = row - 8 + 5;                                      // the children level l - 1 counted
        lv.last = l == rd.depth; lv.bounce = l;
        if ((st = launch_level_lights_queued(ls, lv, in, out, d_n, cap, bound, d_rgb, d_hits, d_normal, row, hs)) != MR_OK ||
            (st = step(l, row, d_n, bound, in, pass)) != MR_OK)
            return st;
    }
    return MR_OK;
}

// one enqueue_recursion per pass of the plan (passes_plan's rule), the passes' counter blocks ([depth + 1][8] each) one after the
// other; pixels: those of fd's window
extern "C++" template <typename STEP>
static mr_status enqueue_recursion_passes(const LightScene &ls, const mr_frame_desc &fd, const mr_lens_desc *lens, const mr_recursion_desc &rd,
                                          const mr_passes_desc &pd, unsigned long long pixels, void *d_workspace, float *d_rgb, mr_hit *d_hits,
                                          float *d_normal, unsigned long long *counts, hipStream_t hs, STEP step) {
    uint32_t i = 0;
    for (uint32_t at = pd.sample_begin, p; at < pd.sample_end; at += p, i++) {
        for (p = fd.spp; p > pd.sample_end - at;) p >>= 1;
        mr_frame_desc fp = fd;
        fp.spp = p;
        const FramePass pass = {pd.spp_total, at};
        const mr_status st = enqueue_recursion(ls, fp, lens, rd, pixels * p, d_workspace, d_rgb, d_hits, d_normal,
                                               counts + 8ull * (rd.depth + 1ull) * i, hs, step, &pass);
        if (st != MR_OK) return st;
    }
    return MR_OK;
}

// The whole recursive frame on one stream (include/miro_hip_recursion.h).  The argument checks first, all before the scene's
// state is read; then the state and the uploads; then nothing but launches (enqueue_recursion).
// with_lens: mr_render_recursion_lens, whose lens checks follow the list
// with_passes: mr_render_recursion_passes -- the call once per pass of `passes` (check_passes follows the lens checks); the
// counters are d_pass_counts
static mr_status render_recursion(const char *who, bool with_lens, mr_scene *s, const mr_frame_desc *frame, const mr_lens_desc *lens,
                                  const mr_recursion_desc *desc, float *d_rgb, void *d_workspace, uint64_t workspace_bytes,
                                  uint64_t *d_level_counts, void *stream, bool with_passes = false, const mr_passes_desc *passes = nullptr) {
    mr_frame_desc fd;
    unsigned long long samples = 0;
    mr_status st = check_recursion_args(who, s, frame, desc, d_rgb, d_level_counts, fd, samples, with_passes ? "d_pass_counts" : "d_level_counts");
    if (st != MR_OK) return st;
    if (desc->depth > 0) {
        if (samples > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "%s: at most 2^32 - 1 samples per call with children", who);
        const uint64_t need = 2ull * recursion_queue_layout(*desc).bytes;
        if (!d_workspace || misaligned(16, d_workspace))
            return fail(MR_ERR_INVALID, "%s: depth >= 1 needs a workspace, 16-byte aligned (mr_render_recursion_workspace)", who);
        if (workspace_bytes < need)
            return fail(MR_ERR_INVALID, "%s: workspace_bytes is %llu, two queues of %llu rays need %llu (mr_render_recursion_workspace)", who,
                        (unsigned long long)workspace_bytes, (unsigned long long)desc->queue_capacity_lo, (unsigned long long)need);
    }
    if (with_lens && (st = check_frame_lens(who, lens, fd)) != MR_OK) return st;
    if (with_passes && (st = check_passes(who, fd, *desc, samples, passes)) != MR_OK) return st;
    if ((st = check_render_lights_state(who, s, fd, false)) != MR_OK) return st;
    LightScene ls;
    if ((st = lights_scene_params(s, desc->environment != 0, stream, ls)) != MR_OK) return st;
    if (with_passes)
        return enqueue_recursion_passes(ls, fd, with_lens ? lens : nullptr, *desc, *passes, samples / fd.spp, d_workspace, d_rgb, nullptr,
                                        nullptr, reinterpret_cast<unsigned long long *>(d_level_counts), static_cast<hipStream_t>(stream),
                                        no_level_step);
    return enqueue_recursion(ls, fd, with_lens ? lens : nullptr, *desc, samples, d_workspace, d_rgb, nullptr, nullptr,
                             reinterpret_cast<unsigned long long *>(d_level_counts), static_cast<hipStream_t>(stream), no_level_step);
}
// ... once per pass of a frame of passes->spp_total samples per pixel (include/miro_hip_passes.h); lens: optional
mr_status mr_render_recursion_passes(mr_scene *s, const mr_frame_desc *frame, const mr_lens_desc *lens, const mr_recursion_desc *desc,
                                     const mr_passes_desc *passes, float *d_rgb, void *d_workspace, uint64_t workspace_bytes,
                                     uint64_t *d_pass_counts, void *stream) {
    return render_recursion("mr_render_recursion_passes", lens != nullptr, s, frame, lens, desc, d_rgb, d_workspace, workspace_bytes,
                            d_pass_counts, stream, true, passes);
}
mr_status mr_render_recursion(mr_scene *s, const mr_frame_desc *frame, const mr_recursion_desc *desc, float *d_rgb, void *d_workspace,
                              uint64_t workspace_bytes, uint64_t *d_level_counts, void *stream) {
    return render_recursion("mr_render_recursion", false, s, frame, nullptr, desc, d_rgb, d_workspace, workspace_bytes, d_level_counts, stream);
}
// ... through the thin lens (include/miro_hip_lens.h; Camera.cpp:135-160, Miro.h:18-19)
mr_status mr_render_recursion_lens(mr_scene *s, const mr_frame_desc *frame, const mr_lens_desc *lens, const mr_recursion_desc *desc, float *d_rgb,
                                   void *d_workspace, uint64_t workspace_bytes, uint64_t *d_level_counts, void *stream) {
    return render_recursion("mr_render_recursion_lens", true, s, frame, lens, desc, d_rgb, d_workspace, workspace_bytes, d_level_counts, stream);
}

// The workspace of mr_render_recursion_photons behind the two queues: hit records, normals and mr_gather_level's scratch for M
// rays, M = max(samples, depth >= 1 ? queue_capacity : 0); each array's size rounded up to 16 bytes (offsets from the queues' end)
struct RecursionPhotonsLayout { uint64_t queues, hits, normals, scratch, bytes; };
static RecursionPhotonsLayout recursion_photons_layout(const mr_recursion_desc &rd, uint64_t samples) {
    auto up = [](uint64_t v) { return (v + 15ull) & ~15ull; };
    const uint64_t cap = rd.depth > 0 ? rd.queue_capacity_lo : 0ull, M = samples > cap ? samples : cap;
    RecursionPhotonsLayout w;
    w.queues = rd.depth == 0 ? 0ull : 2ull * recursion_queue_layout(rd).bytes;
    w.hits = w.queues;
    w.normals = w.hits + up(16ull * M);
    w.scratch = w.normals + up(12ull * M);
    w.bytes = w.scratch + up(48ull * M);
    return w;
}
// what the photon term adds to the checks of the two descriptors, in this order: image order, and no more rays per level than
// one estimate launch answers
static mr_status check_recursion_photons_window(const char *who, const mr_frame_desc &fd, const mr_recursion_desc &rd, unsigned long long samples) {
    if (fd.tiled)
        return fail(MR_ERR_INVALID, "%s: tiled sample order (level 0's photon term finds its pixel from the sample index, in image "
                                    "order); use tiled = 0", who);
    if (samples >= (1ull << 31) || (rd.depth > 0 && rd.queue_capacity_lo >= (1u << 31)))
        return fail(MR_ERR_INVALID, "%s: at most 2^31 - 1 samples and a queue_capacity of at most 2^31 - 1 (one estimate launch answers "
                                    "at most 2^31 - 1 queries)", who);
    return MR_OK;
}

mr_status mr_render_recursion_photons_workspace(const mr_frame_desc *frame, const mr_recursion_desc *desc, uint64_t *bytes) {
    const char *who = "mr_render_recursion_photons_workspace";
    if (!bytes) return fail(MR_ERR_INVALID, "%s: NULL argument (bytes)", who);
    if (!frame) return fail(MR_ERR_INVALID, "%s: NULL argument (frame)", who);
    mr_frame_desc fd;
    unsigned long long samples = 0;
    mr_status st = check_render_lights_frame(who, *frame, fd);
    if (st != MR_OK || (st = check_recursion_desc(who, desc)) != MR_OK || (st = frame_level_lights_samples(who, fd, samples)) != MR_OK ||
        (st = check_recursion_photons_window(who, fd, *desc, samples)) != MR_OK)
        return st;
    *bytes = recursion_photons_layout(*desc, samples).bytes;
    return MR_OK;
}

// mr_render_recursion with the photon-map term after every level (include/miro_hip_recursion_photons.h): enqueue_recursion with
// the workspace's hit and normal buffers handed to every level launch, and as its step the three kernels of mr_gather_queued.hip
// on that level's queue.  The argument checks first, all of them before the scene's or a map's state is read; then the state and
// the uploads; then nothing but launches.
// with_lens: mr_render_recursion_photons_lens, whose lens checks follow the list and whose level 0 makes the lens ray again
static mr_status render_recursion_photons(const char *who, bool with_lens, mr_scene *s, const mr_frame_desc *frame, const mr_lens_desc *lens,
                                          const mr_recursion_desc *desc, mr_photon_map *global_map, mr_photon_map *caustic_map,
                                          float max_dist, uint32_t nphotons, float *d_rgb, void *d_workspace, uint64_t workspace_bytes,
                                          uint64_t *d_level_counts, void *stream, bool with_passes = false,
                                          const mr_passes_desc *passes = nullptr) {
    mr_frame_desc fd;
    unsigned long long samples = 0;
    mr_status st = check_recursion_args(who, s, frame, desc, d_rgb, d_level_counts, fd, samples, with_passes ? "d_pass_counts" : "d_level_counts");
    if (st != MR_OK || (st = check_recursion_photons_window(who, fd, *desc, samples)) != MR_OK) return st;
    mr_photon_map *maps[2] = {global_map, caustic_map};
    if (!maps[0] && !maps[1]) return fail(MR_ERR_INVALID, "%s: NULL argument (global_map and caustic_map are both NULL)", who);
    if (nphotons == 0 || nphotons > (uint32_t)kKnnMaxK) return fail(MR_ERR_INVALID, "%s: nphotons must be in [1, %d]", who, kKnnMaxK);
    if (!(max_dist > 0.0f)) return fail(MR_ERR_INVALID, "%s: max_dist must be positive", who);
    const RecursionPhotonsLayout ws = recursion_photons_layout(*desc, samples);
    if (!d_workspace || misaligned(16, d_workspace))
        return fail(MR_ERR_INVALID, "%s: the call needs a workspace, 16-byte aligned (mr_render_recursion_photons_workspace)", who);
    if (workspace_bytes < ws.bytes)
        return fail(MR_ERR_INVALID, "%s: workspace_bytes is %llu, this frame and descriptor need %llu (mr_render_recursion_photons_workspace)",
                    who, (unsigned long long)workspace_bytes, (unsigned long long)ws.bytes);
    if (with_lens && (st = check_frame_lens(who, lens, fd)) != MR_OK) return st;
    if (with_passes && (st = check_passes(who, fd, *desc, samples, passes)) != MR_OK) return st;

    if ((st = check_render_lights_state(who, s, fd, false)) != MR_OK) return st;
    for (mr_photon_map *m : maps) {
        if (m && !photon_map_resident(m)) return fail(MR_ERR_STATE, "%s: photon map is not balanced and resident on a device", who);
        if (m && photon_map_device(m) != s->device)
            return fail(MR_ERR_STATE, "%s: photon map lives on device %d, the scene on %d", who, photon_map_device(m), s->device);
        if (m && photon_map_stored(m) >= (1u << 24))
            return fail(MR_ERR_STATE, "%s: photon maps of 2^24 photons or more need a fifth layer of blocks", who);
    }
    LightScene ls;
    if ((st = lights_scene_params(s, desc->environment != 0, stream, ls)) != MR_OK) return st;

    hipStream_t hs = static_cast<hipStream_t>(stream);
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(d_level_counts);
    uint8_t *wbase = static_cast<uint8_t *>(d_workspace);
    mr_hit *d_hits = reinterpret_cast<mr_hit *>(wbase + ws.hits);
    // the normal Scene::trace hands on differs from the object's on a procedural texture only: elsewhere the query kernels form it
    float *d_normal = s->tex.procedural ? reinterpret_cast<float *>(wbase + ws.normals) : nullptr;
    float *d_scratch = reinterpret_cast<float *>(wbase + ws.scratch);

    // level l's photon term, before level l + 1 overwrites the hit records and (two levels on) this queue: queries, one estimate
    // per map, the accumulate, over a scratch laid out for `bound` rays.  bound <= the queue's capacity, and the kernels take it
    // as the capacity, so that no index reaches beyond that scratch.  Level 0 has no queue: its queries come from the eye rays
    // made again, its length is the window's, which the frame has added to counts[0]; weight 1, pixel k / spp (in: all NULL).
    // row: the level's eight counters.  pass (optional): the pass of a longer frame this is -- a level-0 sample's pixel is k / the
    // pass's spp (bound / the window's pixels), the divisor pass->S
    const unsigned long long pixels = samples / fd.spp;
    auto photon_term = [&](uint32_t l, unsigned long long *row, const unsigned long long *d_n, unsigned long long bound, const RayQueue &in,
                           const FramePass *pass) -> mr_status {
        const GatherScratch sc = gather_scratch(d_scratch, bound, maps[0] != nullptr, maps[1] != nullptr);
        unsigned long long *d_queries = row + 6;
        mr_frame_desc fp = fd;
        if (pass) fp.spp = (uint32_t)(bound / pixels);
        mr_status e = l > 0 ? launch_gather_queued_queries(s->dev, in.rays, d_hits, d_normal, d_n, bound, sc.pos, sc.nrm, d_queries, hs)
                      : pass ? launch_gather_eye_queries_pass(s->dev, who, fp, with_lens ? lens : nullptr, *pass, d_hits, d_normal, sc.pos, sc.nrm,
                                                              d_queries, hs)
                      : with_lens ? launch_gather_eye_queries_lens(s->dev, who, fd, *lens, d_hits, d_normal, sc.pos, sc.nrm, d_queries, hs)
                                  : launch_gather_eye_queries(s->dev, who, fd, d_hits, d_normal, sc.pos, sc.nrm, d_queries, hs);
        for (int i = 0; i < 2 && e == MR_OK; i++)
            if (maps[i]) e = photon_map_estimate_queued(maps[i], sc.pos, sc.nrm, d_n, bound, max_dist, nphotons, sc.irr[i], hs);
        if (e != MR_OK) return e;
        return launch_gather_queued_accumulate(sc.irr[0], sc.irr[1], in.weights, in.pixels, d_n, bound, fp.spp, pass ? pass->S : fd.spp, d_rgb, hs);
    };
    if (with_passes)
        return enqueue_recursion_passes(ls, fd, with_lens ? lens : nullptr, *desc, *passes, pixels, d_workspace, d_rgb, d_hits, d_normal, counts,
                                        hs, photon_term);
    return enqueue_recursion(ls, fd, with_lens ? lens : nullptr, *desc, samples, d_workspace, d_rgb, d_hits, d_normal, counts, hs, photon_term);
}
// ... once per pass of a frame of passes->spp_total samples per pixel (include/miro_hip_passes.h); lens: optional
mr_status mr_render_recursion_photons_passes(mr_scene *s, const mr_frame_desc *frame, const mr_lens_desc *lens, const mr_recursion_desc *desc,
                                             const mr_passes_desc *passes, mr_photon_map *global_map, mr_photon_map *caustic_map,
                                             float max_dist, uint32_t nphotons, float *d_rgb, void *d_workspace, uint64_t workspace_bytes,
                                             uint64_t *d_pass_counts, void *stream) {
    return render_recursion_photons("mr_render_recursion_photons_passes", lens != nullptr, s, frame, lens, desc, global_map, caustic_map,
                                    max_dist, nphotons, d_rgb, d_workspace, workspace_bytes, d_pass_counts, stream, true, passes);
}
mr_status mr_render_recursion_photons(mr_scene *s, const mr_frame_desc *frame, const mr_recursion_desc *desc, mr_photon_map *global_map,
                                      mr_photon_map *caustic_map, float max_dist, uint32_t nphotons, float *d_rgb, void *d_workspace,
                                      uint64_t workspace_bytes, uint64_t *d_level_counts, void *stream) {
    return render_recursion_photons("mr_render_recursion_photons", false, s, frame, nullptr, desc, global_map, caustic_map, max_dist, nphotons,
                                    d_rgb, d_workspace, workspace_bytes, d_level_counts, stream);
}
// ... through the thin lens (include/miro_hip_lens.h; Camera.cpp:135-160, Miro.h:18-19)
mr_status mr_render_recursion_photons_lens(mr_scene *s, const mr_frame_desc *frame, const mr_lens_desc *lens, const mr_recursion_desc *desc,
                                           mr_photon_map *global_map, mr_photon_map *caustic_map, float max_dist, uint32_t nphotons,
                                           float *d_rgb, void *d_workspace, uint64_t workspace_bytes, uint64_t *d_level_counts, void *stream) {
    return render_recursion_photons("mr_render_recursion_photons_lens", true, s, frame, lens, desc, global_map, caustic_map, max_dist, nphotons,
                                    d_rgb, d_workspace, workspace_bytes, d_level_counts, stream);
}

mr_status mr_gen_eye_rays_lens(mr_scene *s, const mr_camera *cam, uint32_t W, uint32_t H, uint32_t y0, uint32_t y1, uint32_t spp,
                               uint32_t jitter, uint32_t seed, mr_ray *d_rays, void *stream, const mr_lens_desc *lens,
                               const float *d_samples_in, float *d_samples_out, uint64_t *d_counts) {
    if (!s || !cam || !d_rays) return fail(MR_ERR_INVALID, "NULL argument");
    if (!lens) return fail(MR_ERR_INVALID, "mr_gen_eye_rays_lens: NULL lens");
    for (int k = 0; k < 6; k++)
        if (lens->reserved[k] != 0) return fail(MR_ERR_INVALID, "mr_gen_eye_rays_lens: mr_lens_desc.reserved must be 0");
    if (!std::isfinite(lens->aperture) || lens->aperture < 0.0f) return fail(MR_ERR_INVALID, "mr_gen_eye_rays_lens: aperture must be finite and >= 0");
    if (!std::isfinite(lens->focus_plane) || !(lens->focus_plane > 0.0f)) return fail(MR_ERR_INVALID, "mr_gen_eye_rays_lens: focus_plane must be finite and > 0");
    if (W == 0 || H == 0 || spp == 0 || y1 < y0 || y1 > H) return fail(MR_ERR_INVALID, "bad image window");
    if (misaligned(16, d_rays, d_samples_in, d_samples_out) || misaligned(8, d_counts))
        return fail(MR_ERR_INVALID, "d_rays and the sample buffers must be 16-byte aligned, counters 8-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_eye_rays_lens(*cam, W, H, y0, y1, spp, jitter, seed, *lens, d_samples_in, d_samples_out,
                                reinterpret_cast<unsigned long long *>(d_counts), d_rays, static_cast<hipStream_t>(stream));
}

mr_status mr_square_light_tangents(const float normal[3], float t1[3], float t2[3]) {
    if (!normal || !t1 || !t2) return fail(MR_ERR_INVALID, "mr_square_light_tangents: NULL argument");
    tangents_of(normal, t1, t2);
    return MR_OK;
}

// What mr_shade_square_lights and mr_shade_square_lights_surface ask, in this order; `side` is what they launch with.  The
// argument errors come before the scene's state here: a bad call is MR_ERR_INVALID on any scene.  surface: the _surface call,
// which takes d_color / d_normal besides and looks nothing up, so that a texture table is no reason to refuse.
static mr_status check_shade_square_lights(const char *who, bool surface, mr_scene *s, const mr_square_light_desc *lights, uint32_t n_lights,
                                           uint32_t samples, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color,
                                           const float *d_normal, const float *d_uv_in, uint64_t n, uint32_t spp, uint32_t flags,
                                           const float *d_rgb, const float *d_ray_rgb, const uint64_t *d_counts, uint32_t &side) {
    if (!s) return fail(MR_ERR_INVALID, "%s: NULL scene", who);
    if (n_lights == 0 || n_lights > MR_MAX_LIGHTS) return fail(MR_ERR_INVALID, "%s: %u lights, at least 1 and at most %u", who, n_lights, (unsigned)MR_MAX_LIGHTS);
    if (!lights) return fail(MR_ERR_INVALID, "%s: NULL list of %u lights", who, n_lights);
    side = 0;
    while (side < 8 && side * side < samples) side++;
    if (samples == 0 || side * side != samples)
        return fail(MR_ERR_INVALID, "%s: samples = %u is not a perfect square in 1 ... 64 (SquareLight.h:27-33 subdivides the rectangle "
                                    "into int(sqrt(samples))^2 cells)", who, samples);
    mr_status st;
    for (uint32_t i = 0; i < n_lights; i++) {
        const mr_square_light_desc &in = lights[i];
        if ((st = check_light(who, i, in.reserved, in.position, in.color, in.wattage, in.normal)) != MR_OK) return st;
        for (int k = 0; k < 2; k++)
            if (!std::isfinite(in.dimensions[k]) || in.dimensions[k] < 0.0f)
                return fail(MR_ERR_INVALID, "%s: light %u: dimensions must be finite and >= 0", who, i);
    }
    if (!d_rays || !d_hits || (!d_rgb && !d_ray_rgb) || (surface && (!d_color || !d_normal))) return fail(MR_ERR_INVALID, "%s: NULL argument", who);
    if (spp == 0) return fail(MR_ERR_INVALID, "%s: spp is 0", who);
    if (n > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "%s: at most 2^32-1 rays per batch (the sample keys hold the ray index in 32 bits)", who);
    if (flags & ~(uint32_t)(MR_MATH_PRODUCT | MR_TRACE_INCOHERENT | MR_TRACE_ANY))
        return fail(MR_ERR_INVALID, "%s: flags may hold MR_MATH_PRODUCT, MR_TRACE_INCOHERENT, MR_TRACE_ANY only", who);
    if (misaligned(16, d_rays, d_hits) || misaligned(8, d_counts, d_uv_in) || misaligned(4, d_rgb, d_ray_rgb))
        return fail(MR_ERR_INVALID, "%s: ray / hit buffers must be 16-byte aligned, counters and d_uv_in 8-byte aligned", who);
    if (surface && misaligned(4, d_color, d_normal))
        return fail(MR_ERR_INVALID, "%s: d_color and d_normal must be 4-byte aligned", who);
    if ((st = require_device(s)) != MR_OK) return st;
    if (!surface) {
        if ((st = refuse_procedural(s, who, "mr_shade_square_lights_surface")) != MR_OK) return st;
        if ((st = refuse_textured(s, who)) != MR_OK) return st;
    }
    if ((flags & MR_TRACE_ANY) && s->dev.refractive)
        return fail(MR_ERR_STATE, "%s: MR_TRACE_ANY with a refractive material (the nearest occluder decides, Phong.cpp:99-113)", who);
    return MR_OK;
}

mr_status mr_shade_square_lights(mr_scene *s, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t samples, uint32_t seed,
                                 const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels,
                                 const float *d_uv_in, uint64_t n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb,
                                 uint64_t *d_counts, void *stream) {
    uint32_t side = 0;
    const mr_status st = check_shade_square_lights("mr_shade_square_lights", false, s, lights, n_lights, samples, d_rays, d_hits, nullptr, nullptr,
                                                   d_uv_in, n, spp, flags, d_rgb, d_ray_rgb, d_counts, side);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_shade_square_lights(s->dev, lights, n_lights, side, seed, d_rays, d_hits, d_weights, d_pixels, d_uv_in, n, spp, flags, d_rgb,
                                      d_ray_rgb, reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
}

mr_status mr_shade_square_lights_surface(mr_scene *s, const mr_square_light_desc *lights, uint32_t n_lights, uint32_t samples, uint32_t seed,
                                         const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color, const float *d_normal,
                                         const float *d_weights, const uint32_t *d_pixels, const float *d_uv_in, uint64_t n, uint32_t spp,
                                         uint32_t flags, float *d_rgb, float *d_ray_rgb, uint64_t *d_counts, void *stream) {
    uint32_t side = 0;
    const mr_status st = check_shade_square_lights("mr_shade_square_lights_surface", true, s, lights, n_lights, samples, d_rays, d_hits, d_color,
                                                   d_normal, d_uv_in, n, spp, flags, d_rgb, d_ray_rgb, d_counts, side);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_shade_square_lights_surface(s->dev, lights, n_lights, side, seed, d_rays, d_hits, d_color, d_normal, d_weights, d_pixels,
                                              d_uv_in, n, spp, flags, d_rgb, d_ray_rgb, reinterpret_cast<unsigned long long *>(d_counts),
                                              static_cast<hipStream_t>(stream));
}

mr_status mr_scene_set_environment(mr_scene *s, const mr_environment_desc *env) {
    if (!s) return fail(MR_ERR_INVALID, "mr_scene_set_environment: NULL scene");
    HostEnvironment e;
    if (env) {
        for (int k = 0; k < 6; k++)
            if (env->reserved[k] != 0) return fail(MR_ERR_INVALID, "mr_environment_desc.reserved must be 0");
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(env->bg_color[c])) return fail(MR_ERR_INVALID, "environment: bg_color must be finite");
        if (!std::isfinite(env->rotation[0]) || !std::isfinite(env->rotation[1])) return fail(MR_ERR_INVALID, "environment: rotation must be finite");
        // beyond these ranges the reference's lookup indexes outside its bitmap (phi is folded back by 2 PI once only)
        if (!(env->rotation[0] >= 0.0f && env->rotation[0] <= 6.2831853071795864769f))
            return fail(MR_ERR_INVALID, "environment: rotation[0] = %g is outside [0, 2 pi]", (double)env->rotation[0]);
        if (!(env->rotation[1] >= 0.0f && env->rotation[1] <= 1.5707963267948966192f))
            return fail(MR_ERR_INVALID, "environment: rotation[1] = %g is outside [0, pi / 2]", (double)env->rotation[1]);
        for (int c = 0; c < 3; c++) e.bg[c] = env->bg_color[c];
        e.rot[0] = env->rotation[0]; e.rot[1] = env->rotation[1];
        if (env->pixels) {
            const uint32_t W = env->W, H = env->H;
            if (W < kEnvLowresWidth) return fail(MR_ERR_INVALID, "environment: image width %u, at least %u (the low-res image's)", W, kEnvLowresWidth);
            if (W > 65536u || H > 65536u) return fail(MR_ERR_INVALID, "environment: image of %u x %u pixels, at most 65536 each way", W, H);
            const int lrh = (int)((float)kEnvLowresWidth * ((float)H / (float)W));                   // Texture.cpp:53
            if (lrh < 1) return fail(MR_ERR_INVALID, "environment: image height %u gives a low-res image of height 0", H);
            if ((uint32_t)lrh > kEnvMaxLowresHeight) return fail(MR_ERR_INVALID, "environment: image height %u is more than 4 x its width %u", H, W);
            const size_t n = 3 * (size_t)W * H;
            for (size_t i = 0; i < n; i++)
                if (!std::isfinite(env->pixels[i])) return fail(MR_ERR_INVALID, "environment: pixel value %zu is not finite", i);
            e.W = W; e.H = H; e.lw = kEnvLowresWidth; e.lh = (uint32_t)lrh;
            build_environment_image(e, env->pixels);
        }
    }
    s->env = std::move(e);
    s->env_dirty = s->env.W != 0;
    return MR_OK;
}

mr_status mr_scene_get_environment(const mr_scene *s, uint32_t which, uint32_t *W, uint32_t *H, float *max_intensity, float *pixels) {
    if (!s) return fail(MR_ERR_INVALID, "mr_scene_get_environment: NULL scene");
    if (which > 1) return fail(MR_ERR_INVALID, "mr_scene_get_environment: which = %u (0: the image, 1: the low-res image)", which);
    const HostEnvironment &e = s->env;
    const uint32_t w = which ? e.lw : e.W, h = which ? e.lh : e.H;
    if (W) *W = w;
    if (H) *H = h;
    if (max_intensity) *max_intensity = e.max_intensity;
    if (pixels) {
        const float *r = e.rec.data() + (which ? 4 * (size_t)e.W * e.H : 0);
        for (size_t i = 0; i < (size_t)w * h; i++)
            for (int c = 0; c < 3; c++) pixels[3 * i + c] = r[4 * i + c];
    }
    return MR_OK;
}

mr_status mr_shade_environment(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_weights, const uint32_t *d_pixels,
                               const uint8_t *d_lowres, uint64_t n, uint32_t spp, uint32_t flags, float *d_rgb, float *d_ray_rgb,
                               uint64_t *d_counts, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_rays || !d_hits || (!d_rgb && !d_ray_rgb)) return fail(MR_ERR_INVALID, "NULL argument");
    if (spp == 0) return fail(MR_ERR_INVALID, "spp is 0");
    if (n / spp > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "too many pixels");
    if (flags & ~(uint32_t)MR_ENV_LOWRES) return fail(MR_ERR_INVALID, "mr_shade_environment: flags may hold MR_ENV_LOWRES only");
    if (misaligned(16, d_rays, d_hits) || misaligned(8, d_counts) || misaligned(4, d_rgb, d_ray_rgb, d_weights, d_pixels))
        return fail(MR_ERR_INVALID, "ray / hit buffers must be 16-byte aligned, counters 8-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    EnvParams p;
    if ((st = environment_params(s, static_cast<hipStream_t>(stream), p)) != MR_OK) return st;
    return launch_shade_environment(p, d_rays, d_hits, d_weights, d_pixels, d_lowres, n, spp, flags, d_rgb, d_ray_rgb,
                                    reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
}

mr_status mr_scene_set_texcoords(mr_scene *s, const float *texcoords, uint32_t n_texcoords, const uint32_t *tidx) {
    if (!s) return fail(MR_ERR_INVALID, "mr_scene_set_texcoords: NULL scene");
    if (n_texcoords > 0 && (!texcoords || !tidx)) return fail(MR_ERR_INVALID, "mr_scene_set_texcoords: NULL array with %u texture coordinates", n_texcoords);
    const size_t nt = s->mesh.n_triangles();
    for (size_t i = 0; i < 2 * (size_t)n_texcoords; i++)
        if (!std::isfinite(texcoords[i])) return fail(MR_ERR_INVALID, "mr_scene_set_texcoords: texture coordinate %zu is not finite", i / 2);
    if (n_texcoords > 0)
        for (size_t i = 0; i < nt; i++) {
            const uint32_t *t = tidx + 3 * i;
            if (t[0] == kNoTexcoord && t[1] == kNoTexcoord && t[2] == kNoTexcoord) continue;
            for (int k = 0; k < 3; k++)
                if (t[k] >= n_texcoords) return fail(MR_ERR_INVALID, "mr_scene_set_texcoords: object %zu has texture coordinate %u of %u", i, t[k], n_texcoords);
        }
    if (n_texcoords > 0) {
        s->mesh.t.assign(texcoords, texcoords + 2 * (size_t)n_texcoords);
        s->mesh.ti.assign(tidx, tidx + 3 * nt);
    } else {
        s->mesh.t.clear();
        s->mesh.ti.clear();
    }
    if (s->on_device) {
        MR_HIP_CHECK(hipSetDevice(s->device));
        MR_HIP_CHECK(hipDeviceSynchronize());
        return upload_texcoords(s);
    }
    return MR_OK;
}

mr_status mr_scene_get_texcoords(const mr_scene *s, uint32_t *n_texcoords, float *texcoords, uint32_t *tidx) {
    if (!s) return fail(MR_ERR_INVALID, "mr_scene_get_texcoords: NULL scene");
    if (n_texcoords) *n_texcoords = (uint32_t)(s->mesh.t.size() / 2);
    if (texcoords && !s->mesh.t.empty()) memcpy(texcoords, s->mesh.t.data(), s->mesh.t.size() * sizeof(float));
    if (tidx)
        for (size_t i = 0; i < s->mesh.vi.size(); i++) tidx[i] = i < s->mesh.ti.size() ? s->mesh.ti[i] : kNoTexcoord;
    return MR_OK;
}

mr_status mr_scene_set_textures(mr_scene *s, const mr_texture_desc *textures, uint32_t n_textures, const uint32_t *material_texture) {
    if (!s) return fail(MR_ERR_INVALID, "mr_scene_set_textures: NULL scene");
    if (n_textures > MR_MAX_TEXTURES) return fail(MR_ERR_INVALID, "mr_scene_set_textures: %u textures, at most %u", n_textures, (unsigned)MR_MAX_TEXTURES);
    if (n_textures > 0 && !textures) return fail(MR_ERR_INVALID, "mr_scene_set_textures: NULL list of %u textures", n_textures);
    if (n_textures == 0) {                     // clears the table (the materials keep the m_diffuse an earlier call gave them)
        s->tex = HostTextures();
        s->tex_dirty = false;
        return MR_OK;
    }
    if (material_texture && s->materials.empty())
        return fail(MR_ERR_INVALID, "mr_scene_set_textures: material_texture without a material table (mr_scene_set_materials)");
    const uint32_t n_mats = s->materials.empty() ? 1u : (uint32_t)(s->materials.size() / 11);
    HostTextures h;
    h.n_textures = n_textures; h.n_materials = n_mats;
    size_t texels = 0;
    for (uint32_t i = 0; i < n_textures; i++) {
        const mr_texture_desc &in = textures[i];
        if (in.kind > MR_TEX_FLOWER_CENTER) return fail(MR_ERR_INVALID, "texture %u: unknown kind %u", i, in.kind);
        // reserved[0] of a STONE texture is its flag word (miro_hip_bump.h): MR_TEX_REFLECTIVE or 0
        for (int k = (in.kind == MR_TEX_STONE && in.reserved[0] == MR_TEX_REFLECTIVE) ? 1 : 0; k < 5; k++)
            if (in.reserved[k] != 0) return fail(MR_ERR_INVALID, "texture %u: mr_texture_desc.reserved must be 0", i);
        if (in.kind == MR_TEX_CHECKER) {
            for (int c = 0; c < 3; c++)
                if (!std::isfinite(in.color1[c]) || !std::isfinite(in.color2[c])) return fail(MR_ERR_INVALID, "texture %u: the checker's colours must be finite", i);
            if (!std::isfinite(in.scale)) return fail(MR_ERR_INVALID, "texture %u: the checker's scale must be finite", i);
        } else if (in.kind == MR_TEX_STONE || in.kind == MR_TEX_STEM) {
            if (!std::isfinite(in.scale)) return fail(MR_ERR_INVALID, "texture %u: the %s texture's scale must be finite", i, in.kind == MR_TEX_STONE ? "stone" : "stem");
            h.procedural = true;
        } else if (in.kind >= MR_TEX_PETAL) {                                    // the UVW kinds: pivot in color1, radius in color2[0]
            if (in.kind != MR_TEX_LEAF && !(in.color2[0] > 0.0f && std::isfinite(in.color2[0])))
                return fail(MR_ERR_INVALID, "texture %u: the radius (color2[0]) of a PETAL or FLOWER_CENTER texture must be finite and greater than 0", i);
            for (int c = 0; c < 3; c++)
                if (!std::isfinite(in.color1[c]) || !std::isfinite(in.color2[c])) return fail(MR_ERR_INVALID, "texture %u: the pivot (color1) and color2 must be finite", i);
            if (!std::isfinite(in.scale)) return fail(MR_ERR_INVALID, "texture %u: the scale must be finite", i);
            h.procedural = true;
        } else {
            if (in.W == 0 || in.H == 0 || !in.pixels) return fail(MR_ERR_INVALID, "texture %u: an image needs pixels and W, H > 0", i);
            if (in.W > 65536u || in.H > 65536u) return fail(MR_ERR_INVALID, "texture %u: image of %u x %u pixels, at most 65536 each way", i, in.W, in.H);
            if (in.hdr > 1) return fail(MR_ERR_INVALID, "texture %u: hdr must be 0 (FIT_BITMAP) or 1 (FIT_RGBF)", i);
            const size_t n = 3 * (size_t)in.W * in.H;
            for (size_t k = 0; k < n; k++)
                if (!std::isfinite(in.pixels[k])) return fail(MR_ERR_INVALID, "texture %u: pixel value %zu is not finite", i, k);
            texels += (size_t)in.W * in.H;
        }
    }
    if (texels >= (1ull << 31)) return fail(MR_ERR_INVALID, "mr_scene_set_textures: %zu texels in all, fewer than 2^31", texels);
    if (material_texture)
        for (uint32_t i = 0; i < n_mats; i++)
            if (material_texture[i] != kNoTexture && material_texture[i] >= n_textures)
                return fail(MR_ERR_INVALID, "material %u names texture %u of %u", i, material_texture[i], n_textures);
    // A bump-mapped material may reflect (ks != 0; the reference's author tried one, assignment1.cpp:134) where its texture says
    // MR_TEX_REFLECTIVE, and may not transmit: the light through a refractive occluder reads the occluder's N (Phong.cpp:99-113),
    // which no shadow loop here bumps, and with kt == 0 a STONE material never is such an occluder.  The flag is the caller's word
    // that it renders the scene through the calls that have the bumped normal: without it the table is refused as it always was,
    // here, at set-up, and not by mr_gen_secondary_rays in the middle of a frame.  A reflective one is remembered
    // (bumped_specular): its mirror
    // child bounces about the normal Scene::trace hands on (Scene.cpp:234-263, Ray.h:156), so every route takes the children's N
    // from the surface step -- mr_gen_secondary_rays_surface and the PATH generators' _surface form from mr_hit_surface's buffer,
    // the BUMPED level kernels (mr_level_lights_bump.hip, mr_level_lights_queued_bump.hip), the fused frames and the PATH level
    // kernels from their own surface step -- and the two generators that compute the object's normal refuse the scene.  The flag
    // holds while the table does: mr_scene_set_materials is refused while a table is set.
    if (material_texture)
        for (uint32_t i = 0; i < n_mats; i++) {
            if (material_texture[i] == kNoTexture || textures[material_texture[i]].kind != MR_TEX_STONE) continue;
            const float *o = &s->materials[11 * (size_t)i];
            for (int c = 6; c < 9; c++)
                if (o[c] != 0.0f)
                    return fail(MR_ERR_INVALID, "material %u names the STONE texture %u and has a non-zero kt: a bump-mapped material "
                                                "has no transmission (light through a refractive occluder reads the occluder's N, "
                                                "Phong.cpp:99-113, and the shadow loops do not bump it); ks may be non-zero",
                                i, material_texture[i]);
            for (int c = 3; c < 6; c++)
                if (o[c] != 0.0f) {
                    if (textures[material_texture[i]].reserved[0] != MR_TEX_REFLECTIVE)
                        return fail(MR_ERR_INVALID, "material %u names the STONE texture %u and has a non-zero ks: a bump-mapped material "
                                                    "reflects only where the texture says MR_TEX_REFLECTIVE (mr_texture_desc.reserved[0], "
                                                    "miro_hip_bump.h: its mirror child bounces about the bumped normal, which "
                                                    "mr_gen_secondary_rays does not have)", i, material_texture[i]);
                    h.bumped_specular = true;
                }
        }

    h.texel_base = 3 * (size_t)n_textures;
    h.mat_base = h.texel_base + texels;
    h.blob.assign(h.mat_base + (n_mats + 3) / 4, make_float4(0.f, 0.f, 0.f, 0.f));
    const auto bits = [](uint32_t v) { float f; memcpy(&f, &v, sizeof(f)); return f; };
    size_t at = 0;
    for (uint32_t i = 0; i < n_textures; i++) {
        const mr_texture_desc &in = textures[i];
        float4 *q = &h.blob[3 * (size_t)i];
        if (in.kind == MR_TEX_CHECKER) {
            q[0] = make_float4(bits(MR_TEX_CHECKER), 0.f, 0.f, 0.f);
            q[1] = make_float4(in.color1[0], in.color1[1], in.color1[2], in.scale);
            q[2] = make_float4(in.color2[0], in.color2[1], in.color2[2], 0.f);
            continue;
        }
        if (in.kind == MR_TEX_STONE || in.kind == MR_TEX_STEM) {                  // the scale where a checker's is
            q[0] = make_float4(bits(in.kind), 0.f, 0.f, 0.f);
            q[1] = make_float4(0.f, 0.f, 0.f, in.scale);
            continue;
        }
        if (in.kind >= MR_TEX_PETAL) {                                            // pivot and scale, then the radius
            q[0] = make_float4(bits(in.kind), 0.f, 0.f, 0.f);
            q[1] = make_float4(in.color1[0], in.color1[1], in.color1[2], in.scale);
            q[2] = make_float4(in.color2[0], 0.f, 0.f, 0.f);
            continue;
        }
        float max_intensity = -1e15;                                              // Texture.cpp:34,41-50
        float4 *px = &h.blob[h.texel_base + at];
        for (size_t k = 0; k < (size_t)in.W * in.H; k++) {
            const float *p = in.pixels + 3 * k;
            for (int c = 0; c < 3; c++)
                if (max_intensity < p[c]) max_intensity = p[c];
            px[k] = make_float4(p[0], p[1], p[2], 0.f);
        }
        q[0] = make_float4(bits(MR_TEX_IMAGE), bits(in.W), bits(in.H), bits((uint32_t)at));
        q[1] = make_float4(max_intensity, bits(in.hdr), 0.f, 0.f);
        at += (size_t)in.W * in.H;
    }
    uint32_t *mat_tex = reinterpret_cast<uint32_t *>(&h.blob[h.mat_base]);
    bool changed = false;
    for (uint32_t i = 0; i < n_mats; i++) {
        mat_tex[i] = material_texture ? material_texture[i] : kNoTexture;
        if (mat_tex[i] == kNoTexture) continue;
        // TexturedPhong::TexturedPhong (Texture.cpp:513-514): Phong(kd = 1, ks, kt, ...), so m_diffuse is what the constructor's
        // clamp (Phong.cpp:29-31) makes of 1, whatever diffuse the caller's mr_material held
        float *o = &s->materials[11 * (size_t)i];
        for (int c = 0; c < 3; c++) {
            const float kd = fmaxf(fminf(1.0f, 1.0f - o[3 + c] - o[6 + c]), 0.f);
            if (o[c] != kd) { o[c] = kd; changed = true; }
        }
    }
    s->tex = std::move(h);
    s->tex_dirty = true;
    if (changed && s->on_device) {
        MR_HIP_CHECK(hipSetDevice(s->device));
        MR_HIP_CHECK(hipDeviceSynchronize());
        return upload_materials(s);
    }
    return MR_OK;
}

mr_status mr_hit_uv(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n, float *d_uv, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_hits || !d_uv) return fail(MR_ERR_INVALID, "NULL argument");
    if (misaligned(16, d_rays, d_hits) || misaligned(4, d_uv))
        return fail(MR_ERR_INVALID, "ray / hit buffers must be 16-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_hit_uv(s->dev, d_rays, d_hits, n, d_uv, static_cast<hipStream_t>(stream));
}

mr_status mr_texture_lookup(mr_scene *s, uint32_t texture, const float *d_uv, uint64_t n, float *d_rgb, uint64_t *d_counts, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (s->tex.blob.empty()) return fail(MR_ERR_STATE, "mr_texture_lookup: the scene has no textures (mr_scene_set_textures)");
    if (texture >= s->tex.n_textures) return fail(MR_ERR_INVALID, "mr_texture_lookup: texture %u of %u", texture, s->tex.n_textures);
    if (!d_uv || !d_rgb) return fail(MR_ERR_INVALID, "NULL argument");
    if (misaligned(4, d_uv, d_rgb) || misaligned(8, d_counts))
        return fail(MR_ERR_INVALID, "float buffers must be 4-byte aligned, counters 8-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    TexParams tex;
    if ((st = texture_params(s, static_cast<hipStream_t>(stream), tex)) != MR_OK) return st;
    uint32_t kind;
    memcpy(&kind, &s->tex.blob[3 * (size_t)texture].x, sizeof(kind));
    if (kind >= MR_TEX_PETAL)                  // lookup2D of a Texture3D is the base class's black (Texture.h:66): nobody wants that silently
        return fail(MR_ERR_INVALID, "mr_texture_lookup: texture %u is a UVW texture (kind %u); mr_texture_lookup3 looks it up at points", texture, kind);
    if (kind == MR_TEX_STONE || kind == MR_TEX_STEM)
        return launch_texture_lookup_proc(tex, texture, d_uv, n, d_rgb, reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
    return launch_texture_lookup(tex, texture, d_uv, n, d_rgb, reinterpret_cast<unsigned long long *>(d_counts), static_cast<hipStream_t>(stream));
}

mr_status mr_hit_surface(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n, float *d_color, float *d_normal,
                         uint64_t *d_counts, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_hits || !d_color || !d_normal) return fail(MR_ERR_INVALID, "mr_hit_surface: NULL argument");
    if (misaligned(16, d_rays, d_hits) || misaligned(4, d_color, d_normal) || misaligned(8, d_counts))
        return fail(MR_ERR_INVALID, "mr_hit_surface: ray / hit buffers must be 16-byte aligned, float buffers 4-byte, counters 8-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    TexParams tex;
    tex.recs = nullptr; tex.texels = nullptr; tex.mat_tex = nullptr; tex.texcoords = s->dev.texcoords; tex.ti = s->dev.ti;
    if (!s->tex.blob.empty() && (st = texture_params(s, static_cast<hipStream_t>(stream), tex)) != MR_OK) return st;
    return launch_hit_surface(s->dev, tex, d_rays, d_hits, n, d_color, d_normal, reinterpret_cast<unsigned long long *>(d_counts),
                              static_cast<hipStream_t>(stream));
}

mr_status mr_shade_lights_surface(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color, const float *d_normal,
                                  const float *d_weights, const uint32_t *d_pixels, uint64_t n, uint32_t spp, uint32_t flags,
                                  float *d_rgb, float *d_ray_rgb, uint64_t *d_counts, void *stream) {
    const mr_status st = check_shade_lights("mr_shade_lights_surface", s, d_rays, d_hits, !d_color || !d_normal,
                                            misaligned(4, d_color, d_normal), n, spp,
                                            flags, d_rgb, d_ray_rgb, d_counts);
    if (st != MR_OK) return st;
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_shade_lights_surf(s->dev, s->lights.data(), (uint32_t)s->lights.size(), d_rays, d_hits, d_color, d_normal, d_weights, d_pixels,
                                    n, spp, flags, d_rgb, d_ray_rgb, reinterpret_cast<unsigned long long *>(d_counts),
                                    static_cast<hipStream_t>(stream));
}

mr_status mr_shade_accumulate_surface(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, const float *d_color, const float *d_normal,
                                      const float *d_weights, const uint32_t *d_pixels, uint64_t n, const mr_ray *d_shadow_rays,
                                      const mr_hit *d_shadow_hits, const uint32_t *d_shadow_src, const uint64_t *d_shadow_count,
                                      const mr_light *light, uint32_t spp, float *d_rgb, void *stream) {
    mr_status st = check_shade_accumulate("mr_shade_accumulate_surface", s, d_rays, d_hits, !d_color || !d_normal, d_shadow_rays,
                                          d_shadow_hits, d_shadow_src, d_shadow_count, light, spp, d_rgb);
    if (st != MR_OK) return st;
    if (misaligned(4, d_color, d_normal))
        return fail(MR_ERR_INVALID, "mr_shade_accumulate_surface: float buffers must be 4-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    if ((st = reserve_light_scale(s, n)) != MR_OK) return st;
    const hipStream_t q = static_cast<hipStream_t>(stream);
    if ((st = launch_light_scale(s->dev, d_shadow_rays, d_shadow_hits, d_shadow_src, reinterpret_cast<const unsigned long long *>(d_shadow_count),
                                 n, s->d_light_scale, q)) != MR_OK)
        return st;
    return launch_shade_accumulate_surf(s->dev, d_rays, d_hits, d_color, d_normal, d_weights, d_pixels, n, s->d_light_scale, *light, spp, d_rgb, q);
}

mr_status mr_texture_bump_height(mr_scene *s, uint32_t texture, const float *d_uv, uint64_t n, float *d_height, void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (s->tex.blob.empty()) return fail(MR_ERR_STATE, "mr_texture_bump_height: the scene has no textures (mr_scene_set_textures)");
    if (texture >= s->tex.n_textures) return fail(MR_ERR_INVALID, "mr_texture_bump_height: texture %u of %u", texture, s->tex.n_textures);
    if (!d_uv || !d_height) return fail(MR_ERR_INVALID, "mr_texture_bump_height: NULL argument");
    if (misaligned(4, d_uv, d_height))
        return fail(MR_ERR_INVALID, "mr_texture_bump_height: float buffers must be 4-byte aligned");
    MR_HIP_CHECK(hipSetDevice(s->device));
    uint32_t kind;
    memcpy(&kind, &s->tex.blob[3 * (size_t)texture].x, sizeof(kind));
    return launch_bump_height(kind == MR_TEX_STONE, s->tex.blob[3 * (size_t)texture + 1].w, d_uv, n, d_height, static_cast<hipStream_t>(stream));
}

mr_status mr_texture_lookup3(mr_scene *s, uint32_t texture, const float *d_p, uint64_t n, float *d_rgb, float *d_coords, uint64_t *d_counts,
                             void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (s->tex.blob.empty()) return fail(MR_ERR_STATE, "mr_texture_lookup3: the scene has no textures (mr_scene_set_textures)");
    if (texture >= s->tex.n_textures) return fail(MR_ERR_INVALID, "mr_texture_lookup3: texture %u of %u", texture, s->tex.n_textures);
    if (!d_p || !d_rgb) return fail(MR_ERR_INVALID, "mr_texture_lookup3: NULL argument");
    if (misaligned(4, d_p, d_rgb, d_coords) || misaligned(8, d_counts))
        return fail(MR_ERR_INVALID, "mr_texture_lookup3: float buffers must be 4-byte aligned, counters 8-byte aligned");
    uint32_t kind;
    memcpy(&kind, &s->tex.blob[3 * (size_t)texture].x, sizeof(kind));
    if (kind < MR_TEX_PETAL)
        return fail(MR_ERR_INVALID, "mr_texture_lookup3: texture %u is a UV texture (kind %u); mr_texture_lookup looks it up at coordinates", texture, kind);
    MR_HIP_CHECK(hipSetDevice(s->device));
    TexParams tex;
    if ((st = texture_params(s, static_cast<hipStream_t>(stream), tex)) != MR_OK) return st;
    return launch_texture_lookup3(tex, texture, d_p, n, d_rgb, d_coords, reinterpret_cast<unsigned long long *>(d_counts),
                                  static_cast<hipStream_t>(stream));
}

mr_status mr_noise_probe(uint32_t which, const float *d_in, uint64_t n, float *d_out, void *stream) {
    if (which != MR_NOISE_PERLIN && which != MR_NOISE_WORLEY2) return fail(MR_ERR_INVALID, "mr_noise_probe: which must be MR_NOISE_PERLIN or MR_NOISE_WORLEY2");
    if (!d_in || !d_out) return fail(MR_ERR_INVALID, "mr_noise_probe: NULL argument");
    if (misaligned(4, d_in, d_out))
        return fail(MR_ERR_INVALID, "mr_noise_probe: buffers must be 4-byte aligned");
    return launch_noise_probe(which, d_in, n, d_out, static_cast<hipStream_t>(stream));
}

mr_status mr_tonemap(mr_scene *s, const float *d_rgb, uint64_t n_values, uint8_t *d_out, void *stream) {
    if (!s || !d_rgb || !d_out) return fail(MR_ERR_INVALID, "NULL argument");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_tonemap(d_rgb, n_values, d_out, static_cast<hipStream_t>(stream));
}

// Scene.cpp:150-163, 184-197 and Image.cpp:47-52 (include/miro_hip_passes.h).  The first call allocates the scene's three state
// words and must lie outside a stream capture; after it the call is two kernels on `stream`
mr_status mr_finish_image(mr_scene *s, const float *d_rgb, uint64_t n_pixels, uint8_t *d_out8, float *d_minmax, void *stream) {
    const char *who = "mr_finish_image";
    if (!s || !d_rgb || !d_out8) return fail(MR_ERR_INVALID, "%s: NULL argument", who);
    if (n_pixels == 0) return fail(MR_ERR_INVALID, "%s: empty image", who);
    if (n_pixels > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "%s: at most 2^32 - 1 pixels", who);
    if (misaligned(4, d_rgb, d_minmax)) return fail(MR_ERR_INVALID, "%s: d_rgb and d_minmax must be 4-byte aligned", who);
    MR_HIP_CHECK(hipSetDevice(s->device));
    if (!s->d_finish_state) {
        const uint32_t identity[3] = {kFinishMaxIdentity, kFinishMinIdentity, 0u};
        MR_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&s->d_finish_state), sizeof(identity)));
        MR_HIP_CHECK(hipMemcpy(s->d_finish_state, identity, sizeof(identity), hipMemcpyHostToDevice));
    }
    return launch_finish_image(d_rgb, 3ull * n_pixels, d_out8, d_minmax, s->d_finish_state, static_cast<hipStream_t>(stream));
}

mr_status mr_untile_pixels(mr_scene *s, const float *d_slots, float *d_image, uint32_t W, uint32_t rows, uint32_t spp,
                           uint32_t channels, void *stream) {
    if (!s || !d_slots || !d_image) return fail(MR_ERR_INVALID, "NULL argument");
    if (d_slots == d_image) return fail(MR_ERR_INVALID, "mr_untile_pixels does not work in place");
    if (channels == 0 || spp == 0) return fail(MR_ERR_INVALID, "channels and spp must be positive");
    if ((uint64_t)W * rows > 0xFFFFFFFFull) return fail(MR_ERR_INVALID, "window of more than 2^32-1 pixels");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_untile(d_slots, d_image, W, rows, spp, channels, static_cast<hipStream_t>(stream));
}

mr_status mr_hit_attrs(mr_scene *s, const mr_ray *d_rays, const mr_hit *d_hits, uint64_t n, float *d_P, float *d_N,
                       void *stream) {
    mr_status st = require_device(s);
    if (st != MR_OK) return st;
    if (!d_hits) return fail(MR_ERR_INVALID, "d_hits is NULL");
    MR_HIP_CHECK(hipSetDevice(s->device));
    return launch_hit_attrs(s->dev, d_rays, d_hits, n, d_P, d_N, static_cast<hipStream_t>(stream));
}

}  // extern "C"
