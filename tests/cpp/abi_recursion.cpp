// A whole recursive frame through the C ABI alone: Scene::raytraceImage -> Scene::traceScene (Scene.cpp:94-346) as ONE call,
// mr_render_recursion -- no Python, no torch, no per-level driver: g++, include/miro_hip.h, libmiro_hip.so and the HIP runtime for
// the device buffers.
//
//   scene:  a glass sphere (kd = 0, ks = 0.05, kt = 0.9, index 1.5) of radius 1 at the origin under one point light, and one
//           far triangle (a scene needs one bounded object): the scene of tests/test_level_lights_path.py
//   frame:  every level of the recursion on one stream; the host reads the counters once, afterwards
//
// usage: abi_recursion <W> <H> <spp> <depth> <specular | path> <queue capacity | 0 = fan x samples>
// Prints "level <l> <8 counters>" per level, "truncated <l>" for a level whose children did not fit, and "checksum <hex>": FNV-1a
// over the bytes of d_rgb.  The counters are exact; levels >= 1 add with float atomics, so where a pixel receives several
// additions of one level the last bits of the pixels, and with them the checksum, may differ from run to run.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "miro_hip.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 10; } } while (0)
#define MR_OK_(x) do { if ((x) != MR_OK) { fprintf(stderr, "%s: %s\n", #x, mr_last_error()); return 11; } } while (0)

int main(int argc, char **argv) {
    if (argc < 7) { fprintf(stderr, "usage: abi_recursion <W> <H> <spp> <depth> <specular | path> <queue capacity | 0>\n"); return 2; }
    const uint32_t W = (uint32_t)atoi(argv[1]), H = (uint32_t)atoi(argv[2]), spp = (uint32_t)atoi(argv[3]);
    const uint32_t depth = (uint32_t)atoi(argv[4]);
    const bool path = strcmp(argv[5], "path") == 0;
    uint64_t capacity = (uint64_t)atoll(argv[6]);
    const uint64_t npix = (uint64_t)W * H, samples = npix * spp;
    if (capacity == 0) capacity = (path ? 4u : 3u) * samples;

    mr_scene *scene = 0;
    MR_OK_(mr_scene_create(0, &scene));
    const float tri[9] = {40, 0, 40, 41, 0, 40, 40, 1, 40}, nrm[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
    const float centre[3] = {0.0f, 0.0f, 0.0f};
    MR_OK_(mr_scene_add_triangle(scene, tri, nrm));
    MR_OK_(mr_scene_add_sphere(scene, centre, 1.0f, 0));
    mr_material mats[2];
    memset(mats, 0, sizeof(mats));
    mats[0].diffuse[0] = mats[0].diffuse[1] = mats[0].diffuse[2] = 0.5f;
    mats[0].shininess = 1.0f; mats[0].refract_index = 1.0f;
    for (int c = 0; c < 3; c++) { mats[1].specular[c] = 0.05f; mats[1].transmission[c] = 0.9f; }
    mats[1].shininess = 80.0f; mats[1].refract_index = 1.5f;
    const uint32_t object_material[2] = {0, 1};
    MR_OK_(mr_scene_set_materials(scene, mats, 2, object_material));
    MR_OK_(mr_bvh_build(scene, 0));
    mr_light_desc light;
    memset(&light, 0, sizeof(light));
    light.kind = MR_LIGHT_POINT;
    light.position[0] = 3.0f; light.position[1] = 4.0f; light.position[2] = 5.0f;
    light.color[0] = light.color[1] = light.color[2] = 1.0f;
    light.wattage = 50.0f;
    MR_OK_(mr_scene_set_lights(scene, &light, 1));

    mr_frame_desc fd;
    memset(&fd, 0, sizeof(fd));
    fd.camera.eye[2] = 5.0f;                                   // eye (0, 0, 5), lookat the origin, up y, fov 30
    fd.camera.up[1] = 1.0f;
    fd.camera.fov_deg = 30.0f;
    fd.W = W; fd.H = H; fd.y0 = 0; fd.y1 = H;
    fd.band_rows = 1; fd.band_rank = 0; fd.band_world = 1;
    fd.spp = spp; fd.jitter = spp > 1; fd.seed = 168;
    mr_recursion_desc rd;
    memset(&rd, 0, sizeof(rd));
    rd.depth = depth;
    rd.children = path ? MR_LEVEL_PATH : MR_LEVEL_SPECULAR;
    rd.path_kinds = MR_PATH_MIRROR | MR_PATH_REFRACT | MR_PATH_DIFFUSE; rd.path_seed = 168;
    rd.queue_capacity_lo = (uint32_t)capacity; rd.queue_capacity_hi = (uint32_t)(capacity >> 32);

    uint64_t ws_bytes = 0;
    MR_OK_(mr_render_recursion_workspace(&rd, &ws_bytes));
    float *d_rgb = 0;
    void *d_ws = 0;
    uint64_t *d_counts = 0;
    HIP_OK(hipMalloc((void **)&d_rgb, npix * 3 * sizeof(float)));
    if (ws_bytes) HIP_OK(hipMalloc(&d_ws, ws_bytes));
    HIP_OK(hipMalloc((void **)&d_counts, (depth + 1) * 8 * sizeof(uint64_t)));
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));

    MR_OK_(mr_render_recursion(scene, &fd, &rd, d_rgb, d_ws, ws_bytes, d_counts, stream));
    std::vector<float> rgb(npix * 3);
    std::vector<uint64_t> counts((depth + 1) * 8);
    HIP_OK(hipMemcpyAsync(rgb.data(), d_rgb, rgb.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));                      // the one wait of the frame

    for (uint32_t l = 0; l <= depth; l++) {
        printf("level %u", l);
        for (int k = 0; k < 8; k++) printf(" %llu", (unsigned long long)counts[8 * l + k]);
        printf("\n");
        if (counts[8 * l + 5] > capacity) printf("truncated %u\n", l);
    }
    uint64_t h = 1469598103934665603ull;                       // FNV-1a over the pixels' bytes
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(rgb.data());
    for (size_t k = 0; k < rgb.size() * sizeof(float); k++) { h ^= bytes[k]; h *= 1099511628211ull; }
    printf("checksum %016llx\n", (unsigned long long)h);

    hipFree(d_rgb); hipFree(d_ws); hipFree(d_counts);
    hipStreamDestroy(stream);
    mr_scene_destroy(scene);
    return 0;
}
