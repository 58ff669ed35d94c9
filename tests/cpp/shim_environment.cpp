// The environment through the C++ shim, the way the reference's scene code sets it (assignment3.cpp:50-52): a mesh scene,
// Scene::setEnvironment(new LoadedTexture(...)) / setEnvironmentRotation / setBgColor, preCalc(); then one batch of rays read
// from a file is traced (mr_trace) and its misses shaded (mr_shade_environment) on the scene's handle, and d_ray_rgb is
// written out for the Python test to compare with its own path, byte for byte.  Device buffers come from the HIP runtime.
//
// usage: shim_environment <model.obj> <image.bin | -> <W> <H> <phi> <theta> <r,g,b> <rays.bin> <out.bin> <lowres 0|1>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "miro_shim.hpp"

using namespace miro;

namespace miro { class Material { public: int id; }; }

#define HIP_OK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed\n", #x); return 9; } } while (0)

int main(int argc, char **argv) {
    if (argc < 11) { fprintf(stderr, "usage\n"); return 2; }
    Scene scene;
    Material white; white.id = 7;
    TriangleMesh mesh;
    if (!mesh.load(argv[1])) { fprintf(stderr, "cannot load %s\n", argv[1]); return 3; }
    std::vector<Object *> keep;
    for (int i = 0; i < mesh.numTris(); ++i) {
        Triangle *t = new Triangle;
        t->setIndex(i);
        t->setMesh(&mesh);
        t->setMaterial(&white);
        scene.addObject(t);
        keep.push_back(t);
    }
    const int W = atoi(argv[3]), H = atoi(argv[4]);
    LoadedTexture *tex = 0;
    if (strcmp(argv[2], "-") != 0) {
        FILE *fi = fopen(argv[2], "rb");
        if (!fi) return 4;
        std::vector<float> px(3 * (size_t)W * H);
        if (fread(px.data(), 12, (size_t)W * H, fi) != (size_t)W * H) return 4;
        fclose(fi);
        tex = new LoadedTexture(px.data(), W, H);
    }
    float bg[3];
    if (sscanf(argv[7], "%f,%f,%f", bg, bg + 1, bg + 2) != 3) return 5;
    try {
        scene.setEnvironment(tex);                                   // before preCalc(): applied there
        scene.setBgColor(Vector3(bg[0], bg[1], bg[2]));
        scene.preCalc();
        scene.setEnvironmentRotation((float)atof(argv[5]), (float)atof(argv[6]));   // after it: applied at once
    } catch (const MiroHipError &e) { fprintf(stderr, "%s\n", e.what()); return 6; }

    FILE *fp = fopen(argv[8], "rb");
    if (!fp) return 7;
    fseek(fp, 0, SEEK_END);
    const size_t n = (size_t)ftell(fp) / 32;
    fseek(fp, 0, SEEK_SET);
    std::vector<mr_ray> rays(n);
    if (fread(rays.data(), 32, n, fp) != n) return 7;
    fclose(fp);

    mr_ray *d_rays = 0;
    mr_hit *d_hits = 0;
    float *d_ray_rgb = 0;
    HIP_OK(hipMalloc((void **)&d_rays, n * sizeof(mr_ray)));
    HIP_OK(hipMalloc((void **)&d_hits, n * sizeof(mr_hit)));
    HIP_OK(hipMalloc((void **)&d_ray_rgb, 3 * n * sizeof(float)));
    HIP_OK(hipMemcpy(d_rays, rays.data(), n * sizeof(mr_ray), hipMemcpyHostToDevice));
    std::vector<float> out(3 * n);
    try {
        check(mr_trace(scene.handle(), d_rays, n, d_hits, MR_RAYS_ON_DEVICE | MR_HITS_ON_DEVICE, 0));
        check(mr_shade_environment(scene.handle(), d_rays, d_hits, 0, 0, 0, n, 1, atoi(argv[10]) ? MR_ENV_LOWRES : 0, 0, d_ray_rgb, 0, 0));
    } catch (const MiroHipError &e) { fprintf(stderr, "%s\n", e.what()); return 8; }
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), d_ray_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    FILE *fo = fopen(argv[9], "wb");
    if (!fo) return 10;
    fwrite(out.data(), 12, n, fo);
    fclose(fo);
    printf("shim_environment: %zu rays\n", n);
    (void)hipFree(d_rays); (void)hipFree(d_hits); (void)hipFree(d_ray_rgb);
    for (size_t i = 0; i < keep.size(); i++) delete keep[i];
    delete tex;
    return 0;
}
