"""Timing of mr_shade_environment (csrc/mr_environment.hip) next to mr_gen_shadow_rays, the existing streaming kernel with
comparable bytes per ray, on the same traced batches:
  bunny      the 16.8 M-ray first level of the bunny frame at 1024 x 1024 x 16 spp (few rays miss)
  half-miss  16 M seeded rays around the unit sphere of the `sphere` scene (about half of them miss), 1 spp
in the three modes of the kernel: image (full resolution), low-res (MR_ENV_LOWRES) and colour only.  Device events around every
repetition, both kernels alternating after a warm-up; median and spread.  Bytes per ray are what the kernel has to read and
write, counted here from the batch: 16 B of hit record per ray, 16 B of direction per miss (colour only: none), four 16 B
texels per miss from the full image (low-res: from LDS), 12 B of pixel per atomic run head -- the GB/s figure divides the
streamed part (hit records + directions) by the median time.  Prints one JSON line.
usage: python tools/environment_probe.py [--reps 20] [--small] [--out profiles/environment_line.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))
import numpy as np, torch
import miro_amd
from miro_amd import binding, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--small", action="store_true", help="a rehearsal size")
ap.add_argument("--out", default="")
a = ap.parse_args()
f32 = dict(dtype=torch.float32, device="cuda")


def stats(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def sky(W=2048, H=1024, seed=168):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((H, W, 3), generator=g) ** 4 * 2.0 + 0.3
    img[H // 3, W // 5] = 400.0
    return img.numpy()


def batch(name, n, spp, rays):
    d = scenes.SCENES[name]
    sc = miro_amd.Scene(0)
    scenes.populate(sc, d)
    sc.build(4)
    if rays is None:
        side = int(round((n // spp) ** 0.5))
        n = side * side * spp
        rays = torch.empty((n, 8), **f32)
        sc.gen_eye_rays(binding.make_camera(d["eye"], d["lookat"], d["up"], d["fov"]), side, side, rays, spp=spp, jitter=True)
    hits = torch.empty((n, 4), **f32)
    sc.trace_device(rays, n, hits)
    misses = int((hits[:, 1].view(torch.int32) == -1).sum())
    rgb = torch.zeros((n // spp, 3), **f32)
    sh_rays = torch.empty((n, 8), **f32)
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = dict(rays=n, spp=spp, misses=misses, miss_rate=misses / n)
    modes = (("image", dict(pixels=sky(), rotation=(1.0972, 0.3927)), 0), ("lowres", dict(pixels=sky(), rotation=(1.0972, 0.3927)), binding.MR_ENV_LOWRES),
             ("colour", dict(bg_color=(0.3, 0.2, 0.1)), 0))
    for mode, env, flags in modes:
        sc.set_environment(**env)
        shade = lambda: sc.shade_environment(rays, hits, n, rgb, spp=spp, flags=flags)
        shadow = lambda: sc.gen_shadow_rays(rays, hits, n, d["light"], sh_rays, src, cnt)
        for _ in range(3):
            shade(); shadow()
        te, ts = [], []
        for _ in range(a.reps):
            te.append(timed(shade)); ts.append(timed(shadow))
        streamed = 16 * n + (0 if mode == "colour" else 16 * misses)
        shadow_bytes = 48 * n + 36 * (n - misses)
        out[mode] = dict(shade_environment=stats(te), gen_shadow_rays=stats(ts), streamed_bytes_per_ray=streamed / n,
                         texel_bytes_per_ray=(64 * misses / n if mode == "image" else 0.0),
                         streamed_GBps=streamed / (np.median(te) * 1e-3) / 1e9,
                         gen_shadow_rays_bytes_per_ray=shadow_bytes / n, gen_shadow_rays_GBps=shadow_bytes / (np.median(ts) * 1e-3) / 1e9)
    return out


n_half = 1 << (18 if a.small else 24)
g = torch.Generator(device="cuda").manual_seed(168)
r = torch.zeros((n_half, 8), **f32)
r[:, 0:3] = torch.rand((n_half, 3), generator=g, **f32) * 3.0 - 1.5
dirs = torch.randn((n_half, 3), generator=g, **f32)
r[:, 4:7] = dirs / dirs.norm(dim=1, keepdim=True)
r[:, 7] = 1e12
line = dict(tool="environment_probe", reps=a.reps, device=torch.cuda.get_device_name(0), batches={})
line["batches"]["bunny_1024x1024x16_first_level"] = batch("bunny", (256 if a.small else 1024) ** 2 * 16, 16, None)
line["batches"]["half_miss_16M"] = batch("sphere", n_half, 1, r)
txt = json.dumps(line)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(txt + "\n")
