"""Time of the square light on one untextured batch, both ways: mr_shade_square_lights (the yardstick: it computes the hit's N and
reads the material's colour itself) against mr_hit_surface + mr_shade_square_lights_surface (the two buffers written, then read).
The batch is the primary hits of the teapot frame at --size x --size, one light, --samples shadow rays per hit.  HIP events around
windows of --calls back-to-back calls; one warm-up window per row, then the rows alternate for --repeats timed windows each.  The
two calls' d_ray_rgb are compared first.  Prints one JSON line; needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

LIGHT = dict(position=(0.0, 8.0, 0.0), normal=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0), wattage=300.0, dimensions=(2.0, 2.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per row, the rows alternating")
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per window")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "square_surface_probe needs the GPU"
    import miro_amd
    from miro_amd import binding, scenes
    desc = scenes.SCENES["teapot"]
    s = miro_amd.Scene(0)
    scenes.populate(s, desc)
    s.build(4)
    n = a.size * a.size
    f32 = dict(dtype=torch.float32, device="cuda")
    rays, hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
    s.gen_eye_rays(binding.make_camera(desc["eye"], desc["lookat"], desc["up"], desc["fov"]), a.size, a.size, rays)
    s.trace_device(rays, n, hits)
    color, normal = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
    rgb, cnt = torch.zeros((n, 3), **f32), torch.zeros(1, dtype=torch.int64, device="cuda")
    per_ray = {k: torch.zeros((n, 3), **f32) for k in ("plain", "surface")}

    def plain(out=None):
        s.shade_square_lights([LIGHT], a.samples, rays, hits, n, rgb, d_ray_rgb=out, d_counts=cnt)

    def surface_pass(out=None):
        s.hit_surface(rays, hits, n, color, normal)

    def surface(out=None):
        s.shade_square_lights_surface([LIGHT], a.samples, rays, hits, color, normal, n, rgb, d_ray_rgb=out, d_counts=cnt)

    def both(out=None):
        surface_pass()
        surface(out)

    rows = dict(plain=plain, surface_pass=surface_pass, surface=surface, surface_pass_and_surface=both)
    plain(per_ray["plain"])
    both(per_ray["surface"])
    torch.cuda.synchronize()
    shadow_rays = int(cnt.item()) // 2
    differ = int((per_ray["plain"] != per_ray["surface"]).any(dim=1).sum().item())

    def window(name):
        """milliseconds per call over a window of --calls back-to-back calls"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            rows[name]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    for name in rows:
        window(name)
    ms = {name: [] for name in rows}
    for _ in range(a.repeats):
        for name in rows:
            ms[name].append(window(name))
    out = dict(scene="teapot", rays=n, samples=a.samples, shadow_rays_per_call=shadow_rays, rays_whose_L_differs=differ, repeats=a.repeats,
               calls_per_window=a.calls, device=torch.cuda.get_device_name(0))
    for name, v in ms.items():
        v = np.asarray(v)
        out[name] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4))
    out["surface_pass_and_surface_over_plain"] = round(out["surface_pass_and_surface"]["median_ms"] / out["plain"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
