"""Time of the surface pass (mr_hit_surface, hit_surface_kernel of mr_procedural.hip) over 2^20 hits of ONE material: an
all-stone batch (five Worley searches, up to 33 Perlin evaluations and the bump per hit), an all-petal batch (up to 35 Perlin
evaluations per hit) and a plain batch (no texture table: the material's kd and the normalised normal, the memory-bound path
where the kernel's fixed overhead shows first).  The scene is a floor plane under seeded rays that all hit it.  HIP events
around windows of --calls back-to-back calls; one warm-up window per row, then the rows alternate for --repeats timed windows
each.  Prints one JSON line; needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

NONE = 0xFFFFFFFF
TEXTURES = dict(stone=dict(stone=3.0), petal=dict(petal=((0.0, -0.5, 0.0), 7.0)), plain=None)   # None: no texture table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=20, help="timed windows per row, the rows alternating")
    ap.add_argument("--calls", type=int, default=100, help="back-to-back calls per window")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "surface_probe needs the GPU"
    import miro_amd
    s = miro_amd.Scene(0)
    s.add_triangle([40, 0, 40, 41, 0, 40, 40, 1, 40], [0, 0, 1] * 3)     # far away: a scene needs one bounded object
    s.add_plane((0, 1, 0), (0, -0.5, 0), 0)
    s.build(4)
    s.set_materials([((1, 1, 1), (0, 0, 0), (0, 0, 0), 20.0, 1.0), ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 20.0, 1.0)], [1])
    n = a.hits
    rng = np.random.default_rng(9)
    o = np.stack([rng.uniform(-1, 1, n), rng.uniform(2, 4, n), rng.uniform(-1, 1, n)], 1)
    d = np.stack([rng.uniform(-6, 6, n), np.full(n, -0.5), rng.uniform(-6, 6, n)], 1) - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-4, d, 1e30
    assert miro_amd.RAY_DTYPE.names[:8] == ("ox", "oy", "oz", "tmin", "dx", "dy", "dz", "tmax"), miro_amd.RAY_DTYPE.names
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    s.trace_device(d_rays, n, d_hits)
    color = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    normal = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    hit = int((d_hits.cpu().numpy().view(np.uint32)[:, 1] != NONE).sum())
    assert hit == n, (hit, n)

    undefined = {}

    def window(name):
        """milliseconds per call over a window of --calls back-to-back calls"""
        if TEXTURES[name] is None:
            s.set_textures([])
        else:
            s.set_textures([TEXTURES[name]], [0, NONE])
        counts.zero_()
        s.hit_surface(d_rays, d_hits, n, color, normal, d_counts=counts)  # uploads the table; not timed
        torch.cuda.synchronize()
        undefined[name] = int(counts.item())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            s.hit_surface(d_rays, d_hits, n, color, normal, d_counts=counts)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    for name in TEXTURES:
        window(name)
    ms = {name: [] for name in TEXTURES}
    for _ in range(a.repeats):
        for name in TEXTURES:
            ms[name].append(window(name))
    out = dict(hits=n, repeats=a.repeats, calls_per_window=a.calls, device=torch.cuda.get_device_name(0), undefined_per_call=undefined)
    for name, v in ms.items():
        v = np.asarray(v)
        out[name] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4),
                         mhits_per_s=round(n / float(np.median(v)) / 1e3, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
