"""Launch time of the path-tracing generators on one untextured first-bounce queue, both ways: mr_gen_path_rays (the yardstick: it
computes every hit's N and reads the material's colour itself) against mr_gen_path_rays_surface (N and colour read from
mr_hit_surface's two buffers, 24 bytes per listed ray).  The queue is the one tools/level_probe.py starts from: the primary hits
of --scene at --w x --h x --spp in tiled order, kinds = MR_PATH_DIFFUSE, seed 5.  Every launch sits between two HIP events; a
repetition is the median of --launches launches after --warmup untimed ones, the rows alternate for --reps repetitions.  The two
calls' children are compared first (count, sorted ids, weight sum).  --plain-only: the plain call alone, for a library that has
no surface form (the parent commit's, loaded with its own miro_amd package on PYTHONPATH).  Prints one JSON line; needs the GPU
(no fallback)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
try:
    import miro_amd                                             # a package given on PYTHONPATH (an A/B checkout) wins
except ImportError:
    sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))
    import miro_amd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bunny")
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--h", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "path_surface_probe needs the GPU"
    from miro_amd import binding, scenes
    from miro_amd import frame as mframe
    d = scenes.SCENES[a.scene]
    sc = miro_amd.Scene(0)
    scenes.populate(sc, d)
    sc.build(4)
    fr = mframe.FrameRenderer(sc, d, a.w, a.h, spp=a.spp, tiled=True)
    fr.generate()
    n = fr.n
    f32 = dict(dtype=torch.float32, device="cuda")
    rays, hits = fr.d_rays, torch.empty((n, 4), **f32)
    sc.trace_device(rays, n, hits)
    out = dict(plain=None, surface=None)
    for name in out:                                            # kinds = MR_PATH_DIFFUSE: one child per ray at most
        out[name] = (torch.empty((n, 8), **f32), torch.empty((n, 3), **f32), torch.empty(n, dtype=torch.int32, device="cuda"),
                     torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    kw = dict(spp=a.spp, seed=5, bounce=0, kinds=binding.MR_PATH_DIFFUSE)

    def plain():
        o = out["plain"]
        sc.gen_path_rays(rays, hits, None, None, None, n, o[0], o[1], o[2], o[3], o[4], **kw)

    rows = dict(plain=plain)
    if not a.plain_only:
        color, normal = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
        sc.hit_surface(rays, hits, n, color, normal)

        def surface():
            o = out["surface"]
            sc.gen_path_rays_surface(rays, hits, color, normal, None, None, None, n, o[0], o[1], o[2], o[3], o[4], **kw)

        rows["surface"] = surface
    for f in rows.values():
        f()
    torch.cuda.synchronize()
    line = dict(tool="path_surface_probe", library=os.path.relpath(os.environ.get("MIRO_LIB") or binding.lib_path(), ROOT),
                scene=a.scene, rays=n, children=int(out["plain"][4].item()), launches=a.launches, warmup=a.warmup, reps=a.reps,
                device=torch.cuda.get_device_name(0))
    if not a.plain_only:
        m = line["children"]
        p, s = out["plain"], out["surface"]
        same = int(s[4].item()) == m and bool(torch.equal(torch.sort(p[3][:m])[0], torch.sort(s[3][:m])[0]))
        line["children_equal"] = same and float(p[1][:m].double().sum()) == float(s[1][:m].double().sum())

    def repetition(f):
        """median launch time in ms over --launches launches, each between two events, after --warmup untimed ones"""
        for _ in range(a.warmup):
            f()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for e0, e1 in ev:
            e0.record()
            f()
            e1.record()
        torch.cuda.synchronize()
        return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)

    ms = {name: [] for name in rows}
    for _ in range(a.reps):
        for name, f in rows.items():
            ms[name].append(repetition(f))
    for name, v in ms.items():
        line[name + "_ms"] = dict(median=round(statistics.median(v), 4), lo=round(min(v), 4), hi=round(max(v), 4), reps=[round(x, 4) for x in v])
    print(json.dumps(line))


if __name__ == "__main__":
    main()
