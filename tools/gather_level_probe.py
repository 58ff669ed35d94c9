"""Timing of mr_gather_level on the queues of a recursion: the photon_room of miro_amd.scenes, its global and caustic maps
traced by mr_trace_photons and balanced on the device, then per level of a depth-`--depth` frame (trace_device -> gather_level
-> gen_secondary_rays, as FrameRenderer.render_specular queues them): rays, queries (d_counts of one counted call) and the
median time of `--reps` calls after one warm-up call, device events around the call (query kernel, one estimate per map,
accumulate kernel).  Two frames: the tests' (48 x 48, 6000 + 2500 photons, k = 50, max_dist 0.35) and a frame a user would run
(--width squared, --photons per map as Scene.h:67-68, k = PHOTON_SAMPLES, max_dist = PHOTON_MAX_DIST).  Prints one JSON line.
usage: python tools/gather_level_probe.py [--width 512] [--photons 200000] [--k 500] [--reps 5] [--out profiles/gather_level_line.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))
import numpy as np, torch
import miro_amd
from miro_amd import binding, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=512)
ap.add_argument("--photons", type=int, default=200000)
ap.add_argument("--k", type=int, default=500)
ap.add_argument("--max-dist", type=float, default=1e10)
ap.add_argument("--depth", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()

desc = scenes.SCENES["photon_room"]
sc = miro_amd.Scene(0)
scenes.populate(sc, desc)
sc.set_materials(desc["materials"], desc["prim_material"])
sc.build(4)
f32 = dict(dtype=torch.float32, device="cuda")


def maps_of(targets):
    out = []
    for caustic, target in ((False, targets[0]), (True, targets[1])):
        m = miro_amd.PhotonMap(target + 64)
        r = sc.trace_photons(m, desc["disc_light"], target, 40 * target, caustic=caustic)
        m.balance()
        out.append((m, r["stored"], r["emitted"]))
    return out


def frame(W, maps, k, max_dist):
    g, c = maps[0][0], maps[1][0]
    n = W * W
    rays = torch.empty((n, 8), **f32)
    sc.gen_eye_rays(binding.make_camera(desc["eye"], desc["lookat"], desc["up"], desc["fov"]), W, W, rays)
    weights = pixels = None
    rgb = torch.zeros((W * W, 3), **f32)
    levels = []
    for level in range(a.depth + 1):
        hits = torch.empty((n, 4), **f32)
        sc.trace_device(rays, n, hits, binding.MR_TRACE_INCOHERENT if level else 0)
        scratch = torch.empty(12 * n, **f32)
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        call = lambda cnt=None: sc.gather_level(g, c, rays, hits, n, scratch, rgb, d_weights=weights, d_pixels=pixels, max_dist=max_dist,
                                                nphotons=k, d_counts=cnt)
        call(counts)                                            # warms up; the one counted call
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        q, seen = counts.tolist()
        levels.append(dict(level=level, rays=seen, queries=q, gather_ms=float(np.median(ts)), gather_ms_min=float(min(ts)), gather_ms_max=float(max(ts))))
        if level == a.depth:
            break
        o_rays, o_w = torch.empty((3 * n, 8), **f32), torch.empty((3 * n, 3), **f32)
        o_pix = torch.empty(3 * n, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        sc.gen_secondary_rays(rays, hits, weights, pixels, n, o_rays, o_w, o_pix, cnt)
        n = int(cnt.item())
        rays, weights, pixels = o_rays[:n].contiguous(), o_w[:n].contiguous(), o_pix[:n].contiguous()
    return dict(width=W, k=k, max_dist=max_dist, photons=[dict(caustic=i, stored=m[1], emitted=m[2]) for i, m in enumerate(maps)], levels=levels)


line = dict(tool="gather_level_probe", reps=a.reps, depth=a.depth, device=torch.cuda.get_device_name(0), frames=[])
line["frames"].append(frame(48, maps_of((6000, 2500)), 50, 0.35))
line["frames"].append(frame(a.width, maps_of((a.photons, a.photons)), a.k, a.max_dist))
txt = json.dumps(line)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(txt + "\n")
