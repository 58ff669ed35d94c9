"""Timing of mr_shade_lights against the batched shadow chain it replaces (mr_gen_shadow_rays -> mr_trace_indirect -> light
scale -> mr_shade_accumulate, once per light), on the primary hits of the sponza stand-in and of photon_room at 1920 x 1080 x
1 spp.  Both sides run in this one process, alternating, after a warm-up; device events around every repetition; median and
spread (min, max) reported.  1 and 4 point lights; and, on the same hits, one disc light next to one point light (the disc
light has no chain to compare against).  The outputs of both sides are compared at the timed size: with one light as uint32
(every pixel receives one addition), with four within the tolerance of two orders of the same atomics.
Prints one JSON line.
usage: python tools/lights_probe.py [--reps 20] [--width 1920 --height 1080] [--out profiles/lights_line.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))
import numpy as np, torch
import miro_amd
from miro_amd import binding, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--out", default="")
a = ap.parse_args()
W, H = a.width, a.height
n = W * H
f32 = dict(dtype=torch.float32, device="cuda")


def stats(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def one_scene(name):
    d = scenes.SCENES[name]
    sc = miro_amd.Scene(0)
    scenes.populate(sc, d)
    if "materials" in d:
        sc.set_materials(d["materials"], d["prim_material"])
    sc.build(4)
    rays, hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
    sc.gen_eye_rays(binding.make_camera(d["eye"], d["lookat"], d["up"], d["fov"]), W, H, rays)
    sc.trace_device(rays, n, hits)
    n_hits = int((hits[:, 1].view(torch.int32) != -1).sum())
    v = sc.arrays()[0]
    lo, hi = (v.min(axis=0), v.max(axis=0)) if len(v) else (np.array([-2.0, -0.5, -2.0]), np.array([2.0, 4.0, 2.0]))
    ext = hi - lo
    # four point lights inside the scene: the description's own, then three spread over the upper half of its box
    L0 = tuple(float(c) for c in d["light"])
    points = [dict(position=L0, color=(1.0, 1.0, 1.0), wattage=d["wattage"])]
    for fx, fy, fz in ((0.3, 0.7, 0.35), (0.7, 0.6, 0.65), (0.5, 0.8, 0.5)):
        points.append(dict(position=(float(lo[0] + fx * ext[0]), float(lo[1] + fy * ext[1]), float(lo[2] + fz * ext[2])),
                           color=(0.9, 0.8, 0.7), wattage=0.5 * d["wattage"]))
    disc = d.get("disc_light") or dict(position=(float(lo[0] + hi[0]) / 2, float(hi[1] - 0.05 * ext[1]), float(lo[2] + hi[2]) / 2),
                                       normal=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0), wattage=200.0, radius=0.1 * float(min(ext[0], ext[2])))
    sh_rays, sh_hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rgb_chain, rgb_one = torch.zeros((n, 3), **f32), torch.zeros((n, 3), **f32)

    def chain(lights):
        for lt in lights:
            sc.gen_shadow_rays(rays, hits, n, lt["position"], sh_rays, src, cnt)
            sc.trace_indirect(sh_rays, cnt, n, sh_hits, 0)
            sc.shade_accumulate(rays, hits, None, None, n, sh_rays, sh_hits, src, cnt, lt["position"], lt["wattage"], rgb_chain,
                                color=lt["color"])

    def single():
        sc.shade_lights(rays, hits, n, rgb_one)

    out = dict(rays=n, hits=n_hits, nodes=int(sc.info().n_nodes))
    for k in (1, 4):
        lights = points[:k]
        sc.set_lights(lights)
        for _ in range(3):                              # warm-up: code objects, the library's grow-only scratch
            chain(lights); single()
        rgb_chain.zero_(); rgb_one.zero_()
        chain(lights); single()
        torch.cuda.synchronize()
        if k == 1:
            same = bool(torch.equal(rgb_chain.view(torch.int32), rgb_one.view(torch.int32)))
        else:
            same = bool(torch.allclose(rgb_chain, rgb_one, rtol=1e-6, atol=1e-7 * float(rgb_chain.max())))
        tc, ts = [], []
        for _ in range(a.reps):                         # alternating
            tc.append(timed(lambda: chain(lights)))
            ts.append(timed(single))
        out["point_x%d" % k] = dict(outputs_equal=same, chain=stats(tc), shade_lights=stats(ts),
                                    speedup=float(np.median(tc) / np.median(ts)))
    # the disc light next to one point light, on the same hits
    td, tp = [], []
    for _ in range(a.reps + 3):
        sc.set_lights([disc])
        td.append(timed(single))
        sc.set_lights(points[:1])
        tp.append(timed(single))
    out["disc_x1"] = dict(light=disc, shade_lights=stats(td[3:]), point_shade_lights=stats(tp[3:]))
    return out


line = dict(tool="lights_probe", width=W, height=H, spp=1, reps=a.reps, device=torch.cuda.get_device_name(0), scenes={})
for name in ("sponza", "photon_room"):
    line["scenes"]["sponza-standin" if name == "sponza" and scenes.sponza_label() != "sponza" else name] = one_scene(name)
txt = json.dumps(line)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(txt + "\n")
