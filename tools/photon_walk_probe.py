"""Timing of mr_trace_photons: target = 200 000 global + 200 000 caustic photons (Scene.h:67-68) on the sponza stand-in
(a closed atrium, disc light just under its ceiling facing down; white Lambert everywhere, so its caustic pass stores
nothing and stops at --max-emissions) and on the room scene of miro_amd.scenes.  Prints one JSON line: wall time of the
call split into kernel time, read-back and host store; emitted, stored, segments; segments per second of the device rounds;
and, as the yardstick, the rate at which mr_trace(MR_TRACE_INCOHERENT | MR_RAYS_ON_DEVICE | MR_HITS_ON_DEVICE) traces the
diffuse-continuation segments between consecutive stored hits of one emission, rebuilt from d_records with the walk's own
arithmetic (the light's first, coherent segments and the specular ones cannot be rebuilt from the records and are left out).
usage: python tools/photon_walk_probe.py [--target 200000] [--reps 5] [--out profiles/photon_walk_line.json]

--surface: mr_trace_photons_surface instead.  The room geometry plain through both entry points, then the mixed room and the
stone room of miro_amd.scenes through the new one (global and caustic each); the yardstick becomes what the same continuation
segments cost as separate launches, mr_trace and then mr_hit_surface on its hits (yardstick_ms, yardstick_surface_ms).
usage: python tools/photon_walk_probe.py --surface [--out profiles/photon_walk_surface_line.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))
import numpy as np, torch
import miro_amd
from miro_amd import binding, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--target", type=int, default=200000)
ap.add_argument("--max-emissions", type=int, default=4000000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--surface", action="store_true")
a = ap.parse_args()


def build(name):
    d = scenes.SCENES[name]
    sc = miro_amd.Scene(0)
    scenes.populate(sc, d)
    if "materials" in d:
        sc.set_materials(d["materials"], d["prim_material"])
    sc.build(4)
    if "disc_light" in d:
        return sc, d["disc_light"]
    v = sc.arrays()[0]
    lo, hi = v.min(axis=0), v.max(axis=0)
    top = float(hi[1]) - 0.05 * float(hi[1] - lo[1])
    return sc, dict(position=(float(lo[0] + hi[0]) / 2, top, float(lo[2] + hi[2]) / 2), normal=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0),
                    wattage=200.0, radius=0.1 * float(min(hi[0] - lo[0], hi[2] - lo[2])))


def one(sc, light, caustic, surface=False):
    cap = 2 * a.target + 64
    d_rec = torch.zeros((cap, 12), dtype=torch.float32, device="cuda")
    runs = []
    for rep in range(a.reps + 1):                                   # the first run warms up (code objects, allocator)
        m = miro_amd.PhotonMap(cap)
        t0 = time.perf_counter()
        r = sc.trace_photons(m, light, a.target, a.max_emissions, caustic=caustic, d_records=d_rec, records_capacity=cap, surface=surface)
        r["wall_ms"] = (time.perf_counter() - t0) * 1e3
        if rep:
            runs.append(r)
    med = {k: float(np.median([r[k] for r in runs])) for k in ("wall_ms", "kernel_ms", "readback_ms", "store_ms")}
    r = runs[-1]
    out = dict(caustic=int(caustic), emitted=r["emitted"], stored=r["stored"], segments=r["segments"], rounds=r["rounds"], **med)
    out["walk_Msegments_per_s"] = r["segments"] / med["kernel_ms"] / 1e3
    # yardstick: the continuation segments between consecutive stored hits of one emission, traced by mr_trace
    n = min(int(r["stored"]), cap)
    rec = d_rec[:n]
    em, dep = rec[:, 9].view(torch.int32), rec[:, 10].view(torch.int32)
    pair = (em[1:] == em[:-1]) & (dep[1:] == dep[:-1] + 1) if n > 1 else torch.zeros(0, dtype=torch.bool, device="cuda")
    k = int(pair.sum())
    out["yardstick_segments"] = k
    if k >= 1024:
        P, d = rec[:-1][pair][:, 0:3], rec[1:][pair][:, 3:6]
        eps = torch.tensor(1e-4, dtype=torch.float32, device="cuda")
        rays = torch.zeros((k, 8), dtype=torch.float32, device="cuda")
        rays[:, 0:3] = (P + d * eps) + eps * d
        rays[:, 4:7] = d
        rays[:, 7] = 1e12
        hits = torch.empty((k, 4), dtype=torch.float32, device="cuda")
        fl = binding.MR_TRACE_INCOHERENT
        sc.trace_device(rays, k, hits, fl)
        torch.cuda.synchronize()
        end = rec[1:][pair][:, 0:3]
        t = hits[:, 0:1]
        out["yardstick_same_hit_fraction"] = float((((rays[:, 0:3] + t * d) - end).abs().max(dim=1).values < 1e-3).float().mean())
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); sc.trace_device(rays, k, hits, fl); e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        out["yardstick_ms"] = float(np.median(ts))
        out["yardstick_Msegments_per_s"] = k / out["yardstick_ms"] / 1e3
        if surface:                                                  # ... and the surface pass over those hits, a launch of its own
            color, normal = torch.empty((k, 3), dtype=torch.float32, device="cuda"), torch.empty((k, 3), dtype=torch.float32, device="cuda")
            ts = []
            for _ in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); sc.hit_surface(rays, hits, k, color, normal); e1.record(); torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            out["yardstick_surface_ms"] = float(np.median(ts[1:]))
    return out


line = dict(tool="photon_walk_probe", target=a.target, reps=a.reps, device=torch.cuda.get_device_name(0), scenes={})
if a.surface:
    line["surface"] = 1
    sc, light = build("photon_room")
    line["scenes"]["photon_room (mr_trace_photons)"] = dict(light=light, runs=[one(sc, light, False), one(sc, light, True)])
    line["scenes"]["photon_room"] = dict(light=light, runs=[one(sc, light, False, True), one(sc, light, True, True)])
    for name, desc in (("photon_room_mixed", scenes.photon_room_mixed()), ("photon_room_stone", scenes.photon_room_stone())):
        sc = miro_amd.Scene(0)
        scenes.textured_room_setup(sc, desc)
        light = desc["disc_light"]
        line["scenes"][name] = dict(light=light, runs=[one(sc, light, False, True), one(sc, light, True, True)])
else:
    for name in ("sponza", "photon_room"):
        sc, light = build(name)
        line["scenes"][name] = dict(light=light, runs=[one(sc, light, False), one(sc, light, True)])
txt = json.dumps(line)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(txt + "\n")
