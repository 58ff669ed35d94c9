"""Wall time from the start of a photon trace to a map that can answer estimates, host path against resident path, at a
target of 200 000 photons: the room (global and caustic map) and the stone room (global, the surface walk).
  host      mr_trace_photons (or _surface) + mr_photon_map_balance: the three parts of mr_trace_photons_timing and the
            balance call (tree, re-pack, block boxes, upload) separately
  resident  mr_trace_photons_resident, one call: the device rounds and store_ms / balance_ms / pack_ms / deferred of the build
One process; the two paths alternate, median of --reps runs after one warm-up of each; every GPU step runs under a time limit
of its own (the process is ended if a step exceeds --step-seconds).  One JSON line per row, printed and written to --out.
usage: python tools/photon_build_probe.py [--target 200000] [--reps 5] [--out profiles/photon_build_line.json]"""
import argparse, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))
import numpy as np, torch
import miro_amd
from miro_amd import scenes

ap = argparse.ArgumentParser()
ap.add_argument("--target", type=int, default=200000)
ap.add_argument("--max-emissions", type=int, default=4000000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-seconds", type=float, default=30.0)
ap.add_argument("--out", default="")
a = ap.parse_args()


signal.signal(signal.SIGALRM, signal.SIG_DFL)                      # the default action ends the process, also inside the runtime


def limited(step):
    """run one GPU step; a step that takes longer than --step-seconds ends the process"""
    signal.setitimer(signal.ITIMER_REAL, a.step_seconds)
    try:
        return step()
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def host_path(sc, light, caustic, surface):
    m = miro_amd.PhotonMap(a.target + 64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = sc.trace_photons(m, light, a.target, a.max_emissions, caustic=caustic, surface=surface)
    t1 = time.perf_counter()
    m.balance()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return dict(wall_ms=(t2 - t0) * 1e3, kernel_ms=r["kernel_ms"], readback_ms=r["readback_ms"], store_ms=r["store_ms"], balance_ms=(t2 - t1) * 1e3,
                emitted=r["emitted"], stored=r["stored"], rounds=r["rounds"])


def resident_path(sc, light, caustic, surface):
    m = miro_amd.PhotonMap(a.target + 64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = sc.trace_photons(m, light, a.target, a.max_emissions, caustic=caustic, surface=surface, resident=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    b = r["build"]
    return dict(wall_ms=(t1 - t0) * 1e3, kernel_ms=r["kernel_ms"], store_ms=b["store_ms"], balance_ms=b["balance_ms"], pack_ms=b["pack_ms"],
                deferred=b["deferred"], emitted=r["emitted"], stored=r["stored"], rounds=r["rounds"])


def median_of(runs):
    return {k: (float(np.median([r[k] for r in runs])) if k.endswith("_ms") else runs[-1][k]) for k in runs[0]}


def row(name, sc, light, caustic, surface):
    host, res = [], []
    for rep in range(a.reps + 1):                                   # the first pair warms up (code objects, allocator)
        h = limited(lambda: host_path(sc, light, caustic, surface))
        r = limited(lambda: resident_path(sc, light, caustic, surface))
        if rep:
            host.append(h); res.append(r)
    h, r = median_of(host), median_of(res)
    assert (h["emitted"], h["stored"]) == (r["emitted"], r["stored"])
    return dict(tool="photon_build_probe", row=name, target=a.target, reps=a.reps, device=torch.cuda.get_device_name(0), caustic=int(caustic),
                surface=int(surface), host=h, resident=r, speedup=h["wall_ms"] / r["wall_ms"],
                host_wall_ms_runs=[round(x["wall_ms"], 3) for x in host], resident_wall_ms_runs=[round(x["wall_ms"], 3) for x in res],
                resident_kernel_ms_runs=[round(x["kernel_ms"], 3) for x in res])


def room():
    d = scenes.SCENES["photon_room"]
    sc = miro_amd.Scene(0)
    scenes.populate(sc, d)
    sc.set_materials(d["materials"], d["prim_material"])
    sc.build(4)
    return sc, d["disc_light"]


def stone():
    d = scenes.photon_room_stone()
    sc = miro_amd.Scene(0)
    scenes.textured_room_setup(sc, d)
    return sc, d["disc_light"]


lines = []
sc, light = room()
lines.append(row("photon_room global", sc, light, False, False))
lines.append(row("photon_room caustic", sc, light, True, False))
sc, light = stone()
lines.append(row("photon_room_stone global (surface walk)", sc, light, False, True))
txt = "\n".join(json.dumps(l) for l in lines)
print(txt)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(txt + "\n")
