"""Frame time of FrameRenderer.render_specular(fused="device_lights") -- ONE mr_render_recursion, whose specular levels on a scene with a
reflective STONE material are the BUMPED kernels of csrc/mr_level_lights_queued_bump.hip -- against fused=False on the same commit:
the batched chain per level, trace -> hit_surface -> shade_lights_surface -> gen_secondary_rays_surface (csrc/mr_bump_surface.hip).
Not a speed feature: the numbers say what the route costs on the new scene, and that a scene without the flag runs what it ran.

1920 x 1080, depth 3, 1 and 4 spp, two lights: scenes.photon_room_polished() (bumped_specular: the new kernels) and
scenes.photon_room_stone() (diffuse stone only: the kernels of the parent commit on both routes; compare with that commit's line).

Every case runs in a child process of its own under a time limit of its own (--case-seconds), one after the other, and the first
case that does not end with status 0 ends the run: nothing more is started on a device that may have faulted.  Inside a case the two
frames are compared first (per_level equal, pixels within 2e-5 of the largest value, the whole-frame bound of tools/recursion_ab.py).
Then 3 warm frames of each route, then the routes alternate frame by frame, --frames frames each.  A frame is timed by the host
clock from the call of render_specular to its return, after a device synchronise on either side: both routes end in a read-back.
One JSON line per case, printed and appended to --out.
usage: python tools/bump_specular_ab.py [--frames 20] [--out lines.json]   (profiles/bump_specular_ab.log: a header and these lines)"""
import argparse, json, os, signal, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

CASES = {"polished1": ("polished", 1), "polished4": ("polished", 4), "stone1": ("stone", 1), "stone4": ("stone", 4)}
ORDER = tuple(CASES)
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--frame-seconds", type=float, default=30.0)
ap.add_argument("--case-seconds", type=float, default=120.0)
ap.add_argument("--case", default="", choices=[""] + sorted(CASES))
ap.add_argument("--only", default="", help="comma-separated cases for the driver (default: all)")
ap.add_argument("--out", default="")
a = ap.parse_args()

if not a.case:                                          # the driver: one child per case, none after the first that fails
    for name in (a.only.split(",") if a.only else ORDER):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--frames", str(a.frames),
               "--frame-seconds", str(a.frame_seconds)] + (["--out", a.out] if a.out else [])
        try:
            rc = subprocess.run(cmd, timeout=a.case_seconds).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("case %s ended with status %d: stopping" % (name, rc), flush=True)
            sys.exit(rc if 0 < rc < 256 else 1)
    sys.exit(0)

import numpy as np, torch  # noqa: E402
import miro_amd  # noqa: E402
from miro_amd import frame, scenes  # noqa: E402

signal.signal(signal.SIGALRM, signal.SIG_DFL)                      # the default action ends the process, also inside the runtime
assert torch.cuda.is_available(), "the tool measures on the GPU"
W, H, DEPTH = 1920, 1080, 3
name, spp = CASES[a.case]
BATCHED, DEVICE = False, "device_lights"
sc = miro_amd.Scene(0)
d = scenes.textured_room_setup(sc, scenes.photon_room_polished() if name == "polished" else scenes.photon_room_stone())
lights = scenes.SCENES["photon_room_two_lights"]["lights"]
bumped = getattr(sc, "bumped_specular", False) is True          # (a commit before the feature has no such property: stone cases only)
assert bumped is (name == "polished")
renderers = {BATCHED: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False),
             DEVICE: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False, resident_rays=False)}
renderers[BATCHED].generate()                           # the batched route reads the resident eye rays; they do not change


def one_frame(fused):
    """(frame ms by the host clock, per_level)"""
    fr = renderers[fused]
    signal.setitimer(signal.ITIMER_REAL, a.frame_seconds)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_level = fr.render_specular(depth=DEPTH, lights=lights, fused=fused)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, per_level
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(min(ts)), 4), max_ms=round(float(max(ts)), 4))


# ---- the same picture first
_, levels_b = one_frame(BATCHED)
_, levels_d = one_frame(DEVICE)
rgb_b, rgb_d = renderers[BATCHED].d_rgb, renderers[DEVICE].d_rgb
top = float(rgb_b.abs().max())
err = float((rgb_b - rgb_d).abs().max()) / top
equal = levels_b == levels_d and err <= 2e-5
for _ in range(3):                                      # warm frames of each route
    for fused in (BATCHED, DEVICE):
        one_frame(fused)
res = {BATCHED: [], DEVICE: []}
for _ in range(a.frames):                               # alternating
    for fused in (BATCHED, DEVICE):
        res[fused].append(one_frame(fused)[0])

line = dict(tool="bump_specular_ab", case=a.case, scene="photon_room_" + name, bumped_specular=bumped, width=W, height=H,
            spp=spp, depth=DEPTH, lights=len(lights), route=DEVICE, against="batched (fused=False)", per_level=levels_b, frames=a.frames,
            device=torch.cuda.get_device_name(0), pictures_agree=equal, max_rel_diff=err,
            batched_route=dict(frame=stats(res[BATCHED])), device_route=dict(frame=stats(res[DEVICE])))
bm, dm = line["batched_route"]["frame"]["median_ms"], line["device_route"]["frame"]["median_ms"]
line["speedup"] = round(bm / dm, 3)
line["verdict"] = "faster" if dm < bm else "SLOWER"
txt = json.dumps(line)
print(txt, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt + "\n")
sys.exit(0 if equal else 3)
