"""Frame time of FrameRenderer.render_specular(fused="lights_path", path_tracing=True) -- every level of a PATH_TRACING build's
recursion ONE launch of mr_trace_level_lights_path (csrc/mr_level_lights_path.hip) -- against the batched route with the same
children (fused=False, surface_children=True: per level mr_trace -> mr_shade_environment -> mr_hit_surface ->
mr_shade_lights_surface -> mr_gen_path_rays_surface), at 1920 x 1080, depth 3, the same path_seed.  Cases: flower_scene(drops=True)
with kinds = MIRROR | REFRACT | DIFFUSE under its background colour at 1 and 4 spp (both routes), and under a seeded 2048 x 1024
environment image at 1 and 4 spp -- FUSED ONLY: the batched driver refuses mixed kinds under an image, its queues do not record
which child came from Ray::random; the stone room (closed; bump-mapped floor and walls, glass and mirror spheres, two lights) with
all three kinds at 1 spp; the textured teapot (open; four lights) under the image with the specular kinds at 1 spp.  Every case
runs in a child process of its own under a time limit of its own (--case-seconds), one after the other, and the first case that
does not end with status 0 ends the run: nothing more is started on a device that may have faulted.  Inside a case: 3 warm frames
of each route (they upload the texture table and the image), then the routes alternate frame by frame, --frames frames each; a
frame lies between two device events on the current stream, and so does every level (the driver reads the level's counters back
before the next level, in both routes).  Median and spread (min, max) per route and per level; the peak of the bytes the route
allocates during a frame on top of what is resident before it.  Before anything is timed the two frames are compared: per_level
equal, pixels within 2e-5 of the largest value.  One JSON line per case, printed and appended to --out.
usage: python tools/level_lights_path_probe.py [--frames 20] [--out profiles/level_lights_path_line.json]"""
import argparse, json, math, os, signal, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

# scene, spp, path_kinds, environment ("own": the description's; "image": the seeded image), does the batched route serve it
CASES = {"flower1": ("flower_drops", 1, 7, "own", True), "flower4": ("flower_drops", 4, 7, "own", True),
         "flower1_image": ("flower_drops", 1, 7, "image", False), "flower4_image": ("flower_drops", 4, 7, "image", False),
         "stone1": ("stone", 1, 7, None, True), "teapot1": ("teapot_textured", 1, 3, "image", True)}
ORDER = ("flower1", "flower4", "flower1_image", "flower4_image", "stone1", "teapot1")
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--frame-seconds", type=float, default=30.0)
ap.add_argument("--case-seconds", type=float, default=200.0)
ap.add_argument("--case", default="", choices=[""] + sorted(CASES))
ap.add_argument("--out", default="")
a = ap.parse_args()

if not a.case:                                          # the driver: one child per case, none after the first that fails
    for name in ORDER:
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
assert torch.cuda.is_available(), "the probe measures on the GPU"
W, H, DEPTH = 1920, 1080, 3
name, spp, KINDS, env_kind, AB = CASES[a.case]
IMAGE = dict(pixels=(np.random.default_rng(168).random((1024, 2048, 3)) * 4.0).astype(np.float32), rotation=(math.pi / 3 + 0.05, math.pi / 8))
INF, NONE = float("inf"), 0xFFFFFFFF
sc = miro_amd.Scene(0)
environment = None
if name == "stone":
    d = scenes.textured_room_setup(sc, scenes.photon_room_stone())
    lights = scenes.SCENES["photon_room_two_lights"]["lights"]
elif name == "flower_drops":
    d = scenes.flower_setup(sc, scenes.flower_scene(drops=True))
    lights, environment = d["lights"], d["environment"] if env_kind == "own" else IMAGE
else:                                                   # the teapot of tests/test_frame_lights_surface.py: a glossy leaf on a checker floor
    d = scenes.SCENES["teapot"]
    scenes.populate(sc, d)
    sc.build(4)
    nt = sc.info().n_triangles
    tidx = np.full((nt, 3), NONE, np.uint32)
    tidx[nt - 1] = (0, 1, 2)
    sc.set_texcoords(np.array([[0, 0], [4, 8], [8, 0]], np.float32), tidx)
    white, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    sc.set_materials([(white, (0.2, 0.2, 0.2), zero, 40.0, 1.0), (white, zero, zero, INF, 1.0)], [0] * (nt - 1) + [1])
    sc.set_textures([dict(leaf=2.0), dict(color1=(0.9, 0.8, 0.7), color2=(0.2, 0.3, 0.5), scale=1.0)], [0, 1])
    lights = [dict(position=(-2.0, 3.0, 6.0), wattage=30.0), dict(position=(2.0, 4.5, 6.5), wattage=30.0),
              dict(position=(0.0, 20.0, 0.0), wattage=1000.0), dict(position=(0.0, 5.0, 7.0), wattage=30.0)]
    environment = IMAGE
fr = frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False)
fr.generate()
first = True
level_ms = []                                           # of the frame in flight: one entry per level


def timed(step):
    def run(plan, q, level, last):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = step(plan, q, level, last)
        e1.record()
        level_ms.append((e0, e1))
        return out
    return run


fr._level_lights, fr._level_batched = timed(fr._level_lights), timed(fr._level_batched)
FUSED = "lights_path"


def one_frame(fused):
    """(frame ms, [level ms], per_level, bytes allocated on top of the resident ones at the frame's peak)"""
    global first
    signal.setitimer(signal.ITIMER_REAL, a.frame_seconds)
    try:
        del level_ms[:]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        per_level = fr.render_specular(depth=DEPTH, lights=lights, environment=(environment if first else True) if environment else None,
                                       fused=fused, path_tracing=True, path_kinds=KINDS, path_seed=29,
                                       surface_children=None if fused else True)
        e1.record()
        torch.cuda.synchronize()
        first = False
        return e0.elapsed_time(e1), [x.elapsed_time(y) for x, y in level_ms], per_level, torch.cuda.max_memory_allocated() - base
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(min(ts)), 4), max_ms=round(float(max(ts)), 4))


# ---- the same picture first
routes = (False, FUSED) if AB else (FUSED,)
_, _, levels_f, _ = one_frame(FUSED)
levels_b, err, equal = levels_f, None, True
if AB:
    rgb_f = fr.d_rgb.clone()
    _, _, levels_b, _ = one_frame(False)
    top = float(fr.d_rgb.abs().max())
    err = float((fr.d_rgb - rgb_f).abs().max()) / top
    equal = levels_b == levels_f and err <= 2e-5
    del rgb_f
for _ in range(3):                                      # warm frames of each route
    for fused in routes:
        one_frame(fused)
res = {False: [], FUSED: []}
for _ in range(a.frames):                               # alternating
    for fused in routes:
        res[fused].append(one_frame(fused))
line = dict(tool="level_lights_path_probe", case=a.case, scene=name, width=W, height=H, spp=spp, depth=DEPTH, lights=len(lights), path_kinds=KINDS,
            environment="image 2048x1024" if environment and "pixels" in environment else "colour" if environment else "none",
            per_level=levels_b, frames=a.frames, device=torch.cuda.get_device_name(0), pictures_agree=equal, max_rel_diff=err)
for key, fused in (("batched", False), ("fused", FUSED)):
    rs = res[fused]
    if not rs:
        line[key] = None                                # no batched counterpart: not measured
        continue
    line[key] = dict(frame=stats([r[0] for r in rs]), levels=[stats([r[1][k] for r in rs]) for k in range(len(levels_b))],
                     peak_bytes_per_frame=int(max(r[3] for r in rs)))
if AB:
    line["speedup"] = round(line["batched"]["frame"]["median_ms"] / line["fused"]["frame"]["median_ms"], 3)
    line["level_speedup"] = [round(b["median_ms"] / f["median_ms"], 3) for b, f in zip(line["batched"]["levels"], line["fused"]["levels"])]
txt = json.dumps(line)
print(txt, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt + "\n")
sys.exit(0 if equal else 3)
