"""Frame time of FrameRenderer.render_specular(fused="frame_lights" | "frame_lights_path") -- level 0 ONE launch of
mr_render_level_lights (csrc/mr_frame_level_lights.hip: the fused frame that also writes the rays of level 1), the further levels
mr_trace_level_lights[_path] on its children -- against fused="lights" | "lights_path", where level 0 is a level launch too: pixel
slots zeroed, the resident eye rays read back, float atomics into the pixels.  1920 x 1080, depth 3, the frames of
tools/level_lights_probe.py and tools/level_lights_path_probe.py at 1 and 4 spp: the mixed room, the textured teapot under a seeded
2048 x 1024 image and the flower with drops (specular children), the flower with drops under its colour and under the image, the
stone room and the teapot (path tracing, path_seed 29).  The renderer of the frame route is built with resident_rays=False; its
resident bytes and the other renderer's are reported.  Every case runs in a child process of its own under a time limit of its own
(--case-seconds), one after the other, and the first case that does not end with status 0 ends the run: nothing more is started on
a device that may have faulted.  Inside a case: 3 warm frames of each route, then the routes alternate frame by frame, --frames
frames each; a frame lies between two device events on the current stream, and so does every level -- on both routes one step of
the driver, from the allocation of the level's counters and queue to the read-back of the counters, level 0 included; the level-route frame includes its zeroing of the pixel slots, not
generate(), which that route runs once per camera.  Before anything is timed the two frames are compared: per_level equal, pixels
within 2e-5 of the largest value (a pixel that holds a NaN must hold one in both; their number is reported).  One JSON line per case, printed and appended to --out.
usage: python tools/frame_level_lights_probe.py [--frames 20] [--out lines.json]   (profiles/frame_level_lights_ab.log: a header and these lines)"""
import argparse, json, math, os, signal, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

# scene, spp, route, path_kinds, environment ("own": the description's; "image": the seeded image)
CASES = {"mixed1": ("mixed", 1, "lights", 0, None), "teapot1": ("teapot_textured", 1, "lights", 0, "image"),
         "teapot4": ("teapot_textured", 4, "lights", 0, "image"), "flower1": ("flower_drops", 1, "lights", 0, "own"),
         "flower4": ("flower_drops", 4, "lights", 0, "own"),
         "path_flower1": ("flower_drops", 1, "lights_path", 7, "own"), "path_flower4": ("flower_drops", 4, "lights_path", 7, "own"),
         "path_flower1_image": ("flower_drops", 1, "lights_path", 7, "image"), "path_flower4_image": ("flower_drops", 4, "lights_path", 7, "image"),
         "path_stone1": ("stone", 1, "lights_path", 7, None), "path_stone4": ("stone", 4, "lights_path", 7, None),
         "path_teapot1": ("teapot_textured", 1, "lights_path", 3, "image")}
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
assert torch.cuda.is_available(), "the probe measures on the GPU"
W, H, DEPTH = 1920, 1080, 3
name, spp, LEVEL, KINDS, env_kind = CASES[a.case]
FRAME = "frame_" + LEVEL
IMAGE = dict(pixels=(np.random.default_rng(168).random((1024, 2048, 3)) * 4.0).astype(np.float32), rotation=(math.pi / 3 + 0.05, math.pi / 8))
INF, NONE = float("inf"), 0xFFFFFFFF
sc = miro_amd.Scene(0)
environment = None
if name in ("stone", "mixed"):
    d = scenes.textured_room_setup(sc, scenes.photon_room_stone() if name == "stone" else scenes.photon_room_mixed())
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
renderers = {LEVEL: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False),
             FRAME: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False, resident_rays=False)}
renderers[LEVEL].generate()
first = True
level_ms = []                                           # of the frame in flight: one entry per level


def timed(step):
    def run(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = step(*args, **kw)
        e1.record()
        level_ms.append((e0, e1))
        return out
    return run


# every level of either route is one step of the driver: the launch, the allocation of its counters and queue before it and the
# read-back of the counters after it.  Level 0 is _level_lights on the level route and _frame_level0 on the frame route, timed
# alike (as tools/level_lights_path_probe.py times its steps)
for fr in renderers.values():
    fr._level_lights, fr._frame_level0 = timed(fr._level_lights), timed(fr._frame_level0)
lean = renderers[FRAME]
kwargs = dict(path_tracing=True, path_kinds=KINDS, path_seed=29) if LEVEL == "lights_path" else {}


def one_frame(fused):
    """(frame ms, [level ms], per_level, bytes allocated on top of the resident ones at the frame's peak)"""
    global first
    fr = renderers[fused]
    signal.setitimer(signal.ITIMER_REAL, a.frame_seconds)
    try:
        del level_ms[:]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        per_level = fr.render_specular(depth=DEPTH, lights=lights, environment=(environment if first else True) if environment else None,
                                       fused=fused, **kwargs)
        e1.record()
        torch.cuda.synchronize()
        first = False
        return e0.elapsed_time(e1), [x.elapsed_time(y) for x, y in level_ms], per_level, torch.cuda.max_memory_allocated() - base
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(min(ts)), 4), max_ms=round(float(max(ts)), 4))


# ---- the same picture first
_, _, levels_f, _ = one_frame(FRAME)
_, _, levels_l, _ = one_frame(LEVEL)
rgb_l, rgb_f = renderers[LEVEL].d_rgb, lean.d_rgb
nan_l, nan_f = torch.isnan(rgb_l).any(dim=1), torch.isnan(rgb_f).any(dim=1)      # pixels that a path carried a NaN weight into
finite = ~(nan_l | nan_f)
top = float(rgb_l[finite].abs().max())
err = float((rgb_l[finite] - rgb_f[finite]).abs().max()) / top
equal = levels_l == levels_f and bool(torch.equal(nan_l, nan_f)) and err <= 2e-5
for _ in range(3):                                      # warm frames of each route
    for fused in (LEVEL, FRAME):
        one_frame(fused)
res = {LEVEL: [], FRAME: []}
for _ in range(a.frames):                               # alternating
    for fused in (LEVEL, FRAME):
        res[fused].append(one_frame(fused))
line = dict(tool="frame_level_lights_probe", case=a.case, scene=name, width=W, height=H, spp=spp, depth=DEPTH, lights=len(lights),
            route=FRAME, against=LEVEL, path_kinds=KINDS,
            environment="image 2048x1024" if environment and "pixels" in environment else "colour" if environment else "none",
            per_level=levels_l, frames=a.frames, device=torch.cuda.get_device_name(0), pictures_agree=equal, max_rel_diff=err,
            nan_pixels=[int(nan_l.sum()), int(nan_f.sum())])
for key, fused in (("level_route", LEVEL), ("frame_route", FRAME)):
    rs = res[fused]
    line[key] = dict(frame=stats([r[0] for r in rs]), levels=[stats([r[1][k] for r in rs]) for k in range(len(levels_l))],
                     peak_bytes_per_frame=int(max(r[3] for r in rs)), resident_bytes=int(renderers[fused].bytes_resident()))
line["speedup"] = round(line["level_route"]["frame"]["median_ms"] / line["frame_route"]["frame"]["median_ms"], 3)
line["level_speedup"] = [round(b["median_ms"] / f["median_ms"], 3) for b, f in zip(line["level_route"]["levels"], line["frame_route"]["levels"])]
txt = json.dumps(line)
print(txt, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt + "\n")
sys.exit(0 if equal else 3)
