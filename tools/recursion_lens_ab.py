"""Frame time of FrameRenderer.render_specular(fused="device_lens" | "device_lens_path") -- ONE library call, mr_render_recursion_lens
(include/miro_hip_lens.h: level 0 as mr_render_level_lights_lens, whose thin-lens eye rays are made in registers, every further
level one kernel of csrc/mr_level_lights_queued.hip), then ONE read of the counters -- on the same commit against

  batched   FrameRenderer(lens=...): generate() (mr_gen_eye_rays_lens, 32 bytes per sample) + render_specular(fused="lights" |
            "lights_path"), one mr_trace_level_lights[_path] per level, level 0 included: the best lens route before this call;
  pinhole   fused="device_lights" | "device_lights_path" of a renderer without a lens: what the lens prologue itself costs.

1920 x 1080, depth 3, at 1, 4 and 64 spp: the flower with drops under its colour with the flower scene's own lens (DOF_APERTURE
0.20, DOF_FOCUS_PLANE 15.3, Miro.h:18-19), the mixed room and the textured teapot under a seeded 2048 x 1024 image with aperture
0.20 focused at the camera's look-at point (specular children), and the flower with drops path traced (path_kinds 7, path_seed
29): the scenes of tools/recursion_ab.py.  The device renderers are built with resident_rays=False; queue_capacity is the default.

Every case runs in a child process of its own under a time limit of its own (--case-seconds), one after the other, and the first
case that does not end with status 0 ends the run: nothing more is started on a device that may have faulted.  Inside a case the
lens frames are compared first (per_level equal, pixels within 2e-5 of the largest value; a pixel that holds a NaN must hold one
in both).  Then 3 warm frames of each route, then the three routes alternate frame by frame, --frames frames each.  A frame is timed
by the host clock from the call to its return, after a device synchronise on either side.  resident_bytes is bytes_resident() of
each renderer after its frames (the batched route's per-level queues are transient and not in it).  One JSON line per case,
printed and appended to --out.
usage: python tools/recursion_lens_ab.py [--frames 20] [--only a,b] [--out lines.json]   (profiles/recursion_lens_ab.log)"""
import argparse, json, math, os, signal, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

# scene, spp, route of the levels, path_kinds
CASES = {}
for _spp in (1, 4, 64):
    CASES["flower%d" % _spp] = ("flower_drops", _spp, "lights", 0)
    CASES["mixed%d" % _spp] = ("mixed", _spp, "lights", 0)
    CASES["teapot%d" % _spp] = ("teapot_textured", _spp, "lights", 0)
    CASES["path_flower%d" % _spp] = ("flower_drops", _spp, "lights_path", 7)
ORDER = tuple(CASES)
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--frame-seconds", type=float, default=60.0)
ap.add_argument("--case-seconds", type=float, default=240.0)
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
name, spp, LEVEL, KINDS = CASES[a.case]
PATH = LEVEL == "lights_path"
BATCHED, LENS, PINHOLE = LEVEL, "device_lens" + LEVEL[6:], "device_" + LEVEL
IMAGE = dict(pixels=(np.random.default_rng(168).random((1024, 2048, 3)) * 4.0).astype(np.float32), rotation=(math.pi / 3 + 0.05, math.pi / 8))
INF, NONE = float("inf"), 0xFFFFFFFF
sc = miro_amd.Scene(0)
environment = None
if name == "mixed":
    d = scenes.textured_room_setup(sc, scenes.photon_room_mixed())
    lights = scenes.SCENES["photon_room_two_lights"]["lights"]
elif name == "flower_drops":
    d = scenes.flower_setup(sc, scenes.flower_scene(drops=True))
    lights, environment = d["lights"], d["environment"]
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
if name == "flower_drops":
    lens = dict(aperture=0.20, focus_plane=15.3)        # Miro.h:18-19
else:
    lens = dict(aperture=0.20, focus_plane=float(np.linalg.norm(np.subtract(d["lookat"], d["eye"]))))
renderers = {BATCHED: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False, lens=lens),
             LENS: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False, lens=lens, resident_rays=False),
             PINHOLE: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False, resident_rays=False)}
first = True
kwargs = dict(path_tracing=True, path_kinds=KINDS, path_seed=29) if PATH else {}


def one_frame(fused):
    """(frame ms by the host clock, per_level)"""
    global first
    fr = renderers[fused]
    signal.setitimer(signal.ITIMER_REAL, a.frame_seconds)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if fused == BATCHED:
            fr.generate()
        per_level = fr.render_specular(depth=DEPTH, lights=lights, environment=(environment if first else True) if environment else None,
                                       fused=fused, **kwargs)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        first = False
        return (t1 - t0) * 1e3, per_level
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(min(ts)), 4), max_ms=round(float(max(ts)), 4))


# ---- the same picture first
_, levels_b = one_frame(BATCHED)
_, levels_l = one_frame(LENS)
rgb_b, rgb_l = renderers[BATCHED].d_rgb, renderers[LENS].d_rgb
nan_b, nan_l = torch.isnan(rgb_b).any(dim=1), torch.isnan(rgb_l).any(dim=1)
finite = ~(nan_b | nan_l)
top = float(rgb_b[finite].abs().max())
err = float((rgb_b[finite] - rgb_l[finite]).abs().max()) / top
equal = levels_b == levels_l and bool(torch.equal(nan_b, nan_l)) and err <= 2e-5
ROUTES = (BATCHED, LENS, PINHOLE)
for _ in range(3):                                      # warm frames of each route
    for fused in ROUTES:
        one_frame(fused)
res = {r: [] for r in ROUTES}
for _ in range(a.frames):                               # alternating
    for fused in ROUTES:
        res[fused].append(one_frame(fused)[0])

line = dict(tool="recursion_lens_ab", case=a.case, scene=name, width=W, height=H, spp=spp, depth=DEPTH, lights=len(lights), lens=lens,
            route=LENS, against=[BATCHED, PINHOLE], path_kinds=KINDS,
            environment="image 2048x1024" if environment and "pixels" in environment else "colour" if environment else "none",
            per_level=levels_l, frames=a.frames, device=torch.cuda.get_device_name(0), pictures_agree=equal, max_rel_diff=err,
            nan_pixels=[int(nan_b.sum()), int(nan_l.sum())])
for key, r in (("batched_lens_route", BATCHED), ("device_lens_route", LENS), ("device_pinhole_route", PINHOLE)):
    line[key] = dict(frame=stats(res[r]), resident_bytes=int(renderers[r].bytes_resident()))
bm, lm, pm = (line[k]["frame"]["median_ms"] for k in ("batched_lens_route", "device_lens_route", "device_pinhole_route"))
line["speedup_over_batched"] = round(bm / lm, 3)
line["verdict"] = "faster" if lm < bm else "SLOWER"
line["lens_over_pinhole"] = round(lm / pm, 3)
txt = json.dumps(line)
print(txt, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt + "\n")
sys.exit(0 if equal else 3)
