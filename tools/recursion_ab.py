"""Frame time of FrameRenderer.render_specular(fused="device_lights" | "device_lights_path") -- ONE library call, mr_render_recursion
(include/miro_hip_recursion.h: level 0 as mr_render_level_lights, every further level one kernel of csrc/mr_level_lights_queued.hip
that reads the length of its queue from the device), then ONE read of the counters -- against fused="frame_lights" |
"frame_lights_path" on the same commit, where the same level 0 is followed by one mr_trace_level_lights[_path] per level, each
with its counters and queue allocated before it and its child count read back after it.  What is measured is what those host
round trips cost, and what the grid that is sized from an upper bound costs in return.

1920 x 1080, depth 3, 1 and 4 spp: the flower with drops under its colour, the mixed room, the textured teapot under a seeded
2048 x 1024 image (specular children), and the flower with drops path traced (path_kinds 7, path_seed 29): the frames of
tools/frame_level_lights_probe.py.  Both renderers are built with resident_rays=False; queue_capacity is the default, fan x samples.

Every case runs in a child process of its own under a time limit of its own (--case-seconds), one after the other, and the first
case that does not end with status 0 ends the run: nothing more is started on a device that may have faulted.  Inside a case the two
frames are compared first (per_level equal, pixels within 2e-5 of the largest value, the whole-frame bound of
tests/test_level_lights.py; a pixel that holds a NaN must hold one in both).  Then 3 warm frames of each route, then the routes
alternate frame by frame, --frames frames each.  A frame is timed by the host clock from the call of render_specular to its
return, after a device synchronise on either side: both routes end in a read-back, so the return is the end of the device's work,
and the host's share between the launches is what the comparison is about.  Then one mr_render_recursion with the same arguments
is captured into a graph on one stream and replayed --frames times: replay -> synchronise, and replay -> the read of the counters.
Per level: the workgroups the device route launches (its grid, from min(capacity, fan^level x samples)) against those that had
rays.  One JSON line per case, printed and appended to --out.
usage: python tools/recursion_ab.py [--frames 20] [--out lines.json]   (profiles/recursion_device_ab.log: a header and these lines)"""
import argparse, json, math, os, signal, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

# scene, spp, route of the levels, path_kinds, environment ("own": the description's; "image": the seeded image)
CASES = {"flower1": ("flower_drops", 1, "lights", 0, "own"), "flower4": ("flower_drops", 4, "lights", 0, "own"),
         "mixed1": ("mixed", 1, "lights", 0, None), "mixed4": ("mixed", 4, "lights", 0, None),
         "teapot1": ("teapot_textured", 1, "lights", 0, "image"), "teapot4": ("teapot_textured", 4, "lights", 0, "image"),
         "path_flower1": ("flower_drops", 1, "lights_path", 7, "own"), "path_flower4": ("flower_drops", 4, "lights_path", 7, "own")}
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
from miro_amd import binding, frame, scenes  # noqa: E402

signal.signal(signal.SIGALRM, signal.SIG_DFL)                      # the default action ends the process, also inside the runtime
assert torch.cuda.is_available(), "the tool measures on the GPU"
W, H, DEPTH = 1920, 1080, 3
name, spp, LEVEL, KINDS, env_kind = CASES[a.case]
FRAME, DEVICE = "frame_" + LEVEL, "device_" + LEVEL
PATH = LEVEL == "lights_path"
IMAGE = dict(pixels=(np.random.default_rng(168).random((1024, 2048, 3)) * 4.0).astype(np.float32), rotation=(math.pi / 3 + 0.05, math.pi / 8))
INF, NONE = float("inf"), 0xFFFFFFFF
sc = miro_amd.Scene(0)
environment = None
if name == "mixed":
    d = scenes.textured_room_setup(sc, scenes.photon_room_mixed())
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
renderers = {FRAME: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False, resident_rays=False),
             DEVICE: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False, resident_rays=False)}
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
_, levels_f = one_frame(FRAME)
_, levels_d = one_frame(DEVICE)
rgb_f, rgb_d = renderers[FRAME].d_rgb, renderers[DEVICE].d_rgb
nan_f, nan_d = torch.isnan(rgb_f).any(dim=1), torch.isnan(rgb_d).any(dim=1)      # pixels that a path carried a NaN weight into
finite = ~(nan_f | nan_d)
top = float(rgb_f[finite].abs().max())
err = float((rgb_f[finite] - rgb_d[finite]).abs().max()) / top
equal = levels_f == levels_d and bool(torch.equal(nan_f, nan_d)) and err <= 2e-5
for _ in range(3):                                      # warm frames of each route
    for fused in (FRAME, DEVICE):
        one_frame(fused)
res = {FRAME: [], DEVICE: []}
for _ in range(a.frames):                               # alternating
    for fused in (FRAME, DEVICE):
        res[fused].append(one_frame(fused)[0])

# ---- the device route's call alone, captured and replayed
dev = renderers[DEVICE]
fan = 4 if PATH else 3
cap = fan * dev.n
children = binding.MR_LEVEL_PATH if PATH else binding.MR_LEVEL_SPECULAR
need = sc.recursion_workspace_bytes(DEPTH, cap, children=children, environment=bool(environment), kinds=KINDS or 3)


def call(stream):
    sc.render_recursion(dev.cam, W, H, dev.d_rgb, dev.d_level_counts, DEPTH, d_workspace=dev.d_recursion, queue_capacity=cap, spp=spp,
                        jitter=dev.jitter, seed=dev.seed, stream=stream, children=children, environment=bool(environment),
                        kinds=KINDS or 3, path_seed=29, workspace_bytes=need)


signal.setitimer(signal.ITIMER_REAL, a.frame_seconds * 4)
torch.cuda.synchronize()
want = dev.d_level_counts[:DEPTH + 1].tolist()
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, stream=side):
    call(torch.cuda.current_stream())
replay_sync, replay_read = [], []
for k in range(3 + a.frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.replay()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    g.replay()
    got = dev.d_level_counts[:DEPTH + 1].tolist()
    t2 = time.perf_counter()
    equal = equal and got == want
    if k >= 3:
        replay_sync.append((t1 - t0) * 1e3)
        replay_read.append((t2 - t1) * 1e3)
signal.setitimer(signal.ITIMER_REAL, 0)

grids = []
bound = dev.n
for level in range(1, DEPTH + 1):
    bound = min(cap, bound * fan)
    launched = min(max((bound + 255) // 256, 1), 32768)
    grids.append(dict(level=level, launched=launched, with_rays=min((want[level][0] + 255) // 256, launched)))
line = dict(tool="recursion_ab", case=a.case, scene=name, width=W, height=H, spp=spp, depth=DEPTH, lights=len(lights), route=DEVICE,
            against=FRAME, path_kinds=KINDS,
            environment="image 2048x1024" if environment and "pixels" in environment else "colour" if environment else "none",
            per_level=levels_f, level_counts=want, frames=a.frames, device=torch.cuda.get_device_name(0), pictures_agree=equal,
            max_rel_diff=err, nan_pixels=[int(nan_f.sum()), int(nan_d.sum())], queue_capacity=cap, workspace_bytes=int(need),
            workgroups=grids,
            frame_route=dict(frame=stats(res[FRAME]), resident_bytes=int(renderers[FRAME].bytes_resident())),
            device_route=dict(frame=stats(res[DEVICE]), resident_bytes=int(dev.bytes_resident())),
            graph_replay=dict(to_synchronise=stats(replay_sync), to_counts_read=stats(replay_read)))
fm, dm = line["frame_route"]["frame"]["median_ms"], line["device_route"]["frame"]["median_ms"]
line["speedup"] = round(fm / dm, 3)
line["verdict"] = "faster" if dm < fm else "SLOWER"
line["replay_speedup"] = round(fm / line["graph_replay"]["to_counts_read"]["median_ms"], 3)
txt = json.dumps(line)
print(txt, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt + "\n")
sys.exit(0 if equal else 3)
