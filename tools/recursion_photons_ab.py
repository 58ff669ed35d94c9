"""Frame time of FrameRenderer.render_specular(fused="device_photons" | "device_photons_path", photon_maps=(g, c)) -- ONE library call,
mr_render_recursion_photons (include/miro_hip_recursion_photons.h: mr_render_recursion's launches, and after every level the query,
estimate and accumulate kernels of csrc/mr_gather_queued.hip, which read the length of the level's queue from the device), then ONE
read of the counters -- against fused="frame_lights" | "frame_lights_path" with the same maps on the same commit, where level 0 is
followed by generate() and mr_gather_level, and every further level is mr_trace_level_lights[_path] + mr_gather_level with its
buffers allocated before it and its child count read back after it.  The sibling of tools/recursion_ab.py, which measures the same
pair without maps.

1920 x 1080, depth 3, 1 and 4 spp: the flower with drops under its colour and the mixed room (specular children), and the flower
with drops path traced (path_kinds 7, path_seed 29).  Maps: Scene.photon_maps from the scene's disc light, --photons each,
nphotons = --k, max_dist = 1e10.  The frame route needs resident rays (its level 0 gathers on generate()'s buffer); the device
route is built with resident_rays=False.  queue_capacity is the default, fan x samples.

Every case runs in a child process of its own under a time limit of its own (--case-seconds), one after the other, and the first
case that does not end with status 0 ends the run: nothing more is started on a device that may have faulted.  Inside a case the two
frames are compared first (per_level equal, pixels within 2e-5 of the largest value; a pixel that holds a NaN must hold one in
both).  Then 3 warm frames of each route, then the routes alternate frame by frame, --frames frames each.  A frame is timed by the
host clock from the call of render_specular to its return, after a device synchronise on either side.  Then one
mr_render_recursion_photons with the same arguments is captured into a graph on one stream and replayed --frames times, to the
read of the counters.  One JSON line per case, printed and appended to --out.
usage: python tools/recursion_photons_ab.py [--frames 20] [--out lines.json]   (profiles/recursion_photons_ab.log: a header and these lines)"""
import argparse, json, os, signal, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

# scene, spp, route of the levels, path_kinds
CASES = {"flower1": ("flower_drops", 1, "lights", 0), "flower4": ("flower_drops", 4, "lights", 0),
         "mixed1": ("mixed", 1, "lights", 0), "mixed4": ("mixed", 4, "lights", 0),
         "path_flower1": ("flower_drops", 1, "lights_path", 7), "path_flower4": ("flower_drops", 4, "lights_path", 7)}
ORDER = tuple(CASES)
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--photons", type=int, default=20000)
ap.add_argument("--k", type=int, default=50)
ap.add_argument("--frame-seconds", type=float, default=60.0)
ap.add_argument("--case-seconds", type=float, default=180.0)
ap.add_argument("--case", default="", choices=[""] + sorted(CASES))
ap.add_argument("--only", default="", help="comma-separated cases for the driver (default: all)")
ap.add_argument("--out", default="")
a = ap.parse_args()

if not a.case:                                          # the driver: one child per case, none after the first that fails
    for name in (a.only.split(",") if a.only else ORDER):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--frames", str(a.frames), "--photons", str(a.photons),
               "--k", str(a.k), "--frame-seconds", str(a.frame_seconds)] + (["--out", a.out] if a.out else [])
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
W, H, DEPTH, MAX_DIST = 1920, 1080, 3, 1e10
name, spp, LEVEL, KINDS = CASES[a.case]
FRAME, DEVICE = "frame_" + LEVEL, "device_photons" + LEVEL[len("lights"):]
PATH = LEVEL == "lights_path"
sc = miro_amd.Scene(0)
environment = None
if name == "mixed":
    d = scenes.textured_room_setup(sc, scenes.photon_room_mixed())
    lights, disc = scenes.SCENES["photon_room_two_lights"]["lights"], d["disc_light"]
else:
    d = scenes.flower_setup(sc, scenes.flower_scene(drops=True))
    lights, environment, disc = d["lights"], d["environment"], d["lights"][0]
signal.setitimer(signal.ITIMER_REAL, a.frame_seconds * 2)
maps = sc.photon_maps(disc, a.photons, 400 * a.photons, surface=True)
signal.setitimer(signal.ITIMER_REAL, 0)
stored = [m.count() for m in maps]
maps = tuple(m if n > 0 else None for m, n in zip(maps, stored))
assert maps[0] is not None, "the global map is empty"
renderers = {FRAME: frame.FrameRenderer(sc, d, W, H, spp=spp, tiled=False),
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
                                       fused=fused, photon_maps=maps, nphotons=a.k, max_dist=MAX_DIST, **kwargs)
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
need = sc.recursion_photons_workspace_bytes(dev.cam, W, H, DEPTH, cap, spp=spp, children=children, environment=bool(environment),
                                            kinds=KINDS or 3)
queues = sc.recursion_workspace_bytes(DEPTH, cap, children=children, environment=bool(environment), kinds=KINDS or 3)


def call(stream):
    sc.render_recursion_photons(dev.cam, W, H, dev.d_rgb, dev.d_level_counts, DEPTH, maps[0], maps[1], dev.d_recursion, queue_capacity=cap,
                                max_dist=MAX_DIST, nphotons=a.k, spp=spp, jitter=dev.jitter, seed=dev.seed, stream=stream,
                                children=children, environment=bool(environment), kinds=KINDS or 3, path_seed=29, workspace_bytes=need)


signal.setitimer(signal.ITIMER_REAL, a.frame_seconds * 4)
torch.cuda.synchronize()
want = dev.d_level_counts[:DEPTH + 1].tolist()
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g, stream=side):
    call(torch.cuda.current_stream())
replay_read = []
for k in range(3 + a.frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.replay()
    got = dev.d_level_counts[:DEPTH + 1].tolist()
    t1 = time.perf_counter()
    equal = equal and got == want
    if k >= 3:
        replay_read.append((t1 - t0) * 1e3)
signal.setitimer(signal.ITIMER_REAL, 0)

line = dict(tool="recursion_photons_ab", case=a.case, scene=name, width=W, height=H, spp=spp, depth=DEPTH, lights=len(lights), route=DEVICE,
            against=FRAME, path_kinds=KINDS, environment="colour" if environment else "none", photons=stored, nphotons=a.k,
            per_level=levels_f, level_counts=want, queries=[row[6] for row in want], frames=a.frames,
            device=torch.cuda.get_device_name(0), pictures_agree=equal, max_rel_diff=err, nan_pixels=[int(nan_f.sum()), int(nan_d.sum())],
            queue_capacity=cap, workspace_bytes=int(need), of_which_queues=int(queues),
            frame_route=dict(frame=stats(res[FRAME]), resident_bytes=int(renderers[FRAME].bytes_resident())),
            device_route=dict(frame=stats(res[DEVICE]), resident_bytes=int(dev.bytes_resident())),
            graph_replay=dict(to_counts_read=stats(replay_read)))
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
