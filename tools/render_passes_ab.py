"""Frame time of FrameRenderer.render_specular(fused="device_*", samples=256) -- ONE library call, mr_render_recursion_passes
(include/miro_hip_passes.h: the one-call recursive frame enqueued once per pass over one workspace; level 0 of a pass is a kernel
of csrc/mr_frame_passes.hip), then ONE read of the counters -- on the same commit against what a caller could do before it:

  summed    four render_specular(fused="device_*") frames at 64 spp with four seeds into the renderer's d_rgb as a scratch buffer,
            and acc += scratch / 4 in torch after each: four library calls, four read-backs, a second framebuffer, and a picture
            that depends on the cut into calls;
  passes64  samples=256 in passes of 64 (the same renderer: the same workspace);
  passes16, passes4   samples=256 in passes of 16 and of 4: pass size trades queue memory against launches.

1920 x 1080, depth 3: the flower with drops under its colour (pinhole, specular children), the same through the flower scene's own
lens (DOF_APERTURE 0.20, DOF_FOCUS_PLANE 15.3, Miro.h:18-19), and the flower path traced through that lens (path_kinds 7, path_seed
29) -- the scenes of tools/recursion_ab.py and tools/recursion_lens_ab.py.  On the lens cases the reference's own configuration,
samples=1000 in passes of 64 (15 x 64, 32, 8), runs once after the timed frames, for the record.  The renderers are built with
resident_rays=False; queue_capacity is the default (fan x a pass's samples).

Every case runs in a child process of its own under a time limit of its own (--case-seconds), one after the other, and the first
case that does not end with status 0 ends the run: nothing more is started on a device that may have faulted.  Inside a case the
pictures are compared first: passes16 and passes4 against passes64 (per_level equal, pixels within 2e-5 of the largest value; a
pixel that holds a NaN must hold one in both) -- the summed frames are another picture (other seeds) and are compared by their
mean only.  Then one warm frame of each route, then the routes alternate frame by frame, --frames frames each.  A frame is timed by
the host clock from the call to its return, after a device synchronise on either side.  resident_bytes is bytes_resident() of each
renderer after its frames (summed: plus its accumulation buffer).  One JSON line per case, printed and appended to --out.
usage: python tools/render_passes_ab.py [--frames 20] [--only a,b] [--out lines.json]   (profiles/render_passes_ab.log)"""
import argparse, json, os, signal, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

# route of the frame, path_kinds, through the lens
CASES = {"flower": ("device_lights", 0, False), "flower_lens": ("device_lens", 0, True), "path_flower_lens": ("device_lens_path", 7, True)}
ORDER = tuple(CASES)
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--frame-seconds", type=float, default=120.0)
ap.add_argument("--case-seconds", type=float, default=420.0)
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
W, H, DEPTH, S, SEEDS = 1920, 1080, 3, 256, (168, 169, 170, 171)
ROUTE, KINDS, WITH_LENS = CASES[a.case]
sc = miro_amd.Scene(0)
d = scenes.flower_setup(sc, scenes.flower_scene(drops=True))
lights, environment = d["lights"], d["environment"]
lens = dict(aperture=0.20, focus_plane=15.3) if WITH_LENS else None          # Miro.h:18-19
kwargs = dict(path_tracing=True, path_kinds=KINDS, path_seed=29) if KINDS else {}
renderers = {p: frame.FrameRenderer(sc, d, W, H, spp=p, jitter=True, tiled=False, lens=lens, resident_rays=False) for p in (64, 16, 4)}
acc = torch.zeros_like(renderers[64].d_rgb)
first = True
ROUTES = ("summed", "passes64", "passes16", "passes4")


def render(fr, **kw):
    global first
    out = fr.render_specular(depth=DEPTH, lights=lights, environment=(environment if first else True) if environment else None,
                             fused=ROUTE, **kwargs, **kw)
    first = False
    return out


def one_frame(route, samples=S):
    """(frame ms by the host clock, per_level)"""
    signal.setitimer(signal.ITIMER_REAL, a.frame_seconds)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "summed":
            fr = renderers[64]
            per_level = None
            for i, seed in enumerate(SEEDS):
                fr.seed = seed
                levels = render(fr)
                per_level = levels if per_level is None else [(x[0] + y[0], x[1] + y[1]) for x, y in zip(per_level, levels)]
                if i == 0:
                    torch.mul(fr.d_rgb, 1.0 / len(SEEDS), out=acc)
                else:
                    acc.add_(fr.d_rgb, alpha=1.0 / len(SEEDS))
            fr.seed = SEEDS[0]
        else:
            per_level = render(renderers[int(route[6:])], samples=samples)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3, per_level
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(min(ts)), 4), max_ms=round(float(max(ts)), 4))


# ---- the same picture first: the three pass sizes render one frame; the summed frames another one of the same mean
pictures, levels = {}, {}
for route in ROUTES:
    _, levels[route] = one_frame(route)
    pictures[route] = (acc if route == "summed" else renderers[int(route[6:])].d_rgb).clone()
want = pictures["passes64"]
nan_w = torch.isnan(want).any(dim=1)
top = float(want[~nan_w].abs().max())
errs, equal = {}, True
for route in ("passes16", "passes4"):
    nan_g = torch.isnan(pictures[route]).any(dim=1)
    finite = ~(nan_w | nan_g)
    errs[route] = float((pictures[route][finite] - want[finite]).abs().max()) / top
    equal = equal and levels[route] == levels["passes64"] and bool(torch.equal(nan_w, nan_g)) and errs[route] <= 2e-5
finite = ~(nan_w | torch.isnan(pictures["summed"]).any(dim=1))
mean_ratio = float(pictures["summed"][finite].mean()) / float(want[finite].mean())
del pictures
res = {r: [] for r in ROUTES}
for _ in range(a.frames):                               # alternating (the comparison frames above were the warm ones)
    for route in ROUTES:
        res[route].append(one_frame(route)[0])

line = dict(tool="render_passes_ab", case=a.case, scene="flower_drops", width=W, height=H, samples=S, depth=DEPTH, lights=len(lights),
            lens=lens, route=ROUTE, path_kinds=KINDS, per_level=levels["passes64"], frames=a.frames, device=torch.cuda.get_device_name(0),
            pictures_agree=equal, max_rel_diff=errs, summed_mean_over_passes_mean=round(mean_ratio, 5), nan_pixels=int(nan_w.sum()))
for route in ROUTES:
    fr = renderers[64 if route == "summed" else int(route[6:])]
    extra = acc.numel() * acc.element_size() if route == "summed" else 0
    line[route] = dict(frame=stats(res[route]), resident_bytes=int(fr.bytes_resident()) + extra)
sm = line["summed"]["frame"]["median_ms"]
for route in ROUTES[1:]:
    line[route]["over_summed"] = round(line[route]["frame"]["median_ms"] / sm, 3)
    line[route]["verdict"] = "level" if abs(line[route]["over_summed"] - 1.0) <= 0.02 else "faster" if line[route]["over_summed"] < 1.0 else "SLOWER"
if WITH_LENS:                                           # the reference's own configuration, once
    ms, per_level = one_frame("passes64", samples=1000)
    line["samples_1000_passes64"] = dict(frame_ms=round(ms, 2), per_level=per_level, passes=len(miro_amd.binding.passes_plan(64, 1000)))
txt = json.dumps(line)
print(txt, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt + "\n")
sys.exit(0 if equal else 3)
