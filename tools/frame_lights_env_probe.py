"""Frame time of mr_render_lights_environment (csrc/mr_frame_lights_env.hip: one launch, 12 bytes per pixel resident) against
the batched route for the same frame, mr_gen_eye_rays_tiled -> mr_trace -> mr_hit_surface -> mr_shade_lights_surface ->
mr_shade_environment (a 32-byte ray, a 16-byte hit record, a 12-byte colour and a 12-byte normal per sample and the pixel slots
resident; zeroing the slots is part of the route, scattering them to image order -- mr_untile_pixels -- is left out, in the
batched route's favour; the parity tests' per-sample values, 24 bytes more, are not part of the timed route either), and against
mr_render_lights_surface on the same frame, whose misses are worth 0: the difference is what the lookup costs.  The environment
is a seeded 2048 x 1024 float image (the size of an HDR panorama; 32 MiB of 16-byte texel records on the device), rotated as
assignment3.cpp rotates its own.  Cases: makeTestPetalScene (scenes.flower_scene(), its disc light; most of the frame is sky) at
1920 x 1080 x 1 and x 4 spp.  Every case runs in a child process of its own under a time limit of its own (--case-seconds), one
after the other, and the first case that does not end with status 0 ends the run: nothing more is started on a device that may
have faulted.  Inside a case: warm-up (which uploads the texture table and the image), then the three routes alternate; every
repetition is a window of --calls frames between two device events on the stream; median and spread (min, max) of the per-frame
time.  Before anything is timed the fused frame is compared with the pairwise tree over the batched route's per-sample L (the
light chain's row where the ray hit, the environment chain's where it missed) at the timed size (exact), and the five counters
with the batch's.  One JSON line per case, printed and appended to --out.
usage: python tools/frame_lights_env_probe.py [--reps 15] [--calls 20] [--out profiles/frame_lights_env_line.json]"""
import argparse, json, math, os, signal, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

CASES = {"flower1": (1920, 1080, 1), "flower4": (1920, 1080, 4)}
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--step-seconds", type=float, default=60.0)
ap.add_argument("--case-seconds", type=float, default=240.0)
ap.add_argument("--case", default="", choices=[""] + sorted(CASES))
ap.add_argument("--out", default="")
a = ap.parse_args()

if not a.case:                                          # the driver: one child per case, none after the first that fails
    for name in sorted(CASES):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--calls", str(a.calls),
               "--step-seconds", str(a.step_seconds)] + (["--out", a.out] if a.out else [])
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
from miro_amd import binding, scenes  # noqa: E402

f32 = dict(dtype=torch.float32, device="cuda")
signal.signal(signal.SIGALRM, signal.SIG_DFL)                      # the default action ends the process, also inside the runtime


def window(fn):
    """per-frame milliseconds of --calls frames between two events; a window longer than --step-seconds ends the process"""
    signal.setitimer(signal.ITIMER_REAL, a.step_seconds)
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(min(ts)), 4), max_ms=round(float(max(ts)), 4))


def nbytes(*ts):
    return int(sum(t.numel() * t.element_size() for t in ts))


assert torch.cuda.is_available(), "the probe measures on the GPU"
W, H, spp = CASES[a.case]
sc = miro_amd.Scene(0)
d = scenes.flower_setup(sc)
lights = d["lights"]
sc.set_lights(lights)
EW, EH = 2048, 1024
sc.set_environment(pixels=(np.random.default_rng(168).random((EH, EW, 3)) * 4.0).astype(np.float32),
                   rotation=(math.pi / 3 + 0.05, math.pi / 8))
n, cam = W * H * spp, binding.make_camera(d["eye"], d["lookat"], d["up"], d["fov"])
rays, hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
color, normal, slots = torch.zeros((n, 3), **f32), torch.zeros((n, 3), **f32), torch.zeros((W * H, 3), **f32)
rgb, counts = torch.zeros((W * H, 3), **f32), torch.zeros(5, dtype=torch.int64, device="cuda")
rgb0, counts0 = torch.zeros((W * H, 3), **f32), torch.zeros(3, dtype=torch.int64, device="cuda")
undefined, env_counts = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")


def batched():
    sc.gen_eye_rays(cam, W, H, rays, spp=spp, jitter=True, seed=168, tiled=True)
    sc.trace_device(rays, n, hits)
    sc.hit_surface(rays, hits, n, color, normal)
    slots.zero_()
    sc.shade_lights_surface(rays, hits, color, normal, n, slots, spp=spp)
    sc.shade_environment(rays, hits, n, slots, spp=spp)


def fused():
    sc.render_lights_environment(cam, W, H, rgb, spp=spp, jitter=True, seed=168, tiled=True, d_counts=counts)


def fused_without():
    sc.render_lights_surface(cam, W, H, rgb0, spp=spp, jitter=True, seed=168, tiled=True, d_counts=counts0)


# ---- the same picture first: the fused frame against the pairwise tree over the batched route's per-sample L
ray_rgb, env_rgb = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
batched()
sc.hit_surface(rays, hits, n, color, normal, d_counts=undefined)
sc.shade_lights_surface(rays, hits, color, normal, n, None, spp=spp, d_ray_rgb=ray_rgb)
sc.shade_environment(rays, hits, n, None, spp=spp, d_ray_rgb=env_rgb, d_counts=env_counts)
hit_rows = hits[:, 1].contiguous().view(torch.int32) != -1
x = torch.where(hit_rows[:, None], ray_rgb, env_rgb).view(W * H, spp, 3)
while x.shape[1] > 1:
    x = x[:, 0::2] + x[:, 1::2]
x = x[:, 0] * np.float32(1.0 / spp) if spp > 1 else x[:, 0]
want = torch.empty_like(x)
want[torch.from_numpy(binding.tile_pixel_map(W, H, spp).astype(np.int64)).cuda()] = x
counts.zero_()
fused()
torch.cuda.synchronize()
c = [int(v) for v in counts.cpu().numpy()]
e = [int(v) for v in env_counts.cpu().numpy()]
n_hits = int(hit_rows.sum())
equal = bool(torch.equal(rgb, want)) and c == [n, n_hits * len(lights), int(undefined.item()), e[0], e[1]] and e[0] == n - n_hits
del ray_rgb, env_rgb, x, want, hit_rows
for _ in range(3):                                      # warm-up: code objects, the table, the image, the library's grow-only scratch
    batched(); fused(); fused_without()
torch.cuda.synchronize()
tb, tf, t0 = [], [], []
for _ in range(a.reps):                                 # alternating
    tb.append(window(batched))
    tf.append(window(fused))
    t0.append(window(fused_without))
line = dict(tool="frame_lights_env_probe", scene="flower", width=W, height=H, spp=spp, lights=len(lights), samples=n, hits=n_hits,
            misses=e[0], undefined_environment_lookups=e[1], environment=[EW, EH], reps=a.reps, calls_per_window=a.calls,
            device=torch.cuda.get_device_name(0), pictures_equal=equal, batched=stats(tb), fused=stats(tf), fused_without_environment=stats(t0),
            speedup=round(float(np.median(tb) / np.median(tf)), 3), lookup_cost_ms=round(float(np.median(tf) - np.median(t0)), 4),
            batched_bytes_resident=nbytes(rays, hits, color, normal, slots), fused_bytes_resident=nbytes(rgb, counts))
txt = json.dumps(line)
print(txt, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt + "\n")
sys.exit(0 if equal else 3)
