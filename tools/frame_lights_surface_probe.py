"""Frame time of mr_render_lights_surface (csrc/mr_frame_lights_surface.hip: one launch, 12 bytes per pixel resident) against the
batched route for the same frame of a textured scene, mr_gen_eye_rays_tiled -> mr_trace -> mr_hit_surface ->
mr_shade_lights_surface (a 32-byte ray, a 16-byte hit record, a 12-byte colour and a 12-byte normal per sample and the pixel
slots resident; zeroing the slots is part of the route, scattering them to image order -- mr_untile_pixels -- is left out, in
the batched route's favour; the parity tests' per-sample L, 12 bytes more, is not part of the timed route either).  Cases:
makeTestPetalScene (scenes.flower_scene(), its disc light) and the stone room (photon_room_stone() under the two lights of
photon_room_two_lights) at 1920 x 1080 x 4 spp, the mixed room (photon_room_mixed(), the same lights) at 1920 x 1080 x 1 spp.
Every case runs in a child process of its own under a time limit of its own (--case-seconds), one after the other, and the
first case that does not end with status 0 ends the run: nothing more is started on a device that may have faulted.  Inside a
case: warm-up (which uploads the texture table), then the two routes alternate; every repetition is a window of --calls frames
between two device events on the stream; median and spread (min, max) of the per-frame time.  Before anything is timed the fused
frame is compared with the pairwise tree over the batched route's per-sample L at the timed size (exact), and the counters with
the batch's.  One JSON line per case, printed and appended to --out.
usage: python tools/frame_lights_surface_probe.py [--reps 15] [--calls 20] [--out profiles/frame_lights_surface_line.json]"""
import argparse, json, os, signal, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

CASES = {"flower": (1920, 1080, 4), "stone": (1920, 1080, 4), "mixed": (1920, 1080, 1)}
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--step-seconds", type=float, default=60.0)
ap.add_argument("--case-seconds", type=float, default=240.0)
ap.add_argument("--case", default="", choices=[""] + sorted(CASES))
ap.add_argument("--out", default="")
a = ap.parse_args()

if not a.case:                                          # the driver: one child per case, none after the first that fails
    for name in ("flower", "stone", "mixed"):
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
if a.case == "flower":
    d = scenes.flower_setup(sc)
    lights = d["lights"]
else:
    d = scenes.textured_room_setup(sc, scenes.photon_room_stone() if a.case == "stone" else scenes.photon_room_mixed())
    lights = scenes.SCENES["photon_room_two_lights"]["lights"]
sc.set_lights(lights)
n, cam = W * H * spp, binding.make_camera(d["eye"], d["lookat"], d["up"], d["fov"])
rays, hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
color, normal, slots = torch.zeros((n, 3), **f32), torch.zeros((n, 3), **f32), torch.zeros((W * H, 3), **f32)
rgb, counts = torch.zeros((W * H, 3), **f32), torch.zeros(3, dtype=torch.int64, device="cuda")
undefined = torch.zeros(1, dtype=torch.int64, device="cuda")


def batched():
    sc.gen_eye_rays(cam, W, H, rays, spp=spp, jitter=True, seed=168, tiled=True)
    sc.trace_device(rays, n, hits)
    sc.hit_surface(rays, hits, n, color, normal)
    slots.zero_()
    sc.shade_lights_surface(rays, hits, color, normal, n, slots, spp=spp)


def fused():
    sc.render_lights_surface(cam, W, H, rgb, spp=spp, jitter=True, seed=168, tiled=True, d_counts=counts)


# ---- the same picture first: the fused frame against the pairwise tree over the batched route's per-sample L
ray_rgb = torch.empty((n, 3), **f32)
batched()
sc.hit_surface(rays, hits, n, color, normal, d_counts=undefined)
sc.shade_lights_surface(rays, hits, color, normal, n, None, spp=spp, d_ray_rgb=ray_rgb)
x = ray_rgb.view(W * H, spp, 3)
while x.shape[1] > 1:
    x = x[:, 0::2] + x[:, 1::2]
x = x[:, 0] * np.float32(1.0 / spp) if spp > 1 else x[:, 0]
want = torch.empty_like(x)
want[torch.from_numpy(binding.tile_pixel_map(W, H, spp).astype(np.int64)).cuda()] = x
counts.zero_()
fused()
torch.cuda.synchronize()
c = counts.cpu().numpy()
n_hits = int((hits[:, 1].contiguous().view(torch.int32) != -1).sum())
equal = bool(torch.equal(rgb, want)) and (int(c[0]), int(c[1]), int(c[2])) == (n, n_hits * len(lights), int(undefined.item()))
del ray_rgb, x, want
for _ in range(3):                                      # warm-up: code objects, the texture table, the library's grow-only scratch
    batched(); fused()
torch.cuda.synchronize()
tb, tf = [], []
for _ in range(a.reps):                                 # alternating
    tb.append(window(batched))
    tf.append(window(fused))
shadow = n_hits * len(lights)
line = dict(tool="frame_lights_surface_probe", scene=a.case, width=W, height=H, spp=spp, lights=len(lights), samples=n, hits=n_hits,
            shadow_rays=shadow, undefined_lookups=int(undefined.item()), reps=a.reps, calls_per_window=a.calls,
            device=torch.cuda.get_device_name(0), pictures_equal=equal, batched=stats(tb), fused=stats(tf),
            speedup=round(float(np.median(tb) / np.median(tf)), 3),
            batched_bytes_resident=nbytes(rays, hits, color, normal, slots), fused_bytes_resident=nbytes(rgb, counts))
txt = json.dumps(line)
print(txt, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt + "\n")
sys.exit(0 if equal else 3)
