"""Frame time of mr_render_lights (csrc/mr_frame_lights.hip: one launch, 12 bytes per pixel resident) against the batched route
for the same frame, mr_gen_eye_rays_tiled -> mr_trace -> mr_shade_lights (a 32-byte ray, a 16-byte hit record per sample and the
pixel slots resident; zeroing the slots is part of the route, scattering them to image order -- mr_untile_pixels -- is left out,
in the batched route's favour).  Cases: the sponza stand-in with 1, 2 and 4 point lights at 1920 x 1080 x 4 spp, and
photon_room_two_lights (disc + point, glass and mirror spheres) at 1024 x 1024 x 16 spp.  Both routes run in this one process:
warm-up, then they alternate; every repetition is a window of --calls frames between two device events on the stream; median
and spread (min, max) of the per-frame time.  Before anything is timed the fused frame is compared with the batched route's
per-sample L at the timed size (pairwise tree, exact).  With one light the same frame is also timed through mr_render_direct,
and all three report shadow rays per second OF THE WHOLE FRAME (shadow rays traced / frame time: the primary rays are in it).
Every window runs under a time limit of its own (the process is ended if one exceeds --step-seconds).  One JSON line per case,
printed and appended to --out.
usage: python tools/frame_lights_probe.py [--reps 15] [--calls 20] [--out profiles/frame_lights_line.json]"""
import argparse, json, os, signal, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))
import numpy as np, torch
import miro_amd
from miro_amd import binding, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--step-seconds", type=float, default=60.0)
ap.add_argument("--out", default="")
a = ap.parse_args()
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


def sponza_lights(sc, d):
    """the description's own point light, then three spread over the upper half of the scene's box (tools/lights_probe.py)"""
    v = sc.arrays()[0]
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = hi - lo
    out = [dict(position=tuple(float(c) for c in d["light"]), color=(1.0, 1.0, 1.0), wattage=d["wattage"])]
    for fx, fy, fz in ((0.3, 0.7, 0.35), (0.7, 0.6, 0.65), (0.5, 0.8, 0.5)):
        out.append(dict(position=(float(lo[0] + fx * ext[0]), float(lo[1] + fy * ext[1]), float(lo[2] + fz * ext[2])),
                        color=(0.9, 0.8, 0.7), wattage=0.5 * d["wattage"]))
    return out


def one_case(sc, d, label, lights, W, H, spp):
    n, cam = W * H * spp, binding.make_camera(d["eye"], d["lookat"], d["up"], d["fov"])
    sc.set_lights(lights)
    rays, hits, slots = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32), torch.zeros((W * H, 3), **f32)
    rgb, counts = torch.zeros((W * H, 3), **f32), torch.zeros(2, dtype=torch.int64, device="cuda")

    def batched():
        sc.gen_eye_rays(cam, W, H, rays, spp=spp, jitter=True, seed=168, tiled=True)
        sc.trace_device(rays, n, hits)
        slots.zero_()
        sc.shade_lights(rays, hits, n, slots, spp=spp)

    def fused():
        sc.render_lights(cam, W, H, rgb, spp=spp, jitter=True, seed=168, tiled=True, d_counts=counts)

    # ---- the same picture first: the fused frame against the pairwise tree over the batched route's per-sample L
    ray_rgb = torch.empty((n, 3), **f32)
    batched()
    sc.shade_lights(rays, hits, n, None, spp=spp, d_ray_rgb=ray_rgb)
    x = ray_rgb.view(W * H, spp, 3)
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    x = x[:, 0] * np.float32(1.0 / spp)
    want = torch.empty_like(x)
    want[torch.from_numpy(binding.tile_pixel_map(W, H, spp).astype(np.int64)).cuda()] = x
    counts.zero_()
    fused()
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    n_hits = int((hits[:, 1].contiguous().view(torch.int32) != -1).sum())
    equal = bool(torch.equal(rgb, want)) and (int(c[0]), int(c[1])) == (n, n_hits * len(lights))
    del ray_rgb, x, want
    for _ in range(3):                                  # warm-up: code objects, the library's grow-only scratch
        batched(); fused()
    torch.cuda.synchronize()
    tb, tf = [], []
    for _ in range(a.reps):                             # alternating
        tb.append(window(batched))
        tf.append(window(fused))
    shadow = n_hits * len(lights)
    line = dict(tool="frame_lights_probe", scene=label, width=W, height=H, spp=spp, lights=len(lights), samples=n, hits=n_hits,
                shadow_rays=shadow, reps=a.reps, calls_per_window=a.calls, device=torch.cuda.get_device_name(0), pictures_equal=equal,
                batched=stats(tb), fused=stats(tf), speedup=round(float(np.median(tb) / np.median(tf)), 3),
                batched_bytes_resident=nbytes(rays, hits, slots), fused_bytes_resident=nbytes(rgb, counts),
                fused_shadow_rays_per_s_of_frame=round(shadow / (float(np.median(tf)) * 1e-3), 1),
                batched_shadow_rays_per_s_of_frame=round(shadow / (float(np.median(tb)) * 1e-3), 1))
    if len(lights) == 1 and "normal" not in lights[0]:
        # the single-light kernel on the same frame (its own material handling: the scene's table, or its uniform white)
        lt = lights[0]

        def direct():
            sc.render_direct(cam, W, H, rgb, lt["position"], lt["wattage"], spp=spp, jitter=True, seed=168, tiled=True, color=lt["color"],
                             d_counts=counts)

        for _ in range(3):
            direct()
        counts.zero_()
        direct()
        torch.cuda.synchronize()
        direct_shadow = int(counts.cpu().numpy()[1])
        td, tf2 = [], []
        for _ in range(a.reps):
            td.append(window(direct))
            tf2.append(window(fused))
        line["render_direct"] = stats(td)
        line["fused_next_to_render_direct"] = stats(tf2)
        line["render_direct_shadow_rays"] = direct_shadow
        line["render_direct_shadow_rays_per_s_of_frame"] = round(direct_shadow / (float(np.median(td)) * 1e-3), 1)
    txt = json.dumps(line)
    print(txt, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(txt + "\n")


assert torch.cuda.is_available(), "the probe measures on the GPU"
d = scenes.SCENES["sponza"]
sc = miro_amd.Scene(0)
scenes.populate(sc, d)
sc.build(4)
points = sponza_lights(sc, d)
for k in (1, 2, 4):
    one_case(sc, d, scenes.sponza_label(), points[:k], 1920, 1080, 4)
d = scenes.SCENES["photon_room_two_lights"]
sc = miro_amd.Scene(0)
scenes.populate(sc, d)
sc.set_materials(d["materials"], d["prim_material"])
sc.build(4)
one_case(sc, d, "photon_room_two_lights", d["lights"], 1024, 1024, 16)
