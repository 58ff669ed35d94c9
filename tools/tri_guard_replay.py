"""How many triangle tests of the fused frame's uniform leaves does a whole wave surely reject?  

The CPU replay of the frame kernel's walks -- replay_walks of tests/test_frame_uniform_walk.py -- with counters inside its
leaf(): for every wave-level triangle test of a uniform leaf (one triangle for all the lanes that take part: the leaf loop of
uniform_walk, leaf_step's scalar arm) whether every lane rejects it, and whether every lane is SURE of that from the guard of
mr_traverse.h (tri_surely_rejects), modelled here in numpy float32.  The counters sit in a trace hook on leaf()'s calls, so the
replay itself stays the one the GPU tests hold against the kernel's hit records.

    python tools/tri_guard_replay.py                       # the sample of the bench frame: 360 pixel-waves, sponza 1920x1080x64
    python tools/tri_guard_replay.py --spp 16 --rows 540   # other frames

No GPU: the tree and the rays are the oracle's.  tests/test_frame_triangle_guard.py imports the model and the hook."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "cse168-raytracer_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F = np.float32
K_EPS = F(1e-4)            # Miro.h:9
SIGN = np.uint32(0x80000000)
TWO_13 = np.uint32(0x46000000)


def guard_sure(nb, ng, ddotn):
    """tri_surely_rejects of mr_traverse.h on float32 arrays: nb * k < -|ddotn| or ng * k < -|ddotn|, k = 2^13 with ddotn's sign bit"""
    nb, ng, ddotn = (np.ascontiguousarray(x, F) for x in (nb, ng, ddotn))
    k = ((ddotn.view(np.uint32) & SIGN) | TWO_13).view(F)
    lim = -np.abs(ddotn)
    with np.errstate(all="ignore"):
        return (nb * k < lim) | (ng * k < lim)


def reference_rejects(pn, nb, ng, ddotn, tmin, tmax):
    """Triangle.cpp:158 on the IEEE quotients (numpy float32 division)"""
    with np.errstate(all="ignore"):
        t, beta, gamma = F(pn) / ddotn, nb / ddotn, ng / ddotn
        return (beta < -K_EPS) | (gamma < -K_EPS) | (beta + gamma > F(1) + K_EPS) | (t < tmin) | (t > tmax)


COUNTS = ("tests_in_walks", "tests_outside", "all_reject", "all_sure", "guarded", "skipped")


class GuardCounts:
    """with GuardCounts(shadow) as g: replay_walks(...) -- counts the wave-level tests of uniform leaves in g.c.
    shadow: the rays are shadow rays (traced on the scene's own tables: the kernel guards those in leaf_step's scalar arm only,
    the eye rays' in the walk's leaf loop too)."""

    def __init__(self, shadow=False):
        self.shadow = shadow
        self.c = dict.fromkeys(COUNTS, 0)

    def __enter__(self):
        self._prev = sys.gettrace()
        sys.settrace(self._trace)
        return self

    def __exit__(self, *exc):
        sys.settrace(self._prev)
        return False

    def _trace(self, frame, event, arg):
        code = frame.f_code
        if event == "call" and code.co_name == "leaf" and code.co_filename.endswith("test_frame_uniform_walk.py"):
            self._leaf(frame)
        return None                        # no line events

    def _leaf(self, frame):
        v = frame.f_locals                 # leaf()'s arguments and the variables of replay_walks it uses
        outer = frame.f_back
        while outer is not None and outer.f_code.co_name != "replay_walks":
            outer = outer.f_back
        w = outer.f_locals
        lanes, walking = v["lanes"], v["walking"]
        if not w["run_walk"]:
            return                         # a wave outside the octant loops takes no run, and no guard
        if not (walking or np.array_equal(w["cur"] != -1, lanes)):
            return                         # lanes at different leaves: the per-lane arm
        o, md, A, N, E1, E2 = v["o"], v["md"], v["A"], v["N"], v["E1"], v["E2"]
        best = v["best"].copy()
        first, cnt = int(v["meta"][v["node"], 1]), int(v["meta"][v["node"], 2])
        c = self.c
        with np.errstate(all="ignore"):
            for k in range(first, first + cnt):
                p = o - A[k]
                ddotn = (md[:, 0] * N[k, 0] + md[:, 1] * N[k, 1]) + md[:, 2] * N[k, 2]
                pn = (p[:, 0] * N[k, 0] + p[:, 1] * N[k, 1]) + p[:, 2] * N[k, 2]
                ux = p[:, 1] * E2[k, 2] - p[:, 2] * E2[k, 1]
                uy = p[:, 2] * E2[k, 0] - p[:, 0] * E2[k, 2]
                uz = p[:, 0] * E2[k, 1] - p[:, 1] * E2[k, 0]
                nb = (md[:, 0] * ux + md[:, 1] * uy) + md[:, 2] * uz
                wx = E1[k, 1] * p[:, 2] - E1[k, 2] * p[:, 1]
                wy = E1[k, 2] * p[:, 0] - E1[k, 0] * p[:, 2]
                wz = E1[k, 0] * p[:, 1] - E1[k, 1] * p[:, 0]
                ng = (md[:, 0] * wx + md[:, 1] * wy) + md[:, 2] * wz
                reject = reference_rejects(pn, nb, ng, ddotn, F(0), best)
                sure = guard_sure(nb, ng, ddotn)
                assert not (sure & ~reject & lanes).any(), "a lane is sure of a rejection the reference does not make"
                t = pn / ddotn
                take = lanes & ~reject & (t < best)
                best[take] = t[take]
                c["tests_in_walks" if walking else "tests_outside"] += 1
                c["all_reject"] += int(reject[lanes].all())
                c["all_sure"] += int(sure[lanes].all())
                if walking and self.shadow:
                    continue               # the shadow trace's walk keeps the unguarded loop (kernel budget, item 24)
                c["guarded"] += 1
                c["skipped"] += int(sure[lanes].all())


def shadow_waves(rays_made, src, n):
    """shadow rays in the lane order of the frame's waves: sample i's ray at index i, tMax = -1 where there is none"""
    rays = np.zeros(n, dtype=rays_made.dtype)
    rays["dx"] = rays["dy"] = rays["dz"] = 1.0
    rays["tmax"] = -1.0
    rays[np.asarray(src, np.int64)] = rays_made
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rows", type=int, nargs="*", default=[60, 200, 330, 470, 540, 610, 760, 900, 1040])
    ap.add_argument("--first", type=int, default=24)
    ap.add_argument("--every", type=int, default=48)
    a = ap.parse_args()
    import pyoracle as po
    from miro_amd import scenes
    from test_frame_uniform_walk import replay_walks, triangle_records
    po.build()
    d = scenes.SCENES[a.scene]
    sc = po.Scene()
    scenes.populate(sc, d)
    sc.build(4)
    corners, meta, _ = sc.export_tree()
    tris = triangle_records(sc)
    cam = po.make_camera(d["eye"], d["lookat"], d["up"], d["fov"])
    per_pixel = a.spp                                   # image order: a pixel's samples are consecutive
    tot = {False: dict.fromkeys(COUNTS, 0), True: dict.fromkeys(COUNTS, 0)}
    waves = 0
    for row in a.rows:
        row_rays = po.eye_rays(cam, a.w, a.h, spp=a.spp, jitter=a.spp > 1, y0=row, y1=row + 1)
        px = max(64 // per_pixel, 1)                   # a wave: 64 consecutive samples, 64 / spp neighbouring pixels
        pick = np.concatenate([np.arange(x * per_pixel, (x + px) * per_pixel) for x in range(a.first, a.w - px + 1, max(a.every, px))])
        rays = row_rays[pick]
        hits = sc.trace(rays)
        made, src = sc.shadow_rays(rays, hits, d["light"])
        for shadow, rr in ((False, rays), (True, shadow_waves(made, src, len(rays)))):
            with GuardCounts(shadow) as g:
                replay_walks(corners, meta, tris, rr)
            for k in COUNTS:
                tot[shadow][k] += g.c[k]
        waves += len(rays) // 64
    print("%s %dx%dx%d, rows %s, every %dth pixel from %d: %d waves" % (a.scene, a.w, a.h, a.spp, a.rows, a.every, a.first, waves))
    for shadow in (False, True):
        c = tot[shadow]
        n = max(c["tests_in_walks"] + c["tests_outside"], 1)
        print("  %-7s wave-level tests per wave %.2f inside walks + %.2f outside; rejected by every lane %.3f; every lane sure (G1) %.3f; "
              "guarded by the kernel %.2f per wave, skipped %.3f of those" % (
                  "shadow" if shadow else "primary", c["tests_in_walks"] / waves, c["tests_outside"] / waves, c["all_reject"] / n,
                  c["all_sure"] / n, c["guarded"] / waves, c["skipped"] / max(c["guarded"], 1)))


if __name__ == "__main__":
    main()
