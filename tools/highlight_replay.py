"""In how many waves of the fused frame is the highlight's powf computed for nothing?  

highlight_of (mr_phong.h) raises the clamped cosine e between the eye and the mirror direction to the 500th power; below
2^-0.3 = 0.8123 the result is exactly +0.  With ZERO_GUARD the frame kernel writes that +0 without the call when every lane of the
wave that holds a hit has e < T = kHighlightZeroBelow.  This is the count: the oracle's rays and hits, then surface_od,
normalize3, phong_terms and highlight_of restated in numpy float32 in the kernel's operation order (every operation rounded by
itself, as -ffp-contract=off compiles them; float32 numpy division and square root are the IEEE ones), and per wave of 64
consecutive samples whether every hit lane, some or none is below T.

    python tools/highlight_replay.py            # the sample of the bench frame (tools/tri_guard_replay.py's): 360 waves of nine
                                                # rows of sponza 1920x1080, at 64 spp (image order), 16 and 1 spp (tiled order)
    python tools/highlight_replay.py --spp 64 --scene teapot --w 512 --h 512

No GPU: the tree and the rays are the oracle's.  tests/test_frame_highlight_guard.py imports the model."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "cse168-raytracer_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F = np.float32
T = F(0.75)                # kHighlightZeroBelow of mr_phong.h
MISS = np.uint32(0xFFFFFFFF)
KINDS = ("no_hit", "all_below", "all_above", "mixed")


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def clamped_e(arrays, rays, hits, light):
    """highlight_of's e after the clamp, per ray (NaN where the ray has no hit): surface_od<true> of mr_surface.h for a triangle,
    normalize3, the l of phong_terms, the mirror direction and the clamp of highlight_of -- float32, the kernel's order"""
    v, n, vi, ni = arrays
    hit = hits["prim"] != MISS
    prim = np.where(hit, hits["prim"], 0).astype(np.int64)
    beta, gamma = hits["beta"].astype(F), hits["gamma"].astype(F)
    with np.errstate(all="ignore"):
        A = v[vi[prim, 0]].astype(F)
        BmA, CmA = v[vi[prim, 1]].astype(F) - A, v[vi[prim, 2]].astype(F) - A
        P = (A + beta[:, None] * BmA) + gamma[:, None] * CmA
        alpha = F(1) - beta - gamma
        N = (alpha[:, None] * n[ni[prim, 0]].astype(F) + beta[:, None] * n[ni[prim, 1]].astype(F)) + gamma[:, None] * n[ni[prim, 2]].astype(F)
        N = N * (F(1) / np.sqrt(_dot(N, N)))[:, None]                                     # normalize3
        l = np.asarray(light, F)[None, :] - P                                              # phong_terms
        l = l * (F(1) / np.sqrt(_dot(l, l)))[:, None]
        two = F(2) * _dot(l, N)                                                            # highlight_of
        r = -l + two[:, None] * N
        d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1).astype(F)
        e = (-d[:, 0] * r[:, 0] + -d[:, 1] * r[:, 1]) + -d[:, 2] * r[:, 2]
        e = clamp(e)
    e[~hit] = np.nan
    return e, hit


def clamp(e):
    """fmaxf(0.0f, fminf(1.0f, e)): a NaN leaves as 1"""
    return np.fmax(F(0), np.fmin(F(1), np.asarray(e, F)))


def sure(e):
    """a lane's test on its clamped e; false for whatever is not below T"""
    with np.errstate(invalid="ignore"):
        return np.asarray(e, F) < T


def wave_skips(e, lanes):
    """the guard of highlight_of on one wave: the ballot of `e < T` equals the ballot of `true` over the lanes that are there"""
    lanes = np.asarray(lanes, bool)
    return bool(np.array_equal(sure(e) & lanes, lanes))


def wave_kinds(e, hit):
    """per wave of 64 consecutive samples (the last one may be ragged): an index into KINDS"""
    kinds = []
    for w in range(0, len(e), 64):
        lanes, ew = hit[w:w + 64], e[w:w + 64]
        if not lanes.any():
            kinds.append(0)
        elif wave_skips(ew, lanes):
            kinds.append(1)
        elif not (sure(ew) & lanes).any():
            kinds.append(2)
        else:
            kinds.append(3)
    return np.array(kinds)


def count_kinds(kinds):
    return {k: int((kinds == i).sum()) for i, k in enumerate(KINDS)}


def sample_waves(po, cam, W, H, spp, rows, first, every):
    """the rays of one wave per sampled pixel: at 64 spp the pixel's own samples (image order); below, the block of the tiled order
    (mr_tile.h: th x tw pixels, row by row, a pixel's samples consecutive) that holds the pixel"""
    th, tw = 1, 1
    pixels = 64 // spp
    while pixels > 1:
        th *= 2; pixels //= 2
        if pixels > 1:
            tw *= 2; pixels //= 2
    out = []
    for row in rows:
        y0 = row // th * th
        band = po.eye_rays(cam, W, H, spp=spp, jitter=spp > 1, y0=y0, y1=y0 + th)
        for x in range(first, W, every):
            x0 = x // tw * tw
            if x0 + tw > W:
                continue
            idx = [((r * W + x0 + xi) * spp + s) for r in range(th) for xi in range(tw) for s in range(spp)]
            out.append(band[np.asarray(idx)])
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--spp", type=int, nargs="*", default=[64, 16, 1])
    ap.add_argument("--rows", type=int, nargs="*", default=[60, 200, 330, 470, 540, 610, 760, 900, 1040])
    ap.add_argument("--first", type=int, default=24)
    ap.add_argument("--every", type=int, default=48)
    a = ap.parse_args()
    import pyoracle as po
    from miro_amd import scenes
    po.build()
    d = scenes.SCENES[a.scene]
    sc = po.Scene()
    scenes.populate(sc, d)
    sc.build(4)
    cam = po.make_camera(d["eye"], d["lookat"], d["up"], d["fov"])
    print("%s %dx%d, rows %s, every %dth pixel from %d; T = %s" % (a.scene, a.w, a.h, a.rows, a.every, a.first, T))
    for spp in a.spp:
        rays = sample_waves(po, cam, a.w, a.h, spp, a.rows, a.first, a.every)
        hits = sc.trace(rays)
        e, hit = clamped_e(sc.arrays(), rays, hits, d["light"])
        c = count_kinds(wave_kinds(e, hit))
        n_hit = max(c["all_below"] + c["all_above"] + c["mixed"], 1)
        below = sure(e) & hit
        print("  %2d spp (%s): %d waves, %d hold a hit; every hit lane below T (skipped) %.3f, some lanes below %.3f, none %.3f; "
              "hit samples below T %.3f, below 2^-0.3 %.3f; largest e %.6f" % (
                  spp, "image order" if spp == 64 else "tiled order", len(rays) // 64, n_hit, c["all_below"] / n_hit, c["mixed"] / n_hit,
                  c["all_above"] / n_hit, below.sum() / max(hit.sum(), 1), (e[hit] < F(2.0 ** -0.3)).sum() / max(hit.sum(), 1),
                  np.nanmax(e) if hit.any() else float("nan")))


if __name__ == "__main__":
    main()
