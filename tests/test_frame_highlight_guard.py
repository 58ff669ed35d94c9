"""The zero guard of the fused frame's highlight (mr_phong.h: highlight_of<true>): a wave whose hit
lanes all have a clamped e below kHighlightZeroBelow = 0.75 writes e = +0 without calling powf(e, 500.0f), whose result there is
+0 (tools/pow_zero_probe.hip, profiles/pow_zero_probe.log).

CPU: the guard modelled in numpy float32 (tools/highlight_replay.py: clamp / sure / wave_skips) never fires for a wave in which
some lane's clamped e is T or more, a NaN among them; T and its neighbours; T^500 against the rounding boundary 2^-150.

GPU: the pixels of the fused frame stay the batched pipeline's, byte for byte -- gen_eye_rays -> trace -> shadow chain ->
mr_shade_direct, which keeps the plain powf.  The scene is one quad with the light next to the eye, so that the mirror direction
passes through the image: e is 1 in the middle and falls below T on a ring around it.  That a frame holds the kinds of wave it is
about -- wholly below T (skipped), wholly above, holding both -- is asserted with the replay of tools/highlight_replay.py on the
frame's own rays and the kernel's own hit records."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from highlight_replay import KINDS, T, clamp, clamped_e, count_kinds, sure, wave_kinds, wave_skips  # noqa: E402
from miro_amd import frame as mframe  # noqa: E402
from miro_amd import scenes  # noqa: E402
from test_frame_uniform_walk import _bits, _card, _desc, _render  # noqa: E402

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_the_constant_is_far_below_the_rounding_boundary():
    assert T == F(0.75)
    # x^500 rounds to +0 below half the smallest denormal, 2^-150: in the reals up to x = 2^-0.3
    assert 500 * np.log2(float(T)) < -150 - 57 and 500 * np.log2(0.8122) < -150 < 500 * np.log2(0.8123)
    x = np.nextafter(T, F(0)).astype(np.float64)                 # the largest float a sure lane can hold
    assert x ** 500 < 2.0 ** -207 and F(x ** 500) == 0 and not np.signbit(F(x ** 500))


def test_clamp_and_the_lane_test_at_the_neighbours_of_T_and_on_specials():
    below, above = np.nextafter(T, F(0)), np.nextafter(T, F(1))
    e = np.array([below, T, above, 0.0, -0.0, -1.0, -np.inf, 1e-45, 1.0, 2.0, np.inf, np.nan, -np.nan], F)
    c = clamp(e)
    assert not np.isnan(c).any() and (c >= 0).all() and (c <= 1).all()
    assert c[-1] == 1 and c[-2] == 1                             # fminf(1, NaN) = 1: a NaN is never sure
    assert not np.signbit(c[4]) or c[4] == 0                     # -0 clamps to a zero
    assert sure(c).tolist() == [True, False, False, True, True, True, True, True, False, False, False, False, False]
    assert not sure(F(np.nan))                                   # (and an unclamped NaN fails the compare too)


def _random_waves(rng, n):
    """clamped e of n waves: most wholly below T, some with one or a few lanes at or above it, NaNs among those"""
    e = rng.uniform(0.0, float(np.nextafter(T, F(0))), (n, 64)).astype(F)
    k = rng.randint(0, 4, n)                                     # 0: untouched
    for w in np.nonzero(k)[0]:
        lanes = rng.choice(64, rng.randint(1, 4), replace=False)
        e[w, lanes] = {1: T, 2: F(rng.uniform(0.75, 1.0)), 3: F(np.nan)}[int(k[w])]
    return e, k


def test_the_guard_never_fires_when_some_lane_is_not_below_T():
    rng = np.random.RandomState(168)
    raw, k = _random_waves(rng, 4000)
    fired = 0
    for w in range(len(raw)):
        lanes = rng.rand(64) < rng.choice([1.0, 0.9, 0.3, 0.05])
        e = clamp(raw[w])
        skips = wave_skips(e, lanes)
        with np.errstate(invalid="ignore"):
            want = bool((e[lanes] < T).all())
        assert skips == want, (w, k[w])
        if skips and lanes.any():
            assert float(e[lanes].max()) < float(T)
            assert (e[lanes].astype(np.float64) ** 500 < 2.0 ** -150).all()
        fired += skips
    assert 0 < fired < len(raw)
    # lanes that are not there do not block the skip and cannot cause one
    e = np.full(64, 0.5, F)
    e[7] = np.nan
    lanes = np.ones(64, bool)
    assert not wave_skips(clamp(e), lanes)
    lanes[7] = False
    assert wave_skips(clamp(e), lanes)
    e[3] = T
    assert not wave_skips(clamp(e), lanes)


def test_the_replays_e_on_a_hand_made_hit():
    # a triangle in the plane z = 0 seen along -z from (0, 0, 2), the light at the eye: at the foot of the perpendicular e = 1,
    # and at x = 2 the angle between the eye and the mirror direction is 2 * atan(1) = 90 degrees
    v = np.array([[-4, -4, 0], [4, -4, 0], [0, 4, 0]], F)
    n = np.array([[0, 0, 1]], F)
    arrays = (v, n, np.array([[0, 1, 2]], np.uint32), np.array([[0, 0, 0]], np.uint32))
    P = np.array([[0, 0, 0], [2, 0, 0], [0.5, 0, 0]], np.float64)
    rays = np.zeros(4, np.dtype([("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4")]))
    hits = np.zeros(4, np.dtype([("t", "<f4"), ("prim", "<u4"), ("beta", "<f4"), ("gamma", "<f4")]))
    hits["prim"][3] = 0xFFFFFFFF
    for i, p in enumerate(P):
        d = (p - (0, 0, 2)) / np.linalg.norm(p - (0, 0, 2))
        rays["dx"][i], rays["dy"][i], rays["dz"][i] = d
        # p = A + beta (B - A) + gamma (C - A)
        hits["beta"][i], hits["gamma"][i] = np.linalg.solve(np.array([[8, 4], [0, 8]], np.float64), p[:2] + 4)
    e, hit = clamped_e(arrays, rays, hits, (0.0, 0.0, 2.0))
    assert hit.tolist() == [True, True, True, False] and np.isnan(e[3])
    assert abs(e[0] - 1) < 1e-6 and abs(e[1]) < 1e-6 and abs(e[2] - np.cos(2 * np.arctan(0.25))) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu

EYE = (0.5, 0.0, 0.5)           # on the quad's normal through its centre, 0.707 away; the quad's edges are 35 degrees off it


def quad_desc(**over):
    """one card of test_frame_uniform_walk.py cut into two triangles (a unit square tilted 45 degrees about y, normal (s, 0, s)), the
    eye on its normal and the light next to the eye: a lane's e is cos(2 theta) for a hit theta off the normal, T at 20.7 degrees"""
    d = dict(models=[], floor=None, objects=_card(0.0, 2), eye=EYE, lookat=(0.0, 0.0, 0.0), up=scenes.UP, fov=50.0,
             light=(0.52, 0.03, 0.5), wattage=4000.0)
    d.update(over)
    return _desc(d)


def _kinds(miro, sc, fu, rays, d, lo=0, hi=None):
    """the replay's kind per wave for the samples lo .. hi of the frame (whole waves), on the kernel's own hit records"""
    hi = fu.n if hi is None else hi
    assert lo % 64 == 0
    hits = fu.d_hits[lo:hi].cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)
    e, hit = clamped_e(sc.arrays(), rays[lo:hi], hits, d["light"])
    return count_kinds(wave_kinds(e, hit))


def _all_three(c, mixed=True):
    assert c["all_below"] > 0 and c["all_above"] > 0 and (c["mixed"] > 0 or not mixed), str(c)


@gpu
def test_one_pixel_per_wave(miro, oracle):
    d = quad_desc()
    sc, fu, ref, rays, _ = _render(miro, oracle, d, 16, 8, 64)
    c = _kinds(miro, sc, fu, rays, d)
    _all_three(c, mixed=False)              # (at 64 samples per pixel a frame may hold no mixed wave; this one's ring of pixels does)
    assert c["mixed"] > 0 and c["no_hit"] > 0, str(c)
    assert float(fu.d_rgb.max()) > 100.0    # the highlight itself is in the picture: e^500 * f2 * wattage near the middle


@gpu
@pytest.mark.parametrize("spp", [4, 1])
def test_tiled_frames(miro, oracle, spp):
    # 64 x 36 in the tiled order: a wave is a block of 4 x 4 or 8 x 8 pixels
    d = quad_desc()
    sc, fu, _, rays, _ = _render(miro, oracle, d, 64, 36, spp, tiled=True)
    _all_three(_kinds(miro, sc, fu, rays, d))


@gpu
def test_background_only(miro, oracle):
    d = quad_desc(lookat=(1.0, 0.0, 1.0))
    sc, fu, _, rays, _ = _render(miro, oracle, d, 16, 8, 64)
    c = _kinds(miro, sc, fu, rays, d)
    assert c["no_hit"] == 128 == sum(c.values()), str(c)
    assert (fu.d_hits[:, 1].view(torch.int32) == -1).all()


@gpu
def test_ragged_last_wave(miro, oracle):
    # 13 x 7 pixels x 16 samples = 1 456 samples in image order: four pixels per wave, the last wave with 48 live lanes
    d = quad_desc()
    sc, fu, _, rays, _ = _render(miro, oracle, d, 13, 7, 16)
    assert fu.n == 1456
    e, hit = clamped_e(sc.arrays(), rays, fu.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1), d["light"])
    k = wave_kinds(e, hit)
    assert len(k) == 23 and len(e[22 * 64:]) == 48
    _all_three(count_kinds(k))
    assert KINDS[k[-1]] != "no_hit"         # the ragged wave takes the guard with its dead lanes outside the mask


@gpu
@pytest.mark.parametrize("mode", ["any_shadow", "no_shadows"])
def test_shadow_forms(miro, oracle, mode):
    d = quad_desc()
    sc, fu, _, rays, _ = _render(miro, oracle, d, 16, 8, 64, any_shadow=mode == "any_shadow", no_shadows=mode == "no_shadows")
    _all_three(_kinds(miro, sc, fu, rays, d), mixed=False)


@gpu
def test_occluded_highlight(miro, oracle):
    # a second card between the quad and the light: samples in its shadow are zeroed after the guard (or powf) has run
    d = quad_desc(objects=_card(0.0, 2) + [("triangle", (0.2, -0.1, 0.25, 0.3, -0.1, 0.15, 0.25, 0.1, 0.2), (0.70710678, 0.0, 0.70710678) * 3)])
    sc, fu, ref, rays, src = _render(miro, oracle, d, 16, 8, 64)
    _all_three(_kinds(miro, sc, fu, rays, d), mixed=False)
    occluded = fu.d_shadow_hits[src][:, 1].view(torch.int32) != -1
    assert occluded.any() and not occluded.all()


@gpu
def test_per_object_materials(miro):
    # The MAT kernels carry the guard too.  The batched shade refuses a scene with a material table: the picture is compared with
    # one level of the recursion (mr_trace_level, which keeps the plain powf) at one sample per pixel, where no summation order
    # can differ.  Image order: a wave is 64 pixels of a row -- rows through the middle hold both kinds of lane, the top rows
    # are wholly below T; a material of infinite shininess takes no highlight, and those lanes leave the mask.
    d = quad_desc()
    sc = miro.Scene(0)
    n = scenes.populate(sc, d)
    mats = [((0.8, 0.2, 0.2), (0, 0, 0), (0, 0, 0), 1.0, 1.0), ((0.2, 0.8, 0.3), (0, 0, 0), (0, 0, 0), float("inf"), 1.0)]
    sc.set_materials(mats, (np.arange(n) % 2).astype(np.uint32))
    sc.build(4)
    for W, H in ((64, 36), (64, 9)):
        fu = mframe.FusedFrame(sc, d, W, H, spp=1, tiled=False, keep_hits=True)
        fu.step()
        ref = mframe.FrameRenderer(sc, d, W, H, spp=1)
        ref.generate()
        ref.render_specular(depth=0, fused=True)
        torch.cuda.synchronize()
        assert float(fu.d_rgb.max()) > 100.0 and np.array_equal(_bits(fu.d_rgb), _bits(ref.d_rgb))
        rays = np.frombuffer(ref.d_rays.cpu().numpy().tobytes(), dtype=np.dtype(
            [("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("tmin", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("tmax", "<f4")]))
        hits = fu.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)
        assert set(hits["prim"][hits["prim"] != 0xFFFFFFFF].tolist()) == {0, 1}
        e, hit = clamped_e(sc.arrays(), rays, hits, d["light"])
        c = count_kinds(wave_kinds(e, hit))
        assert c["all_below"] > 0 and c["mixed"] + c["all_above"] > 0, str(c)


@gpu
def test_256_lane_frame(miro, oracle):
    # 625 x 256 x 64, the smallest frame that takes the 256-lane build (test_frame_large.py); the replay looks at the middle row
    d = quad_desc()
    sc, fu, _, rays, _ = _render(miro, oracle, d, 625, 256, 64, with_oracle=False)
    assert fu.n > 10000000
    lo = 128 * 625 * 64
    _all_three(_kinds(miro, sc, fu, rays, d, lo, lo + 625 * 64))
