"""mr_render_lights_environment -- the fused light-list frame with the environment for rays that miss
(csrc/mr_frame_lights_env.hip): Camera::eyeRay -> Scene::traceScene, which shades a hit as mr_render_lights_surface does and
returns Scene::getEnvironmentMap(ray) for a ray that leaves the scene (Scene.cpp:338-342, 657-688) -> the pixel's mean, in one
launch: the level-0 image of Scene::raytraceImage, background included.

The yardstick everywhere is the batched chain on the same scene, camera, seed and sample order,

    gen_eye_rays[_tiled] -> trace -> hit_surface -> shade_lights_surface(d_ray_rgb) || shade_environment(flags 0, d_ray_rgb)

where a sample's L is the light chain's row where it hit and the environment chain's row where it missed; tests/test_lights.py,
tests/test_procedural.py and tests/test_environment.py hold its parts against the oracle and the restatements.  The comparisons
are EXACT, as in tests/test_frame_lights.py and tests/test_frame_lights_surface.py, whose shapes, scenes, pixel tree and helpers
these tests share: both sides run the same device functions in the same order under -ffp-contract=off."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_budget  # noqa: E402
from test_frame_lights import MISS, SENTINEL, SHAPE_IDS, SHAPES, bits, camera, frame_desc, pixel_tree, same  # noqa: E402
from test_frame_lights_surface import Fused as SurfaceFused  # noqa: E402
from test_frame_lights_surface import scene_of  # noqa: E402

F = np.float32
NAME = "mr_render_lights_environment"
COUNTS0 = (1000, 5, 77, 31, 9)                          # what d_counts holds before a call: the call does not zero it
BG = (0.25, 0.5, 1.0)
ROTATION = (math.pi / 3 + 0.05, math.pi / 8)            # assignment3.cpp:51


def image(seed):
    """a seeded 48 x 24 float image (W >= 24, H <= 4 W) with values in [0, 4): max_intensity matters"""
    return (np.random.default_rng(seed).random((24, 48, 3)) * 4.0).astype(F)


# the environments of these tests: the arguments of Scene.set_environment
ENVS = {"image": dict(pixels=image(168), rotation=ROTATION), "other_image": dict(pixels=image(7), rotation=ROTATION),
        "colour": dict(bg_color=BG), "none": dict()}


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_render_lights_environment_is_exported_declared_and_bound(miro):
    from miro_amd import binding, frame

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return re.search(r"\bmr_status\s+%s\s*\(" % NAME, src) is not None

    assert hasattr(miro.lib(), NAME)
    assert declared("miro_hip_frame.h") and not declared("miro_hip.h") and not declared("miro_hip_surface.h")
    assert NAME in binding.FRAME_SYMBOLS and NAME not in binding.SURFACE_SYMBOLS and NAME not in miro.EXPORTED_SYMBOLS
    assert len(binding.FRAME_SYMBOLS) == len(set(binding.FRAME_SYMBOLS))
    assert getattr(miro.lib(), NAME).restype is C.c_int32
    assert '#include "miro_hip_frame.h"' in open(os.path.join(ROOT, "include", "miro_hip.h")).read()
    assert hasattr(miro.Scene, "render_lights_environment") and hasattr(frame.FusedFrame, "environment_counts")


def test_frame_lights_env_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_frame_lights_env.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer
    waves per SIMD than BOTH its own record (tests/golden/kernel_budget_frame_lights_env.json, written from the build whose GPU
    run of this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.  One kernel per
    traversal variant of with_trace_variant (six) and shadow-ray form (closest hit, any hit): colour or image is a wave-uniform
    branch, not a template argument.  None of them carries a name that tests/test_build_budget.py holds to six waves."""
    cur = kernel_budget.unit_kernels("mr_frame_lights_env")
    assert len(cur) == 6 * 2 and all("frame_lights_env_kernel" in k for k in cur)
    assert not any("frame_kernel" in k or "trace_kernel" in k for k in cur)
    for var in (1818, 826, 267, 43, 88, 73):                   # kTraceExact, ExactObj, Product, ProductObj, Vote, VoteProduct
        for any_hit in (0, 1):
            assert sum("ILi%dELb%dEE" % (var, any_hit) in k for k in cur) == 1, (var, any_hit)
    assert not any(v["dynamic_stack"] for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_frame_lights_env.json", also_main=True)


def test_argument_errors_come_before_the_scene_and_the_device(miro):
    """The table of tests/test_frame_lights_surface.py against this call: every MR_ERR_INVALID case on a host_only one-triangle
    scene is answered from the arguments alone, under this call's name, before any device or state message.  Then MR_ERR_STATE
    for that scene, for an unbuilt one and for scenes without lights."""
    from miro_amd import binding
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.set_environment(**ENVS["image"])
    s.build(4, host_only=True)
    rgb, hits = C.c_void_p(1024), C.c_void_p(2048)

    def call(fd, scene=s.h, d_rgb=rgb, d_hits=hits, d_sample=None, d_color=None, d_normal=None, d_counts=None):
        st = L.mr_render_lights_environment(scene, C.byref(fd) if fd is not None else None, d_rgb, d_hits, d_sample, d_color, d_normal, d_counts,
                                            None)
        return st, L.mr_last_error()

    ok = frame_desc(binding)
    invalid = [
        ("NULL", call(ok, scene=None)), ("NULL", call(None)), ("NULL", call(ok, d_rgb=None)),
        ("empty", call(frame_desc(binding, W=0))),
        ("spp", call(frame_desc(binding, spp=0))), ("spp", call(frame_desc(binding, spp=3))), ("spp", call(frame_desc(binding, spp=128))),
        ("band", call(frame_desc(binding, bands=(2, 3, 3)))), ("band", call(frame_desc(binding, bands=(0, 1, 2)))),
        ("rows", call(frame_desc(binding, y1=9))), ("rows", call(frame_desc(binding, y0=5, y1=4))),
        ("too large", call(frame_desc(binding, W=65536, H=65536))),
        ("flags", call(frame_desc(binding, flags=binding.MR_FRAME_NO_SHADOWS))), ("flags", call(frame_desc(binding, flags=binding.MR_MATH_FAST))),
        ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY | (1 << 30)))),
        ("aligned", call(ok, d_hits=C.c_void_p(2048 + 8))), ("aligned", call(ok, d_counts=C.c_void_p(4100))),
        ("aligned", call(ok, d_rgb=C.c_void_p(1026))), ("aligned", call(ok, d_sample=C.c_void_p(4098))),
        ("aligned", call(ok, d_color=C.c_void_p(4098))), ("aligned", call(ok, d_normal=C.c_void_p(4097))),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and NAME.encode() in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    st, msg = call(ok)                                                            # then the scene's state: never a CPU path
    assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg
    unbuilt = miro.Scene()
    unbuilt.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    st, msg = call(ok, scene=unbuilt.h)                                           # unbuilt, and without lights
    assert st == binding.MR_ERR_STATE and b"mr_bvh_build" in msg, msg
    st, msg = call(frame_desc(binding, spp=5), scene=unbuilt.h)
    assert st == binding.MR_ERR_INVALID and b"spp" in msg and NAME.encode() in msg  # still the arguments first
    s.set_lights([])                                                              # host_only without lights: still the scene's state
    st, msg = call(ok)
    assert st == binding.MR_ERR_STATE and b"HIP device" not in msg, msg
    assert s.info().n_triangles == 1                                              # the refused calls left the scene alone


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
_CHAINS, _FUSED = {}, {}


def use(miro, name, env):
    """the test scene `name` (tests/test_frame_lights_surface.py builds it once per session) with its lights and the environment
    ENVS[env] set: (scene, description, lights)"""
    scene, desc, lights = scene_of(miro, name)
    scene.set_lights(lights)
    scene.set_environment(**ENVS[env])
    return scene, desc, lights


class Chain:
    """The batched chain of one frame, resident on the device: hits, the surface pass's colour and normal (rows of rays that
    missed keep the sentinel) and its count of undefined lookups, the light chain's and the environment chain's per-ray values,
    the environment's two counters, per-sample L = the light chain's row where the ray hit and the environment chain's where it
    missed, and the pixels of its pairwise tree in image order.  At 1 spp also `added`: the pixels that both batched calls ADD
    into (every pixel receives one addition to 0 from each)."""

    def __init__(self, scene, desc, W, H, spp, tiled, flags=0):
        import torch
        from miro_amd import binding
        self.n = n = W * H * spp
        f32 = dict(dtype=torch.float32, device="cuda")
        rays = torch.empty((n, 8), **f32)
        self.hits = torch.empty((n, 4), **f32)
        self.color, self.normal, self.lights_rgb, self.env_rgb = (torch.full((n, 3), SENTINEL, **f32) for _ in range(4))
        undefined = torch.zeros(1, dtype=torch.int64, device="cuda")
        env_counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        scene.gen_eye_rays(camera(desc), W, H, rays, spp=spp, jitter=spp > 1, seed=168, tiled=tiled)
        scene.trace_device(rays, n, self.hits, flags & (binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT))
        scene.hit_surface(rays, self.hits, n, self.color, self.normal, d_counts=undefined)
        scene.shade_lights_surface(rays, self.hits, self.color, self.normal, n, None, spp=spp, flags=flags, d_ray_rgb=self.lights_rgb)
        scene.shade_environment(rays, self.hits, n, None, spp=spp, flags=0, d_ray_rgb=self.env_rgb, d_counts=env_counts)
        self.added = None
        if spp == 1 and not tiled:
            self.added = torch.zeros((W * H, 3), **f32)
            scene.shade_lights_surface(rays, self.hits, self.color, self.normal, n, self.added, spp=1, flags=flags)
            scene.shade_environment(rays, self.hits, n, self.added, spp=1, flags=0)
        torch.cuda.synchronize()
        self.hit_rows = self.hits[:, 1].contiguous().view(torch.int32) != -1
        self.ray_rgb = torch.where(self.hit_rows[:, None], self.lights_rgb, self.env_rgb)
        slots = pixel_tree(self.ray_rgb.view(W * H, spp, 3), spp)
        self.rgb = slots
        if tiled:                                       # slot p of the tiled order is pixel tile_pixel_map[p]
            m = torch.from_numpy(binding.tile_pixel_map(W, H, spp).astype(np.int64)).cuda()
            self.rgb = torch.empty_like(slots)
            self.rgb[m] = slots
        self.n_hits = int(self.hit_rows.sum().item())
        self.undefined = int(undefined.item())
        self.env_counts = tuple(int(c) for c in env_counts.cpu().numpy())


def chain_of(miro, name, env, W, H, spp, tiled, flags=0):
    key = (name, env, W, H, spp, tiled, flags)
    if key not in _CHAINS:
        scene, desc, _ = use(miro, name, env)
        _CHAINS[key] = Chain(scene, desc, W, H, spp, tiled, flags)
    return _CHAINS[key]


class Fused:
    """One mr_render_lights_environment call on the scene as it is set, with every optional output, each buffer one sentinel row
    longer than the contract says"""

    def __init__(self, scene, desc, W, H, spp, tiled, flags=0, y0=0, y1=None, bands=None, rows=None, stream=None):
        import torch
        rows = (H if y1 is None else y1) - y0 if rows is None else rows
        self.n, self.n_pixels = rows * W * spp, rows * W
        f32 = dict(dtype=torch.float32, device="cuda")
        self.rgb = torch.full((self.n_pixels + 1, 3), SENTINEL, **f32)
        self.hits = torch.full((self.n + 1, 4), SENTINEL, **f32)
        self.sample_rgb, self.color, self.normal = (torch.full((self.n + 1, 3), SENTINEL, **f32) for _ in range(3))
        self.counts = torch.tensor(COUNTS0 + (4242,), dtype=torch.int64, device="cuda")       # a sixth word: never touched
        scene.render_lights_environment(camera(desc), W, H, self.rgb, y0=y0, y1=y1, bands=bands, spp=spp, jitter=spp > 1, seed=168,
                                        tiled=tiled, flags=flags, d_hits=self.hits, d_sample_rgb=self.sample_rgb,
                                        d_sample_color=self.color, d_sample_normal=self.normal, d_counts=self.counts, stream=stream)
        torch.cuda.synchronize()
        for t, k in ((self.rgb, self.n_pixels), (self.hits, self.n), (self.sample_rgb, self.n), (self.color, self.n), (self.normal, self.n)):
            assert bool((t[k] == SENTINEL).all()), "written beyond the end"
        c = self.counts.cpu().numpy()
        assert int(c[5]) == 4242, "written beyond the fifth counter"
        self.counted = tuple(int(v) - v0 for v, v0 in zip(c, COUNTS0))


def fused_of(miro, name, env, W, H, spp, tiled, flags=0):
    key = (name, env, W, H, spp, tiled, flags)
    if key not in _FUSED:
        scene, desc, _ = use(miro, name, env)
        _FUSED[key] = Fused(scene, desc, W, H, spp, tiled, flags)
    return _FUSED[key]


def assert_frame_is_the_chain(fu, ch, n_lights):
    """hit records on their bits; the surface pass's colour and normal, the rows of misses untouched; per-sample L, the light
    chain's where the ray hit and the environment chain's where it missed; pixels against the chain's tree; all five counter
    deltas -- nothing left out.  Not vacuous: the frame has a hit and a miss, by the chain's own hit records."""
    n_miss = ch.n - ch.n_hits
    assert fu.n == ch.n and ch.n_hits > 0 and n_miss > 0 and float(ch.rgb.max()) > 0
    assert np.array_equal(bits(fu.hits[:fu.n]), bits(ch.hits))
    assert same(fu.color[:fu.n][ch.hit_rows], ch.color[ch.hit_rows]) and same(fu.normal[:fu.n][ch.hit_rows], ch.normal[ch.hit_rows])
    assert bool((fu.color[:fu.n][~ch.hit_rows] == SENTINEL).all()) and bool((fu.normal[:fu.n][~ch.hit_rows] == SENTINEL).all())
    assert bool((ch.color[ch.hit_rows] != SENTINEL).any())
    assert bool((ch.ray_rgb != SENTINEL).all()) and bool((ch.env_rgb[ch.hit_rows] == 0).all())
    assert same(fu.sample_rgb[:fu.n], ch.ray_rgb)
    assert same(fu.rgb[:fu.n_pixels], ch.rgb)
    assert ch.env_counts[0] == n_miss
    assert fu.counted == (ch.n, ch.n_hits * n_lights, ch.undefined, ch.env_counts[0], ch.env_counts[1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", ["teapot_textured", "flower", "teapot"])
def test_frame_is_the_batched_chain_bit_for_bit(miro, name, shape):
    """The seeded image, rotated as assignment3.cpp rotates its own, behind the textured teapot, makeTestPetalScene and the
    untextured teapot (no texture table: the plain arm).  Every view has hits and misses at every shape (the oracle counts, at
    37 x 19 x 1 / x 4 / 5 x 1 x 64: 553 of 703, 2215 of 2812 and 93 of 320 samples hit the teapot; 113, 449 and 18 the flower --
    the one row of 5 x 1 x 64 crosses the silhouette); assert_frame_is_the_chain asserts it on the chain's own records.  The
    misses are not 0: the frame differs from mr_render_lights_surface's in the samples that missed and in no other."""
    W, H, spp, tiled = shape
    scene, desc, lights = use(miro, name, "image")
    fu, ch = fused_of(miro, name, "image", W, H, spp, tiled), chain_of(miro, name, "image", W, H, spp, tiled)
    print("%s %s: %d samples, %d hits, %d lights, max %.4g, %d undefined, environment %s" % (name, shape, ch.n, ch.n_hits, len(lights),
                                                                                              float(ch.rgb.max()), ch.undefined, ch.env_counts))
    assert_frame_is_the_chain(fu, ch, len(lights))
    assert float(ch.env_rgb[~ch.hit_rows].max()) > 0 and bool((ch.env_rgb[~ch.hit_rows] >= 0).all())
    assert bool((ch.env_rgb[~ch.hit_rows] <= 1).all())                            # tonemapValue clamps at 1
    if ch.added is not None:                            # 1 spp: the two batched calls add into the pixels, one addition each
        assert same(fu.rgb[:fu.n_pixels], ch.added)
    plain = SurfaceFused(scene, desc, lights, W, H, spp, tiled)
    assert np.array_equal(bits(plain.hits), bits(fu.hits[:, :4]))
    assert same(plain.sample_rgb[:fu.n][ch.hit_rows], fu.sample_rgb[:fu.n][ch.hit_rows])
    assert bool((plain.sample_rgb[:fu.n][~ch.hit_rows] == 0).all()) and not same(plain.sample_rgb, fu.sample_rgb)
    assert plain.counted == fu.counted[:3]
    if tiled:                                           # the sample order changes, the picture does not
        assert same(fu.rgb, fused_of(miro, name, "image", W, H, spp, False).rgb)
        assert not np.array_equal(bits(fu.hits), bits(fused_of(miro, name, "image", W, H, spp, False).hits))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["teapot_textured", "flower"])
def test_colour_only(miro, name):
    """bg_color = (0.25, 0.5, 1.0) and no image: every sample that missed has exactly that L, every sample that hit has
    mr_render_lights_surface's, no lookup is made (d_counts[4] stays), and the frame is still the chain's."""
    import torch
    W, H, spp = 37, 19, 4
    scene, desc, lights = use(miro, name, "colour")
    fu, ch = fused_of(miro, name, "colour", W, H, spp, False), chain_of(miro, name, "colour", W, H, spp, False)
    assert_frame_is_the_chain(fu, ch, len(lights))
    bg = torch.tensor(BG, dtype=torch.float32, device="cuda")
    assert bool((fu.sample_rgb[:fu.n][~ch.hit_rows] == bg).all())
    plain = SurfaceFused(scene, desc, lights, W, H, spp, False)
    assert same(fu.sample_rgb[:fu.n][ch.hit_rows], plain.sample_rgb[:fu.n][ch.hit_rows])
    assert fu.counted[3] == ch.n - ch.n_hits and fu.counted[4] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_without_an_environment_it_is_mr_render_lights_surface(miro, shape):
    """No environment set (bg_color 0, no image) on the textured teapot: all five buffers and the counters [0..2] equal
    mr_render_lights_surface's bit for bit; [3] is the miss count of the hit records, [4] is 0."""
    W, H, spp, tiled = shape
    scene, desc, lights = use(miro, "teapot_textured", "none")
    fu = fused_of(miro, "teapot_textured", "none", W, H, spp, tiled)
    plain = SurfaceFused(scene, desc, lights, W, H, spp, tiled)
    assert float(plain.rgb[:plain.n_pixels].max()) > 0
    for f in ("rgb", "sample_rgb", "color", "normal"):
        assert same(getattr(fu, f), getattr(plain, f)), f
    assert np.array_equal(bits(fu.hits), bits(plain.hits))
    misses = int((bits(plain.hits[:plain.n])[:, 1] == MISS).sum())
    assert 0 < misses < fu.n and fu.counted == plain.counted + (misses, 0)


@pytest.mark.gpu
def test_a_closed_room_has_no_misses(miro):
    """The mixed room is closed: nothing misses, d_counts[3] stays, and the frame is mr_render_lights_surface's with an image,
    with a colour and with nothing set -- all the same bits."""
    W, H, spp = 37, 19, 4
    scene, desc, lights = use(miro, "mixed", "none")
    plain = SurfaceFused(scene, desc, lights, W, H, spp, False)
    assert float(plain.rgb[:plain.n_pixels].max()) > 0 and not bool((bits(plain.hits[:plain.n])[:, 1] == MISS).any())
    for env in ("none", "image", "colour"):
        fu = fused_of(miro, "mixed", env, W, H, spp, False)
        for f in ("rgb", "sample_rgb", "color", "normal"):
            assert same(getattr(fu, f), getattr(plain, f)), (env, f)
        assert np.array_equal(bits(fu.hits), bits(plain.hits)) and fu.counted == plain.counted + (0, 0), env


@pytest.mark.gpu
def test_row_windows_and_interleaved_bands(miro):
    """The textured teapot before the image at 37 x 19 x 4.  Rows [5, 12) are those rows of the full frame; the two ranks of
    band_rows = 3, world = 2 (H = 19: a ragged last band) cover every row once and, put back with band_locate, are the full
    frame -- pixels, hit records, per-sample colour, normal and L -- and their five counters sum to its."""
    W, H, spp = 37, 19, 4
    scene, desc, lights = use(miro, "teapot_textured", "image")
    full, ch = fused_of(miro, "teapot_textured", "image", W, H, spp, False), chain_of(miro, "teapot_textured", "image", W, H, spp, False)
    assert_frame_is_the_chain(full, ch, len(lights))
    scene, desc, lights = use(miro, "teapot_textured", "image")
    per_sample = ("sample_rgb", "color", "normal")
    win = Fused(scene, desc, W, H, spp, False, y0=5, y1=12)
    assert same(win.rgb[:7 * W], full.rgb[5 * W:12 * W])
    assert np.array_equal(bits(win.hits[:win.n]), bits(full.hits[5 * W * spp:12 * W * spp]))
    for f in per_sample:
        assert same(getattr(win, f)[:win.n], getattr(full, f)[5 * W * spp:12 * W * spp]), f
    prim = bits(ch.hits)[5 * W * spp:12 * W * spp, 1]
    n_hit, n_miss = int((prim != MISS).sum()), int((prim == MISS).sum())
    assert n_hit > 0 and n_miss > 0 and win.counted == (7 * W * spp, n_hit * len(lights), 0, n_miss, 0)
    band, world = 3, 2
    shards = []
    for r in range(world):
        rows = miro.band_rows_of(H, band, r, world)
        shards.append(Fused(scene, desc, W, H, spp, False, bands=(band, r, world), rows=rows))
    assert [s.n_pixels // W for s in shards] == [10, 9]            # seven bands; the last one, row 18 alone, is rank 0's fourth
    seen = set()
    for y in range(H):
        r, j = miro.band_locate(H, band, world, y)
        seen.add((r, j))
        sh = shards[r]
        assert same(sh.rgb[j * W:(j + 1) * W], full.rgb[y * W:(y + 1) * W]), y
        assert np.array_equal(bits(sh.hits[j * W * spp:(j + 1) * W * spp]), bits(full.hits[y * W * spp:(y + 1) * W * spp])), y
        for f in per_sample:
            assert same(getattr(sh, f)[j * W * spp:(j + 1) * W * spp], getattr(full, f)[y * W * spp:(y + 1) * W * spp]), (y, f)
    assert len(seen) == H == sum(s.n_pixels // W for s in shards)
    assert tuple(sum(s.counted[k] for s in shards) for k in range(5)) == full.counted
    empty = Fused(scene, desc, W, H, spp, False, y0=7, y1=7)
    assert empty.counted == (0, 0, 0, 0, 0)
    for t in (empty.rgb, empty.hits, empty.sample_rgb, empty.color, empty.normal):
        assert bool((t == SENTINEL).all())


@pytest.mark.gpu
def test_traversal_flags(miro):
    """MR_TRACE_ANY (shadow rays only; the textured teapot is opaque), MR_MATH_PRODUCT and MR_TRACE_INCOHERENT, each against the
    chain run with the same flags.  The environment's value of a sample that misses with and without the flag is the same
    bits: the flags change the traversal, not the eye ray."""
    from miro_amd import binding
    W, H, spp = 37, 19, 4
    name = "teapot_textured"
    base, base_chain = fused_of(miro, name, "image", W, H, spp, False), chain_of(miro, name, "image", W, H, spp, False)
    for flags in (binding.MR_TRACE_ANY, binding.MR_MATH_PRODUCT, binding.MR_TRACE_INCOHERENT):
        fu, ch = fused_of(miro, name, "image", W, H, spp, False, flags), chain_of(miro, name, "image", W, H, spp, False, flags)
        assert_frame_is_the_chain(fu, ch, 4)
        both = ~ch.hit_rows & ~base_chain.hit_rows
        assert int(both.sum()) > 0 and same(fu.sample_rgb[:fu.n][both], base.sample_rgb[:fu.n][both])
    any_hit = fused_of(miro, name, "image", W, H, spp, False, binding.MR_TRACE_ANY)
    assert same(any_hit.rgb, base.rgb) and np.array_equal(bits(any_hit.hits), bits(base.hits)) and any_hit.counted == base.counted
    scene, desc, lights = use(miro, "mixed", "image")
    with pytest.raises(miro.MiroError) as e:
        Fused(scene, desc, W, H, spp, False, flags=binding.MR_TRACE_ANY)
    assert e.value.status == binding.MR_ERR_STATE and "refractive" in str(e.value) and NAME in str(e.value)


@pytest.mark.gpu
def test_grid_stride_loop_and_a_partial_last_workgroup(miro):
    """64 spp on the untextured teapot with two lights before the image, as tests/test_frame_lights.py reaches this case:
    385 x 351 x 64 = 8 648 640 samples are 33 783 workgroups of 256 and three quarters of one more -- above the grid cap of
    32 768, so the first workgroups take a second chunk, and the last chunk's fourth wave lies past the end of the window (its
    lanes are not misses).  Compared on the device."""
    import torch
    W, H, spp = 385, 351, 64
    n = W * H * spp
    assert n % 256 == 192 and n // 256 + 1 > 32768
    scene, desc, lights = use(miro, "teapot", "image")
    scene.set_lights(lights[:2])
    ch = Chain(scene, desc, W, H, spp, False)
    fu = Fused(scene, desc, W, H, spp, False)
    scene.set_lights(lights)
    assert ch.n_hits > 0 and ch.n - ch.n_hits > 0 and float(ch.rgb.max()) > 0
    assert torch.equal(fu.hits[:n].view(torch.int32), ch.hits.view(torch.int32))
    assert same(fu.sample_rgb[:n], ch.ray_rgb)
    assert same(fu.rgb[:W * H], ch.rgb)
    assert fu.counted == (n, ch.n_hits * 2, 0, n - ch.n_hits, ch.env_counts[1]) and ch.env_counts[0] == n - ch.n_hits
    del ch, fu
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_replays_from_a_captured_graph(miro):
    """After one warm call (which uploads the image and the texture table: allocations and copies that may not lie inside a
    capture) the 37 x 19 x 4 frame of the textured teapot is captured into a torch.cuda.graph and replayed twice, d_rgb filled
    with a sentinel before each replay: equal to the direct launch, and the five counters advance by two steps' worth."""
    import torch
    W, H, spp = 37, 19, 4
    name = "teapot_textured"
    first = fused_of(miro, name, "image", W, H, spp, False)
    assert_frame_is_the_chain(first, chain_of(miro, name, "image", W, H, spp, False), 4)
    scene, desc, lights = use(miro, name, "image")
    cam = camera(desc)
    out = torch.full((W * H, 3), SENTINEL, dtype=torch.float32, device="cuda")
    counts = torch.zeros(5, dtype=torch.int64, device="cuda")
    scene.render_lights_environment(cam, W, H, out, spp=spp, jitter=True)         # warm: image and table are on the device
    torch.cuda.synchronize()
    assert same(out, first.rgb[:W * H])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        scene.render_lights_environment(cam, W, H, out, spp=spp, jitter=True, d_counts=counts, stream=torch.cuda.current_stream())
    counts.zero_()
    for _ in range(2):
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(out, first.rgb[:W * H])
    assert tuple(counts.tolist()) == tuple(2 * c for c in first.counted) and first.counted[3] > 0


@pytest.mark.gpu
def test_a_changed_environment_shows_in_the_next_call(miro):
    """The image replaced by another one, then cleared: each call renders the environment as it is set at that call -- the
    chain's frame for it -- and the samples that hit never change."""
    W, H, spp = 37, 19, 4
    name = "teapot_textured"
    scene, desc, lights = use(miro, name, "image")
    one = Fused(scene, desc, W, H, spp, False)
    assert_frame_is_the_chain(one, chain_of(miro, name, "image", W, H, spp, False), 4)
    scene, desc, lights = use(miro, name, "other_image")
    two = Fused(scene, desc, W, H, spp, False)
    ch = chain_of(miro, name, "other_image", W, H, spp, False)
    assert_frame_is_the_chain(two, ch, 4)
    miss = ~ch.hit_rows
    assert not same(one.sample_rgb[:one.n][miss], two.sample_rgb[:two.n][miss]) and not same(one.rgb, two.rgb)
    assert same(one.sample_rgb[:one.n][~miss], two.sample_rgb[:two.n][~miss])
    scene.clear_environment()
    three = Fused(scene, desc, W, H, spp, False)
    assert bool((three.sample_rgb[:three.n][miss] == 0).all()) and same(one.sample_rgb[:one.n][~miss], three.sample_rgb[:three.n][~miss])
    assert same(three.rgb, SurfaceFused(scene, desc, lights, W, H, spp, False).rgb) and three.counted[3:] == (int(miss.sum()), 0)
    scene, desc, lights = use(miro, name, "image")                                 # and back again
    assert same(Fused(scene, desc, W, H, spp, False).rgb, one.rgb)


@pytest.mark.gpu
def test_fused_frame_with_an_environment(miro):
    """FusedFrame(lights=..., environment=True) renders with the scene's environment as it is set, environment={...} sets it
    first: both fill d_rgb and d_hits as the direct render_lights_environment call does, with a five-word counter tensor, and
    environment_counts() is (misses, undefined lookups).  environment=None is today's frame -- mr_render_lights_surface's
    pixels, three counters -- whatever the scene's environment is; without `lights` an environment is a ValueError."""
    import torch
    from miro_amd import frame
    W, H, spp = 37, 19, 4
    name = "teapot_textured"
    want, ch = fused_of(miro, name, "image", W, H, spp, True), chain_of(miro, name, "image", W, H, spp, True)
    assert_frame_is_the_chain(want, ch, 4)
    scene, desc, lights = use(miro, name, "image")
    ff = frame.FusedFrame(scene, desc, W, H, spp=spp, keep_hits=True, lights=lights, environment=True)
    assert ff.tiled and ff.jitter and ff.d_counts.numel() == 5
    ff.step()
    torch.cuda.synchronize()
    assert same(ff.d_rgb, want.rgb[:W * H]) and np.array_equal(bits(ff.d_hits), bits(want.hits[:ff.n]))
    assert ff.ray_counts() == (ch.n, ch.n_hits * 4) and ff.undefined_lookups() == 0
    assert ff.environment_counts() == (ch.n - ch.n_hits, ch.env_counts[1]) == want.counted[3:]
    ff.step()
    assert ff.environment_counts(steps=2) == want.counted[3:]
    scene.clear_environment()
    ff = frame.FusedFrame(scene, desc, W, H, spp=spp, lights=lights, environment=dict(ENVS["image"]))
    ff.step()
    torch.cuda.synchronize()
    assert same(ff.d_rgb, want.rgb[:W * H]) and ff.environment_counts() == want.counted[3:]
    plain = frame.FusedFrame(scene, desc, W, H, spp=spp, lights=lights)            # the image is still set: not applied
    assert plain.d_counts.numel() == 3 and plain.environment_counts() == (0, 0)
    plain.step()
    torch.cuda.synchronize()
    assert same(plain.d_rgb, SurfaceFused(scene, desc, lights, W, H, spp, True).rgb[:W * H]) and not same(plain.d_rgb, ff.d_rgb)
    for bad in (True, dict(bg_color=BG)):
        with pytest.raises(ValueError):
            frame.FusedFrame(scene, desc, W, H, spp=spp, environment=bad)


@pytest.mark.gpu
def test_scene_state_errors(miro):
    """MR_ERR_STATE for a scene without lights, under this call's name; nothing is written."""
    import torch
    from miro_amd import binding
    scene, desc, lights = use(miro, "teapot_textured", "image")
    rgb = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    scene.set_lights([])
    with pytest.raises(miro.MiroError) as e:
        scene.render_lights_environment(camera(desc), 8, 8, rgb)
    assert e.value.status == binding.MR_ERR_STATE and "no lights" in str(e.value) and NAME in str(e.value)
    scene.set_lights(lights)
    torch.cuda.synchronize()
    assert float(rgb.abs().max()) == 0.0
