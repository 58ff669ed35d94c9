"""mr_render_lights_surface -- the fused direct-light frame over the scene's light list on ANY scene, textured ones included
(csrc/mr_frame_lights_surface.hip): Camera::eyeRay -> Scene::trace with its bump-mapped normal -> diffuseColor of a
TexturedPhong -> Phong::shade's loop over Scene::lights() -> the pixel's mean, in one launch.

The yardstick everywhere is the batched chain on the same scene, camera, seed and sample order,

    gen_eye_rays[_tiled] -> trace -> hit_surface -> shade_lights_surface(..., d_ray_rgb=...)

which tests/test_procedural.py, tests/test_solid_textures.py and tests/test_lights.py hold against the oracle and the
restatements.  The comparisons are EXACT, as in tests/test_frame_lights.py, whose shapes, pixel tree and helpers these tests
share: both sides run the same device functions in the same order under -ffp-contract=off."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_budget  # noqa: E402
from test_frame_lights import MISS, SENTINEL, SHAPE_IDS, SHAPES, TEAPOT_LIGHTS, bits, camera, frame_desc, pixel_tree, same  # noqa: E402

F = np.float32
NAME = "mr_render_lights_surface"
NONE = 0xFFFFFFFF
INF = float("inf")
COUNTS0 = (1000, 5, 77)                                 # what d_counts holds before a call: the call does not zero it


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_render_lights_surface_is_exported_declared_and_bound(miro):
    from miro_amd import binding, frame

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return re.search(r"\bmr_status\s+%s\s*\(" % NAME, src) is not None

    assert hasattr(miro.lib(), NAME) and NAME in binding.SURFACE_SYMBOLS and NAME not in miro.EXPORTED_SYMBOLS
    assert declared("miro_hip_surface.h") and not declared("miro_hip.h")
    assert len(miro.EXPORTED_SYMBOLS) == len(set(miro.EXPORTED_SYMBOLS)) == 69
    assert len(binding.SURFACE_SYMBOLS) == len(set(binding.SURFACE_SYMBOLS)) == 9
    assert hasattr(miro.Scene, "render_lights_surface") and hasattr(frame.FusedFrame, "undefined_lookups")


def test_frame_lights_surface_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_frame_lights_surface.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer
    waves per SIMD than BOTH its own record (tests/golden/kernel_budget_frame_lights_surface.json, written from the build whose
    GPU run of this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.  One kernel per
    traversal variant of with_trace_variant (six) and shadow-ray form (closest hit, any hit); none of them carries a name that
    tests/test_build_budget.py holds to six waves."""
    cur = kernel_budget.unit_kernels("mr_frame_lights_surface")
    assert len(cur) == 6 * 2 and all("frame_lights_surface_kernel" in k for k in cur)
    assert not any("frame_kernel" in k or "trace_kernel" in k for k in cur)
    for var in (1818, 826, 267, 43, 88, 73):                   # kTraceExact, ExactObj, Product, ProductObj, Vote, VoteProduct
        for any_hit in (0, 1):
            assert sum("ILi%dELb%dEE" % (var, any_hit) in k for k in cur) == 1, (var, any_hit)
    assert not any(v["dynamic_stack"] for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_frame_lights_surface.json", also_main=True)


def test_argument_errors_come_before_the_scene_and_the_device(miro):
    """Every MR_ERR_INVALID case on a host_only one-triangle scene: answered from the arguments alone, before any device call,
    so "no HIP device" and "host_only" may not be what comes back.  Then MR_ERR_STATE for that scene and for an unbuilt one."""
    from miro_amd import binding
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.build(4, host_only=True)
    rgb, hits = C.c_void_p(1024), C.c_void_p(2048)

    def call(fd, scene=s.h, d_rgb=rgb, d_hits=hits, d_sample=None, d_color=None, d_normal=None, d_counts=None):
        st = L.mr_render_lights_surface(scene, C.byref(fd) if fd is not None else None, d_rgb, d_hits, d_sample, d_color, d_normal, d_counts, None)
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
    st, msg = call(ok, scene=unbuilt.h)
    assert st == binding.MR_ERR_STATE and b"mr_bvh_build" in msg, msg
    st, msg = call(frame_desc(binding, spp=5), scene=unbuilt.h)
    assert st == binding.MR_ERR_INVALID and b"spp" in msg                          # still the arguments first
    assert s.info().n_triangles == 1                                              # the refused calls left the scene alone


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
_SCENES, _CHAINS, _FUSED, _PLAIN = {}, {}, {}, {}
LEAF_BEYOND = 1e10                   # a LEAF's noise coordinates are P.xy * scale: on the wall x = 2 beyond 2^30 (mr_noise.h)


def teapot_textured(miro):
    """The teapot and its floor triangle, triangles only: material 0, a slightly glossy LEAF (a UVW kind, looked up at the hit
    point itself), on the teapot; material 1, a CHECKER over texture coordinates 0 ... 8, on the floor triangle, whose normal
    (0, 400, 0) has the positive largest component Triangle::toUVCoordinates asks for."""
    from miro_amd import scenes
    desc = scenes.SCENES["teapot"]
    s = miro.Scene(0)
    scenes.populate(s, desc)
    s.build(4)
    n = s.info().n_triangles
    tidx = np.full((n, 3), NONE, np.uint32)
    tidx[n - 1] = (0, 1, 2)
    s.set_texcoords(np.array([[0, 0], [4, 8], [8, 0]], F), tidx)
    white, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    materials, prim_material = [(white, (0.2, 0.2, 0.2), zero, 40.0, 1.0), (white, zero, zero, INF, 1.0)], [0] * (n - 1) + [1]
    s.set_materials(materials, prim_material)
    textures = [dict(leaf=2.0), dict(color1=(0.9, 0.8, 0.7), color2=(0.2, 0.3, 0.5), scale=1.0)]
    s.set_textures(textures, [0, 1])
    return s, dict(desc, materials=materials, prim_material=prim_material, textures=textures, material_texture=[0, 1])


def scene_of(miro, name):
    """(scene, description, lights) of a test scene, built once per session"""
    from miro_amd import scenes
    if name not in _SCENES:
        two = scenes.SCENES["photon_room_two_lights"]["lights"]
        if name == "teapot_textured":
            s, desc = teapot_textured(miro)
            lights = TEAPOT_LIGHTS
        elif name == "teapot":
            s, desc, lights = miro.Scene(0), scenes.SCENES["teapot"], TEAPOT_LIGHTS
            scenes.populate(s, desc)
            s.build(4)
        elif name == "flower":
            s = miro.Scene(0)
            desc = scenes.flower_setup(s)
            lights = desc["lights"]
        else:
            s = miro.Scene(0)
            desc = {"mixed": scenes.photon_room_mixed, "stone": scenes.photon_room_stone, "beyond": scenes.photon_room_mixed}[name]()
            if name == "beyond":
                desc = dict(desc, textures=[dict(leaf=LEAF_BEYOND) if "leaf" in t else t for t in desc["textures"]])
            scenes.textured_room_setup(s, desc)
            lights = two
        s.set_lights(lights)
        _SCENES[name] = (s, desc, lights)
    return _SCENES[name]


class Chain:
    """The batched chain of one frame, resident on the device: hits, the surface pass's colour and normal (rows of rays that
    missed keep the sentinel), its count of undefined lookups, per-sample L, and the pixels of its pairwise tree in image order"""

    def __init__(self, scene, desc, lights, W, H, spp, tiled, flags=0):
        import torch
        from miro_amd import binding
        scene.set_lights(lights)
        self.n = n = W * H * spp
        f32 = dict(dtype=torch.float32, device="cuda")
        rays = torch.empty((n, 8), **f32)
        self.hits = torch.empty((n, 4), **f32)
        self.color, self.normal, self.ray_rgb = (torch.full((n, 3), SENTINEL, **f32) for _ in range(3))
        undefined = torch.zeros(1, dtype=torch.int64, device="cuda")
        scene.gen_eye_rays(camera(desc), W, H, rays, spp=spp, jitter=spp > 1, seed=168, tiled=tiled)
        scene.trace_device(rays, n, self.hits, flags & (binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT))
        scene.hit_surface(rays, self.hits, n, self.color, self.normal, d_counts=undefined)
        scene.shade_lights_surface(rays, self.hits, self.color, self.normal, n, None, spp=spp, flags=flags, d_ray_rgb=self.ray_rgb)
        torch.cuda.synchronize()
        slots = pixel_tree(self.ray_rgb.view(W * H, spp, 3), spp)
        self.rgb = slots
        if tiled:                                       # slot p of the tiled order is pixel tile_pixel_map[p]
            m = torch.from_numpy(binding.tile_pixel_map(W, H, spp).astype(np.int64)).cuda()
            self.rgb = torch.empty_like(slots)
            self.rgb[m] = slots
        self.hit_rows = self.hits[:, 1].contiguous().view(torch.int32) != -1
        self.n_hits = int(self.hit_rows.sum().item())
        self.undefined = int(undefined.item())


def chain_of(miro, name, W, H, spp, tiled, flags=0):
    key = (name, W, H, spp, tiled, flags)
    if key not in _CHAINS:
        scene, desc, lights = scene_of(miro, name)
        _CHAINS[key] = Chain(scene, desc, lights, W, H, spp, tiled, flags)
    return _CHAINS[key]


class Fused:
    """One mr_render_lights_surface call with every optional output, each buffer one sentinel row longer than the contract says"""

    def __init__(self, scene, desc, lights, W, H, spp, tiled, flags=0, y0=0, y1=None, bands=None, rows=None, stream=None):
        import torch
        scene.set_lights(lights)
        rows = (H if y1 is None else y1) - y0 if rows is None else rows
        self.n, self.n_pixels = rows * W * spp, rows * W
        f32 = dict(dtype=torch.float32, device="cuda")
        self.rgb = torch.full((self.n_pixels + 1, 3), SENTINEL, **f32)
        self.hits = torch.full((self.n + 1, 4), SENTINEL, **f32)
        self.sample_rgb, self.color, self.normal = (torch.full((self.n + 1, 3), SENTINEL, **f32) for _ in range(3))
        self.counts = torch.tensor(COUNTS0, dtype=torch.int64, device="cuda")
        scene.render_lights_surface(camera(desc), W, H, self.rgb, y0=y0, y1=y1, bands=bands, spp=spp, jitter=spp > 1, seed=168, tiled=tiled,
                                    flags=flags, d_hits=self.hits, d_sample_rgb=self.sample_rgb, d_sample_color=self.color,
                                    d_sample_normal=self.normal, d_counts=self.counts, stream=stream)
        torch.cuda.synchronize()
        for t, k in ((self.rgb, self.n_pixels), (self.hits, self.n), (self.sample_rgb, self.n), (self.color, self.n), (self.normal, self.n)):
            assert bool((t[k] == SENTINEL).all()), "written beyond the end"
        self.counted = tuple(int(c) - c0 for c, c0 in zip(self.counts.cpu().numpy(), COUNTS0))


def fused_of(miro, name, W, H, spp, tiled, flags=0):
    key = (name, W, H, spp, tiled, flags)
    if key not in _FUSED:
        scene, desc, lights = scene_of(miro, name)
        _FUSED[key] = Fused(scene, desc, lights, W, H, spp, tiled, flags)
    return _FUSED[key]


def without_table(miro, name, W, H, spp, tiled):
    """The same frame of the same scene with its texture table cleared (every hit plain Phong); the table is set again afterwards,
    materials first, as the scene's setup set them"""
    key = (name, W, H, spp, tiled)
    if key not in _PLAIN:
        scene, desc, lights = scene_of(miro, name)
        scene.set_textures([])
        _PLAIN[key] = Fused(scene, desc, lights, W, H, spp, tiled)
        if "materials" in desc:
            scene.set_materials(desc["materials"], desc["prim_material"])
        scene.set_textures(desc["textures"], desc["material_texture"])
    return _PLAIN[key]


def assert_frame_is_the_chain(fu, ch, n_lights):
    """hit records on their bits; the surface pass's colour and normal, the rows of misses untouched on both sides; per-sample L;
    pixels against the chain's tree; all three counter deltas -- nothing left out"""
    assert fu.n == ch.n and ch.n_hits > 0 and float(ch.rgb.max()) > 0
    assert np.array_equal(bits(fu.hits[:fu.n]), bits(ch.hits))
    assert same(fu.color[:fu.n][ch.hit_rows], ch.color[ch.hit_rows]) and same(fu.normal[:fu.n][ch.hit_rows], ch.normal[ch.hit_rows])
    assert bool((fu.color[:fu.n][~ch.hit_rows] == SENTINEL).all()) and bool((fu.normal[:fu.n][~ch.hit_rows] == SENTINEL).all())
    assert bool((ch.color[ch.hit_rows] != SENTINEL).any())
    assert same(fu.sample_rgb[:fu.n], ch.ray_rgb)
    assert same(fu.rgb[:fu.n_pixels], ch.rgb)
    assert fu.counted == (ch.n, ch.n_hits * n_lights, ch.undefined)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", ["mixed", "stone", "flower", "teapot_textured"])
def test_frame_is_the_batched_chain_bit_for_bit(miro, name, shape):
    """mixed: the room with petal, leaf, flower centre, stem, checker and plain materials under a disc and a point light, glass and
    mirror spheres and a plane (kTraceExactObj, the refractive occluder's scale); stone: the room with bump-mapped floor and
    walls; flower: makeTestPetalScene under its disc light; teapot_textured: triangles only (kTraceExact) under four point
    lights, a leaf on the teapot and a checker over texture coordinates on the floor.  Not vacuous: the frame differs from the
    same scene without its texture table, and on the stone room the floor's normals are bumped."""
    W, H, spp, tiled = shape
    lights = scene_of(miro, name)[2]
    fu, ch = fused_of(miro, name, W, H, spp, tiled), chain_of(miro, name, W, H, spp, tiled)
    print("%s %s: %d samples, %d hits, %d lights, max %.4g, %d undefined" % (name, shape, ch.n, ch.n_hits, len(lights), float(ch.rgb.max()), ch.undefined))
    assert len(lights) == {"mixed": 2, "stone": 2, "flower": 1, "teapot_textured": 4}[name]
    assert_frame_is_the_chain(fu, ch, len(lights))
    plain = without_table(miro, name, W, H, spp, tiled)
    assert np.array_equal(bits(plain.hits), bits(fu.hits)) and not same(plain.rgb, fu.rgb) and not same(plain.color, fu.color)
    assert float(plain.rgb[:plain.n_pixels].max()) > 0 and plain.counted[2] == 0
    if name == "stone":                                 # the floor plane's own normal is (0, 1, 0): some of its samples are bumped
        floor = (plain.normal[:fu.n] == torch_row(plain.normal, (0.0, 1.0, 0.0))).all(dim=1)
        assert int(floor.sum()) > 0 and bool((fu.normal[:fu.n][floor] != plain.normal[:fu.n][floor]).any())
    if tiled:                                           # the sample order changes, the picture does not
        assert same(fu.rgb, fused_of(miro, name, W, H, spp, False).rgb)
        assert not np.array_equal(bits(fu.hits), bits(fused_of(miro, name, W, H, spp, False).hits))


def torch_row(like, values):
    import torch
    return torch.tensor(values, dtype=like.dtype, device=like.device)


@pytest.mark.gpu
def test_undefined_lookups_are_counted(miro):
    """The mixed room with its LEAF at scale 1e10: on the wall x = 2 the noise coordinates P.xy * scale lie beyond 2^30, where the
    reference's int(floor()) is undefined (mr_noise.h).  mr_hit_surface's own count on the batch is positive and below the
    number of hits, and d_counts[2] equals it; everything else is the chain's as before."""
    W, H, spp = 37, 19, 4
    fu, ch = fused_of(miro, "beyond", W, H, spp, False), chain_of(miro, "beyond", W, H, spp, False)
    print("%d of %d hits undefined" % (ch.undefined, ch.n_hits))
    assert 0 < ch.undefined < ch.n_hits and fu.counted[2] == ch.undefined
    assert_frame_is_the_chain(fu, ch, 2)
    assert chain_of(miro, "mixed", W, H, spp, False).undefined == 0 == fused_of(miro, "mixed", W, H, spp, False).counted[2]


@pytest.mark.gpu
def test_traversal_flags(miro):
    """MR_MATH_PRODUCT, MR_TRACE_INCOHERENT and both on the triangles-only textured scene against the chain run with the same
    flags (kTraceProduct, kTraceVote, kTraceVoteProduct).  MR_TRACE_ANY (shadow rays only) on that opaque scene: the closest-hit
    frame in every output; on the mixed room with its glass sphere: MR_ERR_STATE."""
    from miro_amd import binding
    W, H, spp = 37, 19, 4
    name = "teapot_textured"
    for flags in (binding.MR_MATH_PRODUCT, binding.MR_TRACE_INCOHERENT, binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT):
        assert_frame_is_the_chain(fused_of(miro, name, W, H, spp, False, flags), chain_of(miro, name, W, H, spp, False, flags), 4)
    for flags in (binding.MR_TRACE_ANY, binding.MR_TRACE_ANY | binding.MR_MATH_PRODUCT, binding.MR_TRACE_ANY | binding.MR_TRACE_INCOHERENT,
                  binding.MR_TRACE_ANY | binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT):
        base = flags & ~binding.MR_TRACE_ANY
        want, any_hit = fused_of(miro, name, W, H, spp, False, base), fused_of(miro, name, W, H, spp, False, flags)
        assert same(any_hit.rgb, want.rgb) and same(any_hit.sample_rgb, want.sample_rgb)
        assert same(any_hit.color, want.color) and same(any_hit.normal, want.normal)
        assert np.array_equal(bits(any_hit.hits), bits(want.hits)) and any_hit.counted == want.counted
        assert_frame_is_the_chain(any_hit, chain_of(miro, name, W, H, spp, False, base), 4)
    scene, desc, lights = scene_of(miro, "mixed")
    with pytest.raises(miro.MiroError) as e:
        Fused(scene, desc, lights, W, H, spp, False, flags=binding.MR_TRACE_ANY)
    assert e.value.status == binding.MR_ERR_STATE and "refractive" in str(e.value)


@pytest.mark.gpu
def test_row_windows_and_interleaved_bands(miro):
    """The mixed room at 37 x 19 x 4.  Rows [3, 11) are those rows of the full frame; the shards of band_rows = 2, world = 3
    (H = 19: a ragged last band), every rank, put back with band_rows_of / band_locate, are the full frame -- pixels, hit
    records, per-sample colour, normal and L -- and their counters sum to its; an empty window is MR_OK and writes nothing."""
    W, H, spp = 37, 19, 4
    scene, desc, lights = scene_of(miro, "mixed")
    full, ch = fused_of(miro, "mixed", W, H, spp, False), chain_of(miro, "mixed", W, H, spp, False)
    assert_frame_is_the_chain(full, ch, len(lights))
    per_sample = ("sample_rgb", "color", "normal")
    win = Fused(scene, desc, lights, W, H, spp, False, y0=3, y1=11)
    assert same(win.rgb[:8 * W], full.rgb[3 * W:11 * W])
    assert np.array_equal(bits(win.hits[:win.n]), bits(full.hits[3 * W * spp:11 * W * spp]))
    for f in per_sample:
        assert same(getattr(win, f)[:win.n], getattr(full, f)[3 * W * spp:11 * W * spp]), f
    prim = bits(ch.hits)[3 * W * spp:11 * W * spp, 1]
    assert win.counted == (8 * W * spp, int((prim != MISS).sum()) * len(lights), 0)
    band, world = 2, 3
    shards = []
    for r in range(world):
        rows = miro.band_rows_of(H, band, r, world)
        shards.append(Fused(scene, desc, lights, W, H, spp, False, bands=(band, r, world), rows=rows))
    assert [s.n_pixels // W for s in shards] == [7, 6, 6]          # ten bands; the last one, row 18 alone, is rank 0's fourth
    for y in range(H):
        r, j = miro.band_locate(H, band, world, y)
        sh = shards[r]
        assert same(sh.rgb[j * W:(j + 1) * W], full.rgb[y * W:(y + 1) * W]), y
        assert np.array_equal(bits(sh.hits[j * W * spp:(j + 1) * W * spp]), bits(full.hits[y * W * spp:(y + 1) * W * spp])), y
        for f in per_sample:
            assert same(getattr(sh, f)[j * W * spp:(j + 1) * W * spp], getattr(full, f)[y * W * spp:(y + 1) * W * spp]), (y, f)
    assert tuple(sum(s.counted[k] for s in shards) for k in range(3)) == full.counted
    empty = Fused(scene, desc, lights, W, H, spp, False, y0=7, y1=7)
    assert empty.counted == (0, 0, 0)
    for t in (empty.rgb, empty.hits, empty.sample_rgb, empty.color, empty.normal):
        assert bool((t == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[SHAPE_IDS[1], SHAPE_IDS[3]])
def test_without_a_texture_table_it_is_mr_render_lights(miro, shape):
    """The teapot with its four lights and no texture table: d_rgb, d_hits, d_sample_rgb and the two ray counters equal
    mr_render_lights' bit for bit; the colour rows of the hits hold the white Lambert's diffuse, no lookup is undefined."""
    import torch
    W, H, spp, tiled = shape
    scene, desc, lights = scene_of(miro, "teapot")
    fu = Fused(scene, desc, lights, W, H, spp, tiled)
    n = fu.n
    rgb = torch.full((W * H, 3), SENTINEL, dtype=torch.float32, device="cuda")
    hits = torch.full((n, 4), SENTINEL, dtype=torch.float32, device="cuda")
    sample = torch.full((n, 3), SENTINEL, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    scene.render_lights(camera(desc), W, H, rgb, spp=spp, jitter=spp > 1, seed=168, tiled=tiled, d_hits=hits, d_sample_rgb=sample, d_counts=cnt)
    torch.cuda.synchronize()
    assert float(rgb.max()) > 0 and int(cnt[1]) > 0
    assert same(fu.rgb[:W * H], rgb) and np.array_equal(bits(fu.hits[:n]), bits(hits)) and same(fu.sample_rgb[:n], sample)
    assert fu.counted == (int(cnt[0]), int(cnt[1]), 0)
    hit_rows = hits[:, 1].contiguous().view(torch.int32) != -1
    assert bool((fu.color[:n][hit_rows] == 1.0).all()) and bool((fu.color[:n][~hit_rows] == SENTINEL).all())


@pytest.mark.gpu
def test_replays_from_a_captured_graph(miro):
    """After one warm call (which uploads the texture table: an allocation and a copy that may not lie inside a capture) the
    37 x 19 x 4 frame of the mixed room is captured into a torch.cuda.graph and replayed twice, d_rgb filled with a sentinel
    before each replay: equal to the direct launch."""
    import torch
    W, H, spp = 37, 19, 4
    scene, desc, lights = scene_of(miro, "mixed")
    first = fused_of(miro, "mixed", W, H, spp, False)
    assert_frame_is_the_chain(first, chain_of(miro, "mixed", W, H, spp, False), len(lights))
    scene.set_lights(lights)
    cam = camera(desc)
    out = torch.full((W * H, 3), SENTINEL, dtype=torch.float32, device="cuda")
    scene.render_lights_surface(cam, W, H, out, spp=spp, jitter=True)             # warm: the table is on the device
    torch.cuda.synchronize()
    assert same(out, first.rgb[:W * H])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        scene.render_lights_surface(cam, W, H, out, spp=spp, jitter=True, stream=torch.cuda.current_stream())
    for _ in range(2):
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(out, first.rgb[:W * H])


@pytest.mark.gpu
def test_fused_frame_with_a_light_list_on_a_textured_scene(miro):
    """FusedFrame(lights=...) on the mixed room -- a frame that raised before -- fills d_rgb and d_hits as the direct
    render_lights_surface call does, ray_counts() is (samples, hits x lights) and undefined_lookups() the third counter; on the
    teapot without a table it still equals Scene.render_lights."""
    import torch
    from miro_amd import frame
    W, H, spp = 37, 19, 4
    scene, desc, lights = scene_of(miro, "mixed")
    ff = frame.FusedFrame(scene, desc, W, H, spp=spp, keep_hits=True, lights=lights)
    assert ff.tiled and ff.jitter and ff.d_counts.numel() == 3
    ff.step()
    torch.cuda.synchronize()
    want, ch = fused_of(miro, "mixed", W, H, spp, True), chain_of(miro, "mixed", W, H, spp, True)
    assert_frame_is_the_chain(want, ch, len(lights))
    assert same(ff.d_rgb, want.rgb[:W * H]) and np.array_equal(bits(ff.d_hits), bits(want.hits[:ff.n]))
    assert ff.ray_counts() == (ch.n, ch.n_hits * len(lights)) and ff.undefined_lookups() == 0
    scene, desc, lights = scene_of(miro, "beyond")
    ff = frame.FusedFrame(scene, desc, W, H, spp=spp, lights=lights, tiled=False)
    ff.step()
    assert ff.undefined_lookups() == chain_of(miro, "beyond", W, H, spp, False).undefined > 0
    scene, desc, lights = scene_of(miro, "teapot")
    ff = frame.FusedFrame(scene, desc, W, H, spp=spp, lights=lights)
    ff.step()
    rgb = torch.full((W * H, 3), SENTINEL, dtype=torch.float32, device="cuda")
    scene.render_lights(ff.cam, W, H, rgb, spp=spp, jitter=True, seed=168, tiled=True)
    torch.cuda.synchronize()
    assert float(rgb.max()) > 0 and same(ff.d_rgb, rgb) and ff.undefined_lookups() == 0


@pytest.mark.gpu
def test_scene_state_errors(miro):
    """MR_ERR_STATE for a scene without lights and for a scene that is not built; neither writes anything."""
    import torch
    from miro_amd import binding, scenes
    scene, desc, lights = scene_of(miro, "mixed")
    rgb = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    scene.set_lights([])
    with pytest.raises(miro.MiroError) as e:
        scene.render_lights_surface(camera(desc), 8, 8, rgb)
    assert e.value.status == binding.MR_ERR_STATE and "no lights" in str(e.value) and NAME in str(e.value)
    scene.set_lights(lights)
    unbuilt = miro.Scene(0)
    scenes.populate(unbuilt, scenes.SCENES["teapot"])
    unbuilt.set_lights(TEAPOT_LIGHTS)
    with pytest.raises(miro.MiroError) as e:
        unbuilt.render_lights_surface(camera(desc), 8, 8, rgb)
    assert e.value.status == binding.MR_ERR_STATE and "mr_bvh_build" in str(e.value)
    torch.cuda.synchronize()
    assert float(rgb.abs().max()) == 0.0
