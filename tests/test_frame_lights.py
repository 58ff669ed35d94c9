"""mr_render_lights -- the fused direct-light frame over the scene's light list (csrc/mr_frame_lights.hip): Camera::eyeRay ->
Scene::trace -> Phong::shade's loop over Scene::lights() (Phong.cpp:59-63) -> the pixel's mean, in one launch.

The yardstick everywhere is the batched chain on the same scene, camera, seed and sample order,

    gen_eye_rays[_tiled] -> trace -> shade_lights(..., d_ray_rgb=...)

which tests/test_lights.py holds against the oracle and the restatement, and tests/test_lights_fuzz.py does so -- chain and
frame -- on seeded tie and NaN scenes.  The comparisons are EXACT: both sides run the same
device functions in the same order under -ffp-contract=off.  Hit records are compared on their bits, per-sample L with
np.array_equal(equal_nan=True), and d_rgb against the pairwise tree over the chain's per-sample L (x[:, 0::2] + x[:, 1::2] in
float32 until one value is left, times float32(1 / spp) when spp > 1 -- the xor-butterfly of the kernel, seen from sample 0)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402

F = np.float32
MISS = 0xFFFFFFFF
INF = float("inf")
SENTINEL = -7.0

# four point lights placed around the teapot as assignment1.cpp:106-128 places its four around its spheres (two low ones left
# and right in front, a strong one high above, one in front above; that scene looks down -z, the teapot's camera sits at +z)
TEAPOT_LIGHTS = [dict(position=(-2.0, 3.0, 6.0), color=(1.0, 1.0, 1.0), wattage=30.0),
                 dict(position=(2.0, 4.5, 6.5), color=(1.0, 1.0, 1.0), wattage=30.0),
                 dict(position=(0.0, 20.0, 0.0), color=(1.0, 1.0, 1.0), wattage=1000.0),
                 dict(position=(0.0, 5.0, 7.0), color=(1.0, 1.0, 1.0), wattage=30.0)]
# MR_MAX_LIGHTS point lights on a ring above A1makeSphereScene, every one with its own colour and wattage
SPHERE_LIGHTS = [dict(position=(4.0 * np.cos(0.8 * k), 3.0 + 0.5 * k, 4.0 * np.sin(0.8 * k)),
                      color=(1.0 - 0.1 * k, 0.3 + 0.08 * k, 0.5 + 0.05 * (k % 3)), wattage=40.0 + 25.0 * k) for k in range(8)]
# ... and a material table for it: a diffuse floor, a sphere with a highlight (finite shininess)
SPHERE_MATERIALS = [((0.8, 0.7, 0.6), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), INF, 1.0),
                    ((0.5, 0.6, 0.9), (0.2, 0.2, 0.2), (0.0, 0.0, 0.0), 40.0, 1.0)]
SHAPES = [(37, 19, 1, False), (37, 19, 4, False), (5, 1, 64, False), (37, 19, 4, True)]       # W, H, spp, tiled; jitter = spp > 1
SHAPE_IDS = ["37x19x1", "37x19x4", "5x1x64", "37x19x4-tiled"]


def frame_desc(binding, W=8, H=8, y0=0, y1=None, bands=(1, 0, 1), spp=1, flags=0):
    fd = binding.FrameDesc()
    fd.camera = binding.make_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 45.0)
    fd.W, fd.H, fd.y0, fd.y1 = W, H, y0, H if y1 is None else y1
    fd.band_rows, fd.band_rank, fd.band_world = bands
    fd.spp, fd.jitter, fd.seed, fd.tiled, fd.flags = spp, 0, 168, 0, flags
    return fd


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_render_lights_is_exported_and_declared_outside_the_69(miro):
    from miro_amd import binding
    name = "mr_render_lights"

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return re.search(r"\bmr_status\s+%s\s*\(" % name, src) is not None

    assert hasattr(miro.lib(), name) and name in binding.SURFACE_SYMBOLS and name not in miro.EXPORTED_SYMBOLS
    assert declared("miro_hip_surface.h") and not declared("miro_hip.h")
    assert len(miro.EXPORTED_SYMBOLS) == len(set(miro.EXPORTED_SYMBOLS)) == 69
    assert hasattr(miro.Scene, "render_lights")


def test_render_lights_argument_errors_come_before_the_scene_and_the_device(miro):
    """Every MR_ERR_INVALID case on an UNBUILT one-triangle scene: answered from the arguments alone, so neither "not built" nor
    "no HIP device" may be what comes back.  Then MR_ERR_STATE for the unbuilt and for a host_only scene; and the scene is as
    usable afterwards as before."""
    from miro_amd import binding
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    rgb, hits = C.c_void_p(1024), C.c_void_p(2048)

    def call(fd, scene=s.h, d_rgb=rgb, d_hits=hits, d_sample=None, d_counts=None):
        st = L.mr_render_lights(scene, C.byref(fd) if fd is not None else None, d_rgb, d_hits, d_sample, d_counts, None)
        return st, L.mr_last_error()

    ok = frame_desc(binding)
    invalid = [
        ("NULL", call(ok, scene=None)), ("NULL", call(None)), ("NULL", call(ok, d_rgb=None)),
        ("spp", call(frame_desc(binding, spp=0))), ("spp", call(frame_desc(binding, spp=3))), ("spp", call(frame_desc(binding, spp=128))),
        ("band", call(frame_desc(binding, bands=(2, 3, 3)))), ("band", call(frame_desc(binding, bands=(0, 1, 2)))),
        ("rows", call(frame_desc(binding, y1=9))), ("rows", call(frame_desc(binding, y0=5, y1=4))),
        ("too large", call(frame_desc(binding, W=65536, H=65536))),
        ("flags", call(frame_desc(binding, flags=binding.MR_FRAME_NO_SHADOWS))), ("flags", call(frame_desc(binding, flags=binding.MR_MATH_FAST))),
        ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY | (1 << 30)))),
        ("aligned", call(ok, d_hits=C.c_void_p(2048 + 8))), ("aligned", call(ok, d_counts=C.c_void_p(4100))),
        ("aligned", call(ok, d_sample=C.c_void_p(4098))),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and b"mr_render_lights" in msg and b"HIP device" not in msg and b"built" not in msg, (word, msg)
    # the scene's state comes next: not built, then built host_only -- never a CPU path
    st, msg = call(ok)
    assert st == binding.MR_ERR_STATE and b"HIP device" not in msg, msg
    s.build(4, host_only=True)
    st, msg = call(ok)
    assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg
    for word, (st, msg) in [("spp", call(frame_desc(binding, spp=5))), ("flags", call(frame_desc(binding, flags=binding.MR_FRAME_NO_SHADOWS)))]:
        assert st == binding.MR_ERR_INVALID and word.encode() in msg             # still the arguments first
    # the refused calls left the scene alone
    assert s.info().n_triangles == 1
    s.set_lights([dict(position=(0, 2, 0), wattage=7.0), dict(position=(0, 1, 0), normal=(0, -1, 0), wattage=5.0, radius=1.0)])
    s.build(4, host_only=True)
    assert s.info().n_triangles == 1


def test_frame_lights_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_frame_lights.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer waves
    per SIMD than BOTH its own record (tests/golden/kernel_budget_frame_lights.json, written from the build whose GPU run of
    this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.  One kernel per traversal
    variant of with_trace_variant (six) and shadow-ray form (closest hit, any hit)."""
    cur = kernel_budget.unit_kernels("mr_frame_lights")
    assert len(cur) == 6 * 2 and all("frame_lights_kernel" in k for k in cur)
    for var in (1818, 826, 267, 43, 88, 73):                   # kTraceExact, ExactObj, Product, ProductObj, Vote, VoteProduct
        for any_hit in (0, 1):
            assert sum("ILi%dELb%dEE" % (var, any_hit) in k for k in cur) == 1, (var, any_hit)
    assert not any(v["dynamic_stack"] for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_frame_lights.json", also_main=True)


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
_SCENES, _CHAINS, _FUSED = {}, {}, {}


def scene_of(miro, name):
    """(scene, description, lights) of a test scene, built once per session; the caller sets the lights it wants"""
    from miro_amd import scenes
    if name not in _SCENES:
        desc = scenes.SCENES["photon_room" if name == "photon_room_point" else name]
        s = miro.Scene(0)
        scenes.populate(s, desc)
        if name == "a1sphere":
            s.set_materials(SPHERE_MATERIALS, [0, 1])
        elif "materials" in desc:
            s.set_materials(desc["materials"], desc["prim_material"])
        s.build(4)
        lights = {"teapot": TEAPOT_LIGHTS, "a1sphere": SPHERE_LIGHTS}.get(name)
        if name == "photon_room_point":
            lights = [dict(position=desc["light"], color=(1.0, 1.0, 1.0), wattage=desc["wattage"])]
        _SCENES[name] = (s, desc, lights if lights is not None else desc["lights"])
    return _SCENES[name]


def camera(desc):
    from miro_amd import binding
    return binding.make_camera(desc["eye"], desc["lookat"], desc["up"], desc["fov"])


def pixel_tree(x, spp):
    """[pixels, spp, 3] float32 -> [pixels, 3]: the kernel's butterfly as sample 0 sees it (numpy or torch, float32 throughout)"""
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    x = x[:, 0]
    return x * F(1.0 / spp) if spp > 1 else x


class Chain:
    """The batched chain of one frame, resident on the device: rays, hits, per-sample L, and the pixels of its pairwise tree
    in image order.  Computed once per (scene, lights, shape, flags) and shared."""

    def __init__(self, miro, scene, desc, lights, W, H, spp, tiled, flags=0):
        import torch
        from miro_amd import binding
        scene.set_lights(lights)
        self.n = n = W * H * spp
        rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        self.hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        self.ray_rgb = torch.full((n, 3), SENTINEL, dtype=torch.float32, device="cuda")
        scene.gen_eye_rays(camera(desc), W, H, rays, spp=spp, jitter=spp > 1, seed=168, tiled=tiled)
        scene.trace_device(rays, n, self.hits, flags & (binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT))
        scene.shade_lights(rays, self.hits, n, None, spp=spp, flags=flags, d_ray_rgb=self.ray_rgb)
        torch.cuda.synchronize()
        slots = pixel_tree(self.ray_rgb.view(W * H, spp, 3), spp)
        self.rgb = slots
        if tiled:                                       # slot p of the tiled order is pixel tile_pixel_map[p]
            m = torch.from_numpy(binding.tile_pixel_map(W, H, spp).astype(np.int64)).cuda()
            self.rgb = torch.empty_like(slots)
            self.rgb[m] = slots
        self.n_hits = int((self.hits[:, 1].contiguous().view(torch.int32) != -1).sum().item())


def chain_of(miro, name, W, H, spp, tiled, flags=0, lights=None):
    key = (name, W, H, spp, tiled, flags, None if lights is None else len(lights))
    if key not in _CHAINS:
        scene, desc, own = scene_of(miro, name)
        _CHAINS[key] = Chain(miro, scene, desc, own if lights is None else lights, W, H, spp, tiled, flags)
    return _CHAINS[key]


class Fused:
    """One mr_render_lights call with every optional output, each buffer one sentinel row longer than the contract says"""

    def __init__(self, scene, desc, lights, W, H, spp, tiled, flags=0, y0=0, y1=None, bands=None, rows=None, stream=None, outputs=True):
        import torch
        scene.set_lights(lights)
        rows = (H if y1 is None else y1) - y0 if rows is None else rows
        self.n, self.n_pixels = rows * W * spp, rows * W
        self.rgb = torch.full((self.n_pixels + 1, 3), SENTINEL, dtype=torch.float32, device="cuda")
        self.hits = torch.full((self.n + 1, 4), SENTINEL, dtype=torch.float32, device="cuda") if outputs else None
        self.sample_rgb = torch.full((self.n + 1, 3), SENTINEL, dtype=torch.float32, device="cuda") if outputs else None
        self.counts = torch.tensor([1000, 5], dtype=torch.int64, device="cuda")      # not zeroed by the call
        scene.render_lights(camera(desc), W, H, self.rgb, y0=y0, y1=y1, bands=bands, spp=spp, jitter=spp > 1, seed=168, tiled=tiled,
                            flags=flags, d_hits=self.hits, d_sample_rgb=self.sample_rgb, d_counts=self.counts, stream=stream)
        torch.cuda.synchronize()
        for t, k in ((self.rgb, self.n_pixels), (self.hits, self.n), (self.sample_rgb, self.n)):
            assert t is None or bool((t[k] == SENTINEL).all()), "written beyond the end"
        c = self.counts.cpu().numpy()
        self.counted = (int(c[0]) - 1000, int(c[1]) - 5)


def fused_of(miro, name, W, H, spp, tiled, flags=0):
    key = (name, W, H, spp, tiled, flags)
    if key not in _FUSED:
        scene, desc, lights = scene_of(miro, name)
        _FUSED[key] = Fused(scene, desc, lights, W, H, spp, tiled, flags)
    return _FUSED[key]


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same(a, b):
    return np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy(), equal_nan=True)


def assert_frame_is_the_chain(fu, ch, n_lights):
    """hit records on their bits, per-sample L, pixels against the chain's tree, counter deltas -- nothing left out"""
    assert fu.n == ch.n and ch.n_hits > 0 and float(ch.rgb.max()) > 0
    assert np.array_equal(bits(fu.hits[:fu.n]), bits(ch.hits))
    assert same(fu.sample_rgb[:fu.n], ch.ray_rgb)
    assert same(fu.rgb[:fu.n_pixels], ch.rgb)
    assert fu.counted == (ch.n, ch.n_hits * n_lights)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", ["teapot", "photon_room_two_lights", "a1sphere"])
def test_frame_is_the_batched_chain_bit_for_bit(miro, name, shape):
    """teapot: four point lights, no material table (white Lambert, triangles only); the two-light room: disc + point, glass and
    mirror spheres and a plane (kTraceExactObj, the refractive occluder's scale); a1sphere: MR_MAX_LIGHTS point lights and a
    material table.  37 x 19 at 1 spp is 703 samples -- a ragged last wave and a ragged last workgroup."""
    W, H, spp, tiled = shape
    lights = scene_of(miro, name)[2]
    fu, ch = fused_of(miro, name, W, H, spp, tiled), chain_of(miro, name, W, H, spp, tiled)
    print("%s %s: %d samples, %d hits, %d lights, max %.4g" % (name, shape, ch.n, ch.n_hits, len(lights), float(ch.rgb.max())))
    assert len(lights) == {"teapot": 4, "photon_room_two_lights": 2, "a1sphere": 8}[name]
    assert_frame_is_the_chain(fu, ch, len(lights))
    if tiled:                                           # the sample order changes, the picture does not
        assert same(fu.rgb, fused_of(miro, name, W, H, spp, False).rgb)
        assert not np.array_equal(bits(fu.hits), bits(fused_of(miro, name, W, H, spp, False).hits))


@pytest.mark.gpu
def test_eight_lights_are_four_plus_four(miro):
    """The same eight lights in one frame against the first four in one frame plus the last four in another: within 1e-6 of the
    frame's largest value.  Only the ORDER OF ADDITIONS differs -- ((((a+b)+c)+d)+e)+... in one launch, (a+b+c+d) + (e+f+g+h)
    here -- and every term is the same float32 number on both sides: at most seven roundings of values below the maximum."""
    scene, desc, lights = scene_of(miro, "a1sphere")
    W, H, spp = 37, 19, 1
    whole = fused_of(miro, "a1sphere", W, H, spp, False)
    first, last = Fused(scene, desc, lights[:4], W, H, spp, False), Fused(scene, desc, lights[4:], W, H, spp, False)
    a = whole.rgb[:W * H].cpu().numpy().astype(np.float64)
    b = first.rgb[:W * H].cpu().numpy().astype(np.float64) + last.rgb[:W * H].cpu().numpy().astype(np.float64)
    print("max %.4g, worst difference %.3g" % (a.max(), np.abs(a - b).max()))
    assert a.max() > 0 and first.rgb.max() > 0 and last.rgb.max() > 0
    assert np.abs(a - b).max() <= 1e-6 * a.max()
    assert first.counted[1] == last.counted[1] == whole.counted[1] // 2 > 0
    assert np.array_equal(bits(first.hits), bits(whole.hits))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["teapot", "photon_room_two_lights"])
def test_row_windows_and_interleaved_bands(miro, name):
    """Rows [3, 11) of the 37 x 19 frame are those rows of the full frame; the shards of band_rows = 2, world = 3 (H = 19: a
    ragged last band), every rank, put back with band_rows_of / band_locate, are the full frame -- pixels, hit records,
    per-sample L and counters -- and the full frame is the chain's."""
    W, H, spp = 37, 19, 4
    scene, desc, lights = scene_of(miro, name)
    full, ch = fused_of(miro, name, W, H, spp, False), chain_of(miro, name, W, H, spp, False)
    assert_frame_is_the_chain(full, ch, len(lights))
    win = Fused(scene, desc, lights, W, H, spp, False, y0=3, y1=11)
    assert same(win.rgb[:8 * W], full.rgb[3 * W:11 * W])
    assert np.array_equal(bits(win.hits[:win.n]), bits(full.hits[3 * W * spp:11 * W * spp]))
    assert same(win.sample_rgb[:win.n], full.sample_rgb[3 * W * spp:11 * W * spp])
    prim = bits(ch.hits)[3 * W * spp:11 * W * spp, 1]
    assert win.counted == (8 * W * spp, int((prim != MISS).sum()) * len(lights))
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
        assert same(sh.sample_rgb[j * W * spp:(j + 1) * W * spp], full.sample_rgb[y * W * spp:(y + 1) * W * spp]), y
    assert sum(s.counted[0] for s in shards) == full.counted[0] and sum(s.counted[1] for s in shards) == full.counted[1]
    # an empty window: MR_OK, nothing launched, nothing written
    empty = Fused(scene, desc, lights, W, H, spp, False, y0=7, y1=7)
    assert empty.counted == (0, 0)


@pytest.mark.gpu
def test_traversal_flags(miro):
    """MR_MATH_PRODUCT and MR_TRACE_INCOHERENT on the teapot: hit records equal to mr_trace's with the same flag, per-sample L and
    pixels equal to the chain run with the same flag.  MR_TRACE_ANY (shadow rays only) on the opaque teapot: the closest-hit
    frame's pixels and primary records; on the room with its glass sphere: MR_ERR_STATE."""
    from miro_amd import binding
    W, H, spp = 37, 19, 4
    plain = fused_of(miro, "teapot", W, H, spp, False)
    for flags in (binding.MR_MATH_PRODUCT, binding.MR_TRACE_INCOHERENT, binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT):
        assert_frame_is_the_chain(fused_of(miro, "teapot", W, H, spp, False, flags), chain_of(miro, "teapot", W, H, spp, False, flags), 4)
    for flags in (binding.MR_TRACE_ANY, binding.MR_TRACE_ANY | binding.MR_MATH_PRODUCT, binding.MR_TRACE_ANY | binding.MR_TRACE_INCOHERENT):
        base = flags & ~binding.MR_TRACE_ANY
        want = fused_of(miro, "teapot", W, H, spp, False, base)
        any_hit = fused_of(miro, "teapot", W, H, spp, False, flags)
        assert same(any_hit.rgb, want.rgb) and same(any_hit.sample_rgb, want.sample_rgb)
        assert np.array_equal(bits(any_hit.hits), bits(want.hits)) and any_hit.counted == want.counted
        assert_frame_is_the_chain(any_hit, chain_of(miro, "teapot", W, H, spp, False, base), 4)
    assert float(plain.rgb[:W * H].max()) > 0
    scene, desc, lights = scene_of(miro, "photon_room_two_lights")
    with pytest.raises(miro.MiroError) as e:
        Fused(scene, desc, lights, W, H, spp, False, flags=binding.MR_TRACE_ANY)
    assert e.value.status == binding.MR_ERR_STATE and "refractive" in str(e.value)


@pytest.mark.gpu
def test_scene_state_errors(miro):
    """MR_ERR_STATE for a scene without lights and for a scene with a texture table, whose message names the batched route."""
    import torch
    from miro_amd import binding, scenes
    scene, desc, lights = scene_of(miro, "teapot")
    rgb = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    scene.set_lights([])
    with pytest.raises(miro.MiroError) as e:
        scene.render_lights(camera(desc), 8, 8, rgb)
    assert e.value.status == binding.MR_ERR_STATE and "no lights" in str(e.value)
    scene.set_lights(lights)
    room = miro.Scene(0)
    rdesc = scenes.textured_room_setup(room, scenes.photon_room_mixed())
    room.set_lights(scenes.SCENES["photon_room_two_lights"]["lights"])
    with pytest.raises(miro.MiroError) as e:
        room.render_lights(camera(rdesc), 8, 8, rgb)
    assert e.value.status == binding.MR_ERR_STATE and "mr_shade_lights_surface" in str(e.value) and "texture table" in str(e.value)
    torch.cuda.synchronize()
    assert float(rgb.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 16])
def test_one_point_light_is_the_single_light_kernel(miro, spp):
    """photon_room with its material table and its one point light as a one-element list: d_rgb equals mr_render_direct's on the
    same descriptor (64 x 48), and the primary hit records are the same bits."""
    import torch
    scene, desc, lights = scene_of(miro, "photon_room_point")
    W, H = 64, 48
    n = W * H * spp
    want_rgb = torch.full((W * H, 3), SENTINEL, dtype=torch.float32, device="cuda")
    want_hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    scene.render_direct(camera(desc), W, H, want_rgb, desc["light"], desc["wattage"], spp=spp, jitter=spp > 1, seed=168, d_hits=want_hits,
                        d_counts=cnt)
    torch.cuda.synchronize()
    fu = Fused(scene, desc, lights, W, H, spp, False)
    print("spp %d: max %.4g, %s rays" % (spp, float(want_rgb.max()), cnt.tolist()))
    assert float(want_rgb.max()) > 0
    assert same(fu.rgb[:W * H], want_rgb)
    assert np.array_equal(bits(fu.hits[:n]), bits(want_hits))
    assert fu.counted == tuple(cnt.tolist())
    assert_frame_is_the_chain(fu, Chain(miro, scene, desc, lights, W, H, spp, False), 1)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(288, 256), (384, 352)], ids=["18432-chunks", "33792-chunks"])
def test_grid_stride_loop_and_xcd_order(miro, W, H):
    """64 spp on the teapot with two lights.  288 x 256: 18 432 chunks of 256 samples -- above kXcdMinGrid (16 384: workgroups are
    dealt to the XCDs in runs of 64), below the grid cap.  384 x 352: 33 792 chunks -- above kTraceGridCap (32 768), so the
    first 1 024 workgroups take a second chunk.  Compared on the device."""
    import torch
    scene, desc, lights = scene_of(miro, "teapot")
    spp = 64
    assert (W * H * spp) // 256 in (18432, 33792)
    ch = Chain(miro, scene, desc, lights[:2], W, H, spp, False)
    fu = Fused(scene, desc, lights[:2], W, H, spp, False)
    assert ch.n_hits > 0 and float(ch.rgb.max()) > 0
    assert torch.equal(fu.hits[:fu.n].view(torch.int32), ch.hits.view(torch.int32))
    assert same(fu.sample_rgb[:fu.n], ch.ray_rgb)
    assert same(fu.rgb[:W * H], ch.rgb)
    assert fu.counted == (ch.n, ch.n_hits * 2)
    del ch, fu
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_replays_from_a_captured_graph_and_runs_on_a_side_stream(miro):
    """The 37 x 19 x 4 frame captured into a torch.cuda.graph and replayed twice, d_rgb filled with a sentinel before each replay,
    equals the direct launch (the call only enqueues: one kernel, no allocation, no counter ring); the same frame on a side
    stream equals the default-stream result."""
    import torch
    W, H, spp = 37, 19, 4
    scene, desc, lights = scene_of(miro, "photon_room_two_lights")
    first = fused_of(miro, "photon_room_two_lights", W, H, spp, False)
    assert_frame_is_the_chain(first, chain_of(miro, "photon_room_two_lights", W, H, spp, False), len(lights))
    scene.set_lights(lights)
    cam = camera(desc)
    out = torch.full((W * H, 3), SENTINEL, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scene.render_lights(cam, W, H, out, spp=spp, jitter=True, stream=side)
    side.synchronize()
    assert same(out, first.rgb[:W * H])                                       # the side stream
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        scene.render_lights(cam, W, H, out, spp=spp, jitter=True, stream=torch.cuda.current_stream())
    for _ in range(2):
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same(out, first.rgb[:W * H])


@pytest.mark.gpu
def test_fused_frame_with_a_light_list(miro):
    """FusedFrame(lights=...): the list is set in the constructor, step() fills d_rgb as the direct render_lights call does,
    ray_counts() is (samples, hits x lights), keep_hits keeps the primary records only, no_shadows is refused.  Without `lights`
    FusedFrame still is mr_render_direct: equal to a direct render_direct call."""
    import torch
    from miro_amd import binding, frame
    W, H, spp = 37, 19, 4
    scene, desc, lights = scene_of(miro, "teapot")
    scene.set_lights([])
    ff = frame.FusedFrame(scene, desc, W, H, spp=spp, keep_hits=True, lights=lights, any_shadow=True)
    assert ff.d_hits is not None and ff.d_shadow_hits is None and ff.tiled and ff.jitter and ff.flags == binding.MR_TRACE_ANY
    ff.step()
    torch.cuda.synchronize()
    want = fused_of(miro, "teapot", W, H, spp, True, binding.MR_TRACE_ANY)
    ch = chain_of(miro, "teapot", W, H, spp, True)
    assert_frame_is_the_chain(want, ch, len(lights))
    assert same(ff.d_rgb, want.rgb[:W * H]) and np.array_equal(bits(ff.d_hits), bits(want.hits[:ff.n]))
    assert ff.ray_counts() == (ch.n, ch.n_hits * len(lights))
    with pytest.raises(ValueError):
        frame.FusedFrame(scene, desc, W, H, spp=spp, lights=lights, no_shadows=True)
    plain = frame.FusedFrame(scene, desc, W, H, spp=spp, keep_hits=True)
    assert plain.lights is None and plain.d_shadow_hits is not None
    plain.step()
    rgb = torch.full((W * H, 3), SENTINEL, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    scene.render_direct(plain.cam, W, H, rgb, desc["light"], desc["wattage"], spp=spp, jitter=True, seed=168, tiled=True, d_counts=cnt)
    torch.cuda.synchronize()
    assert float(rgb.max()) > 0 and same(plain.d_rgb, rgb) and plain.ray_counts() == tuple(cnt.tolist())
    assert not same(plain.d_rgb, ff.d_rgb)
