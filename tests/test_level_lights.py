"""mr_trace_level_lights -- one level of Scene::traceScene's recursion (Scene.cpp:270-346) in one launch on ANY scene
(csrc/mr_level_lights.hip): Scene::trace with its bump-mapped normal -> the environment of a ray that misses -> diffuseColor of a
TexturedPhong -> Phong::shade's loop over Scene::lights() -> weight x L to the ray's pixel -> the reflect / Fresnel / refract
children of the next level.

The yardstick everywhere is the batched chain on the same queue,

    trace -> hit_surface -> shade_lights_surface(..., d_ray_rgb) || shade_environment(flags 0, d_ray_rgb) -> gen_secondary_rays

which tests/test_procedural.py, tests/test_solid_textures.py, tests/test_lights.py, tests/test_environment.py and
tests/test_specular.py hold against the oracle and the restatements (tests/test_lights_fuzz.py: the light loop and this kernel
against its chain on seeded tie and NaN scenes).  Per-ray outputs and counters are compared EXACTLY (both
sides run the same device functions in the same order under -ffp-contract=off), the children as sets (the two compactions order
them differently), the pixel sums within the bound of tests/test_level.py (float atomics).

Not reachable at test size and not tested: the kernel's grid-stride loop, which starts at 8.4 M rays (the grid cap is 32 768
workgroups of 256 lanes)."""
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
from test_frame_lights import MISS, SENTINEL, bits, camera, same  # noqa: E402
from test_frame_lights_environment import BG, ROTATION, image  # noqa: E402
from test_frame_lights_surface import scene_of  # noqa: E402
from test_level import canon  # noqa: E402

F = np.float32
NAME = "mr_trace_level_lights"
COUNTS0 = (1000, 5, 77, 31, 9)                          # what d_counts holds before a call: the call does not zero it
W, H, SPP = 80, 60, 2
ENVS = {None: None, "colour": dict(bg_color=BG), "image": dict(pixels=image(168), rotation=ROTATION)}
PIX = 0x7A7A7A7A                                        # the sentinel of an int32 queue column


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_trace_level_lights_is_exported_declared_and_bound(miro):
    from miro_amd import binding

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return re.search(r"\bmr_status\s+%s\s*\(" % NAME, src) is not None

    assert hasattr(miro.lib(), NAME)
    assert declared("miro_hip_frame.h") and not declared("miro_hip.h") and not declared("miro_hip_surface.h")
    assert NAME in binding.FRAME_SYMBOLS and NAME not in binding.SURFACE_SYMBOLS and NAME not in miro.EXPORTED_SYMBOLS
    assert len(binding.FRAME_SYMBOLS) == len(set(binding.FRAME_SYMBOLS))
    assert len(miro.EXPORTED_SYMBOLS) == 69 and len(binding.SURFACE_SYMBOLS) == 9
    assert getattr(miro.lib(), NAME).restype is C.c_int32
    assert hasattr(miro.Scene, "trace_level_lights") and C.sizeof(binding.LevelLightsDesc) == 56


def test_level_lights_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_level_lights.hip: no dynamic stack; at least four waves per SIMD; no more spilled VGPRs, no more scratch
    per lane and no fewer waves than BOTH its own record (tests/golden/kernel_budget_level_lights.json, written from the build
    whose GPU run of this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.  Twelve level
    kernels, one per traversal variant of with_trace_variant (six) and children (none, specular): the environment is a
    wave-uniform branch.  The unit's only other kernel is the one-word store that zeroes d_out_count, held to the same record."""
    cur = kernel_budget.unit_kernels("mr_level_lights")
    level = [k for k in cur if "level_lights_kernel" in k]
    assert len(level) == 6 * 2 and sorted(set(cur) - set(level)) == ["mr_level_lights:_ZN2mr12_GLOBAL__N_117zero_count_kernelEPy"]
    assert not any("frame_kernel" in k or "trace_kernel" in k for k in cur)
    for var in (1818, 826, 267, 43, 88, 73):                   # kTraceExact, ExactObj, Product, ProductObj, Vote, VoteProduct
        for children in (0, 1):
            assert sum("ILi%dELi%dEE" % (var, children) in k for k in cur) == 1, (var, children)
    assert not any(v["dynamic_stack"] for v in cur.values())
    assert all(v["waves_per_simd"] >= 4 for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_level_lights.json", also_main=True)


def level_desc(binding, spp=1, flags=0, children=0, environment=0, capacity=0, reserved=None):
    ld = binding.LevelLightsDesc()
    ld.spp, ld.flags, ld.children, ld.environment = spp, flags, children, environment
    ld.out_capacity_lo, ld.out_capacity_hi = capacity & 0xFFFFFFFF, capacity >> 32
    if reserved is not None:
        ld.reserved[reserved] = 1
    return ld


def test_argument_errors_come_before_the_scene_and_the_device(miro):
    """Every MR_ERR_INVALID case on a host_only one-triangle scene: answered from the arguments alone, under this call's name,
    with the offending argument, before any device call, so "no HIP device" and "host_only" may not be what comes back.  Then
    MR_ERR_STATE for that scene, for an unbuilt one and for one without lights."""
    from miro_amd import binding
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.build(4, host_only=True)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    base = dict(scene=s.h, rays=p(4096), weights=None, pixels=None, n=64, rgb=p(8192), hits=None, ray_rgb=None, color=None, normal=None,
                out_rays=None, out_weights=None, out_pixels=None, out_count=None, counts=None)
    queue = dict(out_rays=p(1 << 16), out_weights=p(1 << 17), out_pixels=p(1 << 18), out_count=p(1 << 19))

    def call(ld, **kw):
        a = dict(base, **kw)
        st = L.mr_trace_level_lights(a["scene"], C.byref(ld) if ld is not None else None, a["rays"], a["weights"], a["pixels"], a["n"],
                                     a["rgb"], a["hits"], a["ray_rgb"], a["color"], a["normal"], a["out_rays"], a["out_weights"],
                                     a["out_pixels"], a["out_count"], a["counts"], None)
        return st, L.mr_last_error()

    ok = level_desc(binding)
    spec = level_desc(binding, children=binding.MR_LEVEL_SPECULAR, capacity=192)
    invalid = [
        ("NULL", call(ok, scene=None)), ("NULL", call(None)), ("NULL", call(ok, rays=None)),
        ("d_ray_rgb", call(ok, rgb=None)),
        ("spp", call(level_desc(binding, spp=0))),
        ("flags", call(level_desc(binding, flags=binding.MR_TRACE_ANY))), ("flags", call(level_desc(binding, flags=binding.MR_MATH_FAST))),
        ("flags", call(level_desc(binding, flags=1 << 30))),
        ("mr_gen_path_rays", call(level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=192), **queue)),
        ("children", call(level_desc(binding, children=7, capacity=192), **queue)),
        ("environment", call(level_desc(binding, environment=2))),
        ("reserved", call(level_desc(binding, reserved=0))), ("reserved", call(level_desc(binding, reserved=5))),
        ("output queue", call(spec)), ("output queue", call(spec, **dict(queue, out_count=None))),
        ("output queue", call(spec, **dict(queue, out_weights=None))),
        ("out_capacity", call(level_desc(binding, children=binding.MR_LEVEL_SPECULAR), **queue)),
        ("aligned", call(ok, rays=p(4096 + 8))), ("aligned", call(spec, **dict(queue, out_rays=p((1 << 16) + 4)))),
        ("aligned", call(ok, hits=p(2048 + 8))), ("aligned", call(ok, counts=p(4100))),
        ("aligned", call(spec, **dict(queue, out_count=p((1 << 19) + 4)))),
        ("aligned", call(ok, rgb=p(8194))), ("aligned", call(ok, ray_rgb=p(4098))), ("aligned", call(ok, color=p(4098))),
        ("aligned", call(ok, normal=p(4097))), ("aligned", call(ok, weights=p(4098))), ("aligned", call(ok, pixels=p(4097))),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and NAME.encode() in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    st, msg = call(ok)                                                            # then the scene's state: never a CPU path
    assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg
    st, msg = call(ok, rgb=None, ray_rgb=p(4096))                                 # d_rgb may be NULL when d_ray_rgb is given
    assert st == binding.MR_ERR_STATE, msg
    unbuilt = miro.Scene()
    unbuilt.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    st, msg = call(ok, scene=unbuilt.h)                                           # unbuilt, and without lights
    assert st == binding.MR_ERR_STATE and b"mr_bvh_build" in msg, msg
    st, msg = call(level_desc(binding, spp=0), scene=unbuilt.h)
    assert st == binding.MR_ERR_INVALID and b"spp" in msg and NAME.encode() in msg  # still the arguments first
    s.set_lights([])                                                              # host_only without lights: still the scene's state
    st, msg = call(ok)
    assert st == binding.MR_ERR_STATE and b"HIP device" not in msg, msg
    assert s.info().n_triangles == 1                                              # the refused calls left the scene alone


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
_FLOWER = {}


def use(miro, name, env):
    """(scene, description, lights) of a test scene (built once per session) with its lights and the environment ENVS[env] set"""
    from miro_amd import scenes
    if name == "flower_drops":
        if not _FLOWER:
            s = miro.Scene(0)
            desc = scenes.flower_setup(s, scenes.flower_scene(drops=True))
            _FLOWER["s"] = (s, desc, desc["lights"])
        scene, desc, lights = _FLOWER["s"]
    else:
        scene, desc, lights = scene_of(miro, name)
    scene.set_lights(lights)
    scene.set_environment(**(ENVS[env] or {}))
    return scene, desc, lights


def eye_queue(scene, desc, w=W, h=H, spp=SPP):
    import torch
    rays = torch.empty((w * h * spp, 8), dtype=torch.float32, device="cuda")
    scene.gen_eye_rays(camera(desc), w, h, rays, spp=spp, jitter=spp > 1, seed=168)
    return rays


class Chain:
    """The batched chain of one level: hit records, the surface pass's colour and normal (rows of rays that missed keep the
    sentinel), the expected per-ray L (the light chain's row of a hit, the environment chain's row of a miss, 0 without an
    environment), the pixel sums, the counters and the children"""

    def __init__(self, scene, n_lights, rays, weights, pixels, n, spp, flags, env, children, n_pixels):
        import torch
        f32 = dict(dtype=torch.float32, device="cuda")
        i64 = dict(dtype=torch.int64, device="cuda")
        self.n = n
        self.hits = torch.empty((n, 4), **f32)
        self.color, self.normal, lights_rgb, env_rgb = (torch.full((n, 3), SENTINEL, **f32) for _ in range(4))
        self.rgb = torch.zeros((n_pixels, 3), **f32)
        undefined, shadow, envc, count = torch.zeros(1, **i64), torch.zeros(1, **i64), torch.zeros(2, **i64), torch.zeros(1, **i64)
        scene.trace_device(rays, n, self.hits, flags)
        scene.hit_surface(rays, self.hits, n, self.color, self.normal, d_counts=undefined)
        scene.shade_lights_surface(rays, self.hits, self.color, self.normal, n, self.rgb, d_weights=weights, d_pixels=pixels, spp=spp,
                                   flags=flags, d_ray_rgb=lights_rgb, d_counts=shadow)
        if env:
            scene.shade_environment(rays, self.hits, n, self.rgb, d_weights=weights, d_pixels=pixels, spp=spp, flags=0,
                                    d_ray_rgb=env_rgb, d_counts=envc)
        self.out = None
        if children:
            self.out = (torch.empty((3 * n, 8), **f32), torch.empty((3 * n, 3), **f32), torch.empty(3 * n, dtype=torch.int32, device="cuda"))
            scene.gen_secondary_rays(rays, self.hits, weights, pixels, n, *self.out, count, spp=spp)
        torch.cuda.synchronize()
        self.hit_rows = self.hits[:, 1].contiguous().view(torch.int32) != -1
        self.n_hits = int(self.hit_rows.sum().item())
        self.ray_rgb = torch.where(self.hit_rows[:, None], lights_rgb, env_rgb if env else torch.zeros_like(env_rgb))
        assert int(shadow.item()) == self.n_hits * n_lights
        if env:
            assert int(envc[0].item()) == n - self.n_hits
        self.counted = (n, int(shadow.item()), int(undefined.item()), n - self.n_hits, int(envc[1].item()))
        self.n_children = int(count.item())
        if children:
            self.out = tuple(o[:self.n_children].contiguous() for o in self.out)


class Fused:
    """One mr_trace_level_lights call with every optional output, each per-ray buffer `rows` long (at least n + 1: a sentinel row
    past the end) and the output queue `slots` long, all filled with sentinels first"""

    def __init__(self, scene, rays, weights, pixels, n, spp, flags, env, children, n_pixels, rows=None, slots=None, capacity=None,
                 rgb=True, stream=None):
        import torch
        from miro_amd import binding
        f32 = dict(dtype=torch.float32, device="cuda")
        rows = n + 1 if rows is None else rows
        slots = 3 * n if slots is None else slots
        self.n = n
        self.rgb = torch.zeros((n_pixels, 3), **f32) if rgb else None
        self.hits = torch.full((rows, 4), SENTINEL, **f32)
        self.ray_rgb, self.color, self.normal = (torch.full((rows, 3), SENTINEL, **f32) for _ in range(3))
        self.counts = torch.tensor(COUNTS0, dtype=torch.int64, device="cuda")
        self.count = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
        self.out = None
        if children:
            self.out = (torch.full((slots, 8), SENTINEL, **f32), torch.full((slots, 3), SENTINEL, **f32),
                        torch.full((slots,), PIX, dtype=torch.int32, device="cuda"))
        self.launch = lambda st=stream: scene.trace_level_lights(
            rays, weights, pixels, n, self.rgb, children=binding.MR_LEVEL_SPECULAR if children else binding.MR_LEVEL_LAST,
            environment=bool(env), d_hits=self.hits, d_ray_rgb=self.ray_rgb, d_color=self.color, d_normal=self.normal,
            d_out_rays=self.out[0] if children else None, d_out_weights=self.out[1] if children else None,
            d_out_pixels=self.out[2] if children else None, d_out_count=self.count if children else None, d_counts=self.counts,
            spp=spp, flags=flags, stream=st, out_capacity=capacity)
        self.launch()
        torch.cuda.synchronize()
        for t in (self.hits, self.ray_rgb, self.color, self.normal):
            assert bool((t[n:] == SENTINEL).all()), "written beyond the end"
        self.counted = tuple(int(c) - c0 for c, c0 in zip(self.counts.cpu().numpy(), COUNTS0))
        self.n_children = int(self.count.item()) if children else 0

    def children(self, m=None):
        return tuple(o[:self.n_children if m is None else m] for o in self.out)


def rows_of(queue):
    return canon(*[o.cpu().numpy() for o in queue])


def assert_level_is_the_chain(fu, ch, exact_rgb=False):
    """hit records on their bits; colour and normal, the rows of misses untouched; per-ray L; all five counters; the children as
    sets; the pixel sums within the float-atomic bound of tests/test_level.py -- nothing left out"""
    import torch
    n = ch.n
    assert fu.n == n
    assert np.array_equal(bits(fu.hits[:n]), bits(ch.hits))
    assert same(fu.color[:n][ch.hit_rows], ch.color[ch.hit_rows]) and same(fu.normal[:n][ch.hit_rows], ch.normal[ch.hit_rows])
    assert bool((fu.color[:n][~ch.hit_rows] == SENTINEL).all()) and bool((fu.normal[:n][~ch.hit_rows] == SENTINEL).all())
    assert same(fu.ray_rgb[:n], ch.ray_rgb)
    assert fu.counted == ch.counted, (fu.counted, ch.counted)
    if ch.out is not None:
        assert fu.n_children == ch.n_children
        assert np.array_equal(rows_of(fu.children()), rows_of(ch.out))
    scale = float(ch.rgb.abs().max())
    if exact_rgb:
        assert same(fu.rgb, ch.rgb)
    assert torch.allclose(fu.rgb, ch.rgb, rtol=1e-5, atol=1e-6 * scale), float((fu.rgb - ch.rgb).abs().max())


def run_levels(miro, name, env, flags, depth=3):
    """depth + 1 levels on the same queues, the batched queue feeding the next level; returns per level (rays, hits, misses,
    children) and the number of lights"""
    from miro_amd import binding
    scene, desc, lights = use(miro, name, env)
    rays, weights, pixels, n = eye_queue(scene, desc), None, None, W * H * SPP
    seen = []
    for level in range(depth + 1):
        fl = flags | (binding.MR_TRACE_INCOHERENT if level > 0 else 0)
        children = level < depth
        ch = Chain(scene, len(lights), rays, weights, pixels, n, SPP, fl, ENVS[env], children, W * H)
        fu = Fused(scene, rays, weights, pixels, n, SPP, fl, ENVS[env], children, W * H)
        print("%s env=%s flags=%d level %d: %d rays, %d hits, %d children, counters %s, max %.4g" %
              (name, env, flags, level, n, ch.n_hits, ch.n_children, ch.counted, float(ch.rgb.max())))
        assert_level_is_the_chain(fu, ch)
        seen.append((n, ch.n_hits, n - ch.n_hits, ch.n_children))
        if not children or ch.n_children == 0:
            break
        rays, weights, pixels, n = ch.out[0], ch.out[1], ch.out[2], ch.n_children
    return seen, len(lights)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "stone"])
def test_level_by_level_in_the_rooms(miro, name):
    """mixed: the closed room with glass and mirror spheres, a glossy checker plane and five texture kinds under a disc and a
    point light (kTraceExactObj); stone: bump-mapped floor and walls, whose children bounce about the un-bumped normal.  No
    environment: a miss (there is none in a closed room at level 0, a few rays leak later) is worth 0.  Children really occur."""
    seen, n_lights = run_levels(miro, name, None, 0)
    assert n_lights == 2 and len(seen) == 4
    assert sum(s[3] for s in seen) >= 1000
    assert seen[0][1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 1 << 6], ids=["exact", "product"])
@pytest.mark.parametrize("env", ["colour", "image"])
def test_level_by_level_on_the_open_textured_teapot(miro, env, flags):
    """teapot_textured: triangles only (kTraceExact, then kTraceVote from level 1 on), a glossy LEAF teapot on a CHECKER floor
    under four point lights: reflect children, and rays that leave the scene at levels 0 and 1 -- worth bg_color, or the lookup of
    a 48 x 24 image under the rotation of assignment3.cpp:51.  flags 1 << 6 = MR_MATH_PRODUCT."""
    from miro_amd import binding
    assert flags in (0, binding.MR_MATH_PRODUCT)
    seen, n_lights = run_levels(miro, "teapot_textured", env, flags)
    assert n_lights == 4 and len(seen) >= 2
    assert seen[0][2] > 0 and seen[1][2] > 0 and seen[0][3] > 0


@pytest.mark.gpu
def test_level_by_level_without_a_texture_table(miro):
    """teapot: no table, every hit plain Phong; the default material has no children, so the recursion ends after level 0"""
    seen, n_lights = run_levels(miro, "teapot", "colour", 0)
    assert n_lights == 4 and seen[0][1] > 0 and seen[0][2] > 0


@pytest.mark.gpu
def test_level_by_level_on_the_flower_with_drops(miro):
    """the reference's final scene with glass spheres on its petals: petal, stem, leaf and flower-centre textures under a disc
    light, refract and Fresnel children from the drops, a background colour for the rays that leave"""
    seen, n_lights = run_levels(miro, "flower_drops", "colour", 0)
    assert n_lights == 1 and seen[0][3] > 0 and seen[0][2] > 0


@pytest.mark.gpu
def test_one_ray_per_pixel_is_one_add_per_pixel(miro):
    """teapot_textured at 1 spp, level 0, NULL weights and pixels: every pixel receives one addition, so d_rgb is the chain's bit
    for bit.  With d_rgb NULL the per-ray outputs are unchanged."""
    scene, desc, lights = use(miro, "teapot_textured", "image")
    n = W * H
    rays = eye_queue(scene, desc, spp=1)
    ch = Chain(scene, len(lights), rays, None, None, n, 1, 0, ENVS["image"], True, n)
    fu = Fused(scene, rays, None, None, n, 1, 0, ENVS["image"], True, n)
    assert_level_is_the_chain(fu, ch, exact_rgb=True)
    assert float(ch.rgb.max()) > 0 and ch.counted[3] > 0
    no_rgb = Fused(scene, rays, None, None, n, 1, 0, ENVS["image"], False, n, rgb=False)
    assert same(no_rgb.ray_rgb, fu.ray_rgb) and np.array_equal(bits(no_rgb.hits), bits(fu.hits)) and no_rgb.counted == fu.counted


@pytest.mark.gpu
def test_partial_last_workgroup(miro):
    """n = 9 600 - 37 rays through explicit d_pixels (9 563 = 37 workgroups of 256 and 91 lanes): the chain on the same n; rows
    past n of every optional output keep the sentinel (Fused checks them: its buffers are 9 601 rows long)"""
    import torch
    scene, desc, lights = use(miro, "teapot_textured", "colour")
    rays = eye_queue(scene, desc)
    n = W * H * SPP - 37
    pixels = (torch.arange(W * H * SPP, device="cuda") // SPP).to(torch.int32)
    ch = Chain(scene, len(lights), rays, None, pixels, n, SPP, 0, ENVS["colour"], True, W * H)
    fu = Fused(scene, rays, None, pixels, n, SPP, 0, ENVS["colour"], True, W * H, rows=W * H * SPP + 1)
    assert_level_is_the_chain(fu, ch)
    assert ch.n_children > 0 and bool((fu.hits[n:] == SENTINEL).all())


@pytest.mark.gpu
def test_capacity(miro):
    """out_capacity = count - 5: d_out_count still holds count, the first count - 5 slots hold members of the expected set, each
    once, and the slots after them keep the sentinel"""
    scene, desc, lights = use(miro, "mixed", None)
    rays, n = eye_queue(scene, desc), W * H * SPP
    ch = Chain(scene, len(lights), rays, None, None, n, SPP, 0, None, True, W * H)
    count = ch.n_children
    assert count > 100
    fu = Fused(scene, rays, None, None, n, SPP, 0, None, True, W * H, slots=count + 3, capacity=count - 5)
    assert fu.n_children == count
    want = {r.tobytes() for r in rows_of(ch.out)}
    got = rows_of(fu.children(count - 5))
    assert len({r.tobytes() for r in got}) == count - 5 == len(got) and all(r.tobytes() in want for r in got)
    assert bool((fu.out[0][count - 5:] == SENTINEL).all()) and bool((fu.out[1][count - 5:] == SENTINEL).all())
    assert bool((fu.out[2][count - 5:] == PIX).all())
    assert same(fu.ray_rgb[:n], ch.ray_rgb) and fu.counted == ch.counted


@pytest.mark.gpu
def test_replays_from_a_captured_graph(miro):
    """After one warm call outside the capture (it uploads the texture table) one level of the mixed room with children is
    captured into a torch.cuda.graph and replayed twice, the outputs filled with sentinels and d_out_count with a wrong value
    before each replay: per-ray outputs and the child set equal the direct launch, d_out_count is zeroed by each replay."""
    import torch
    scene, desc, lights = use(miro, "mixed", None)
    rays, n = eye_queue(scene, desc), W * H * SPP
    ch = Chain(scene, len(lights), rays, None, None, n, SPP, 0, None, True, W * H)
    fu = Fused(scene, rays, None, None, n, SPP, 0, None, True, W * H)           # the warm call, a direct launch
    assert_level_is_the_chain(fu, ch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fu.launch(torch.cuda.current_stream())
    for _ in range(2):
        for t in (fu.hits, fu.ray_rgb, fu.color, fu.normal, fu.out[0], fu.out[1]):
            t.fill_(SENTINEL)
        fu.out[2].fill_(PIX)
        fu.count.fill_(999999)
        fu.rgb.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fu.n_children = int(fu.count.item())
        assert fu.n_children == ch.n_children
        assert np.array_equal(bits(fu.hits[:n]), bits(ch.hits)) and same(fu.ray_rgb[:n], ch.ray_rgb)
        assert same(fu.color[:n][ch.hit_rows], ch.color[ch.hit_rows]) and same(fu.normal[:n][ch.hit_rows], ch.normal[ch.hit_rows])
        assert np.array_equal(rows_of(fu.children()), rows_of(ch.out))
        assert torch.allclose(fu.rgb, ch.rgb, rtol=1e-5, atol=1e-6 * float(ch.rgb.abs().max()))


@pytest.mark.gpu
def test_an_empty_queue_and_the_scene_state_errors(miro):
    """n == 0 is MR_OK, launches nothing and zeroes d_out_count on a level with children; MR_ERR_STATE for a scene without lights
    and for one that is not built"""
    import torch
    from miro_amd import binding, scenes
    scene, desc, lights = use(miro, "mixed", None)
    rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
    rgb = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    out = (torch.empty((192, 8), dtype=torch.float32, device="cuda"), torch.empty((192, 3), dtype=torch.float32, device="cuda"),
           torch.empty(192, dtype=torch.int32, device="cuda"))
    count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    counts = torch.zeros(5, dtype=torch.int64, device="cuda")
    scene.trace_level_lights(rays, None, None, 0, rgb, children=binding.MR_LEVEL_SPECULAR, d_out_rays=out[0], d_out_weights=out[1],
                             d_out_pixels=out[2], d_out_count=count, d_counts=counts)
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and counts.tolist() == [0] * 5 and float(rgb.abs().max()) == 0.0
    scene.set_lights([])
    with pytest.raises(miro.MiroError) as e:
        scene.trace_level_lights(rays, None, None, 64, rgb)
    assert e.value.status == binding.MR_ERR_STATE and "no lights" in str(e.value) and NAME in str(e.value)
    scene.set_lights(lights)
    unbuilt = miro.Scene(0)
    scenes.populate(unbuilt, scenes.SCENES["teapot"])
    unbuilt.set_lights(lights)
    with pytest.raises(miro.MiroError) as e:
        unbuilt.trace_level_lights(rays, None, None, 64, rgb)
    assert e.value.status == binding.MR_ERR_STATE and "mr_bvh_build" in str(e.value)
    torch.cuda.synchronize()
    assert float(rgb.abs().max()) == 0.0


def whole_frame(miro, name, env, w, h, spp, depth=3):
    """render_specular(fused="lights") and the same call with fused=False: (per_level, pixels) of each, the renderer and the
    description"""
    import torch
    from miro_amd import frame
    scene, desc, lights = use(miro, name, env)
    fr = frame.FrameRenderer(scene, desc, w, h, spp=spp, tiled=False)
    fr.generate()
    out = []
    for fused in ("lights", False):
        per_level = fr.render_specular(depth=depth, lights=lights, environment=ENVS[env], fused=fused)
        torch.cuda.synchronize()
        out.append((per_level, fr.d_rgb.clone()))
    return out, fr, desc


def assert_frames_agree(out):
    (levels_f, rgb_f), (levels_b, rgb_b) = out
    print("per_level", levels_b, "max", float(rgb_b.max()))
    assert levels_f == levels_b and len(levels_b) > 1
    top = float(rgb_b.abs().max())
    assert top > 0 and float((rgb_f - rgb_b).abs().max()) <= 2e-5 * top, float((rgb_f - rgb_b).abs().max()) / top


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [("mixed", None), ("teapot_textured", "image")])
def test_whole_frames(miro, name, env):
    """render_specular(depth=3, fused="lights") against fused=False: the same rays and shadow rays per level, pixels within 2e-5 of
    the largest value (the bound tests/test_gather_level.py and tests/test_photon_build.py use for a multi-level frame)"""
    out, _, _ = whole_frame(miro, name, env, W, H, SPP)
    assert_frames_agree(out)


@pytest.mark.gpu
def test_whole_frame_of_the_flower_with_drops(miro):
    """flower_scene(drops=True) at 96 x 64, 1 spp: the frames agree, and level 0 emits at least 50 refract children -- every eye
    ray whose hit lies on a drop has exactly one (Scene.cpp:315-336), and only the drops have children in this scene"""
    out, fr, desc = whole_frame(miro, "flower_drops", "colour", 96, 64, 1)
    assert_frames_agree(out)
    prim = bits(fr.d_hits)[:, 1]                        # the batched run (the second) left level 0's records here
    hit = prim != MISS
    material = np.asarray(desc["prim_material"])[prim[hit]]
    refract = int((material == 4).sum())
    print("%d eye rays hit a drop; level 1 has %d rays" % (refract, out[1][0][1][0]))
    assert refract >= 50 and out[1][0][1][0] >= refract
