"""mr_render_level_lights -- the level-0 frame of mr_render_lights_environment that also writes the rays of level 1, in one launch
(csrc/mr_frame_level_lights.hip, include/miro_hip_render.h).

Two yardsticks, both entry points that earlier tests hold against the batched chains and the oracle:

  the frame half     mr_render_lights_environment on the same scene and descriptor: pixels, hit records, per-sample L, colour and
                     normal and all five counters, compared EXACTLY (`same`, bit patterns for the hit records);
  the children half  mr_trace_level_lights (MR_LEVEL_SPECULAR) / mr_trace_level_lights_path (MR_LEVEL_PATH, the same kinds, seed,
                     bounce 0) on the queue mr_gen_eye_rays[_tiled] makes for the same window, seed and order, with weights and
                     ids NULL and d_pixels = the window pixel of every sample: specular children as sorted record sets (ray, weight,
                     pixel), path children by child id (id, ray, weight, pixel, octant, and the low-res byte by id), d_out_count
                     exactly.

Every comparison first asserts on the yardstick side alone that the case is not empty: hits, misses where the scene is open, and
children of every kind the case claims.  Whole frames (render_specular(fused="frame_lights" | "frame_lights_path") against "lights"
| "lights_path") are held to the whole-frame bound of tests/test_level_lights.py, 2e-5 x the largest value."""
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
from test_frame_lights import MISS, SENTINEL, bits, camera, frame_desc, same  # noqa: E402
from test_level import canon  # noqa: E402
from test_level_lights import ENVS, use  # noqa: E402
from test_level_lights import Fused as SpecLevel  # noqa: E402
from test_level_lights_path import BYTE, ID, PIX, Q, child_id, glass_sphere, rows_of  # noqa: E402
from test_level_lights_path import Fused as PathLevel  # noqa: E402

F = np.float32
NAME = "mr_render_level_lights"
COUNTS0 = (1000, 5, 77, 31, 9)                          # what d_counts holds before a call: the call does not zero it
SPECULAR, PATH = 1, 2                                   # MR_LEVEL_SPECULAR, MR_LEVEL_PATH
GLASS_DESC = dict(eye=(0.0, 0.0, 5.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=30.0)


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_render_level_lights_is_exported_declared_and_bound(miro):
    """Fails on the parent commit: the symbol, the header and the fourth list are this feature's."""
    from miro_amd import binding

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return re.search(r"\bmr_status\s+%s\s*\(" % NAME, src) is not None

    assert hasattr(miro.lib(), NAME)
    assert declared("miro_hip_render.h")
    assert not declared("miro_hip.h") and not declared("miro_hip_surface.h") and not declared("miro_hip_frame.h")
    assert binding.RENDER_SYMBOLS == [NAME]
    assert NAME not in binding.FRAME_SYMBOLS and NAME not in binding.SURFACE_SYMBOLS and NAME not in miro.EXPORTED_SYMBOLS
    assert len(miro.EXPORTED_SYMBOLS) == 69 and len(binding.SURFACE_SYMBOLS) == 9 and len(binding.FRAME_SYMBOLS) == 3
    assert getattr(miro.lib(), NAME).restype is C.c_int32
    top = open(os.path.join(ROOT, "include", "miro_hip.h")).read()
    assert top.rstrip().endswith('#include "miro_hip_render.h"\n#endif /* MIRO_HIP_H */')
    assert hasattr(miro.Scene, "render_level_lights")


def test_frame_level_desc_matches_the_header(miro):
    """sizeof and the offsets of the two pointers, worked out from the header's own field list: twelve 32-bit words, two pointers"""
    from miro_amd import binding
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "miro_hip_render.h")).read(), flags=re.S)
    body = re.search(r"typedef struct mr_frame_level_desc \{(.*?)\} mr_frame_level_desc;", src, re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    words = 0
    for f in fields:
        if f.startswith("uint32_t"):
            for name in f[len("uint32_t"):].split(","):
                m = re.search(r"\[(\d+)\]", name)
                words += int(m.group(1)) if m else 1
    assert words == 12 and [f for f in fields if not f.startswith("uint32_t")] == ["uint8_t *d_out_octants", "uint8_t *d_out_lowres"]
    D = binding.FrameLevelDesc
    assert [n for n, _ in D._fields_] == ["children", "environment", "path_kinds", "path_seed", "out_capacity_lo", "out_capacity_hi",
                                          "reserved", "d_out_octants", "d_out_lowres"]
    assert C.sizeof(D) == 4 * words + 16 == 64 and D.d_out_octants.offset == 48 and D.d_out_lowres.offset == 56
    assert D.reserved.offset == 24 and D.reserved.size == 24


def test_frame_level_lights_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_frame_level_lights.hip: no dynamic stack; at least four waves per SIMD; no more spilled VGPRs, no more
    scratch per lane and no fewer waves than BOTH its own record (tests/golden/kernel_budget_frame_level_lights.json, written from
    the build whose GPU run of this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.
    Twelve frame kernels, one per traversal variant of with_trace_variant (six) and kind of children (specular, path tracing): the
    environment, the texture table and the optional outputs are wave-uniform branches.  The unit has no other kernel: the
    one-word store that zeroes d_out_count is mr_level_lights.hip's, held to that unit's record."""
    cur = kernel_budget.unit_kernels("mr_frame_level_lights")
    frame = [k for k in cur if "frame_level_lights_kernel" in k]
    assert len(frame) == 6 * 2
    assert sorted(set(cur) - set(frame)) == []
    for var in (1818, 826, 267, 43, 88, 73):                   # kTraceExact, ExactObj, Product, ProductObj, Vote, VoteProduct
        for children in (SPECULAR, PATH):
            assert sum("ILi%dELi%dEE" % (var, children) in k for k in cur) == 1, (var, children)
    assert not any(v["dynamic_stack"] for v in cur.values())
    assert all(v["waves_per_simd"] >= 4 for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_frame_level_lights.json", also_main=True)


def level_desc(binding, children=0, environment=0, kinds=7, capacity=0, reserved=None, octants=None, lowres=None):
    ld = binding.FrameLevelDesc()
    ld.children, ld.environment, ld.path_kinds, ld.path_seed = children, environment, kinds, 168
    ld.out_capacity_lo, ld.out_capacity_hi = capacity & 0xFFFFFFFF, capacity >> 32
    ld.d_out_octants, ld.d_out_lowres = octants, lowres
    if reserved is not None:
        ld.reserved[reserved] = 1
    return ld


def test_argument_errors_come_before_the_scene_and_the_device(miro):
    """Every MR_ERR_INVALID case on a host_only one-triangle scene: answered from the arguments alone, under this call's name,
    before any device call, so "no HIP device" and "host_only" may not be what comes back.  The frame call's own cases first, then
    the level calls'.  Octants and low-res bytes take any address.  Then MR_ERR_STATE for that scene, for an unbuilt one and for one
    without lights."""
    from miro_amd import binding
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.build(4, host_only=True)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    base = dict(scene=s.h, rgb=p(8192), hits=None, sample_rgb=None, color=None, normal=None, out_rays=None, out_weights=None,
                out_pixels=None, out_ids=None, out_count=None, counts=None)
    queue = dict(out_rays=p(1 << 16), out_weights=p(1 << 17), out_pixels=p(1 << 18), out_count=p(1 << 19))

    def call(fd, ld, **kw):
        a = dict(base, **kw)
        st = getattr(L, NAME)(a["scene"], C.byref(fd) if fd is not None else None, C.byref(ld) if ld is not None else None, a["rgb"],
                              a["hits"], a["sample_rgb"], a["color"], a["normal"], a["out_rays"], a["out_weights"], a["out_pixels"],
                              a["out_ids"], a["out_count"], a["counts"], None)
        return st, L.mr_last_error()

    fd = frame_desc(binding)
    last = level_desc(binding)
    spec = level_desc(binding, children=binding.MR_LEVEL_SPECULAR, capacity=256)
    path = level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=256)
    invalid = [
        # the frame call's, in its order
        ("NULL", call(fd, last, scene=None)), ("NULL", call(None, last)), ("NULL", call(fd, last, rgb=None)),
        ("empty image", call(frame_desc(binding, W=0), last)),
        ("spp", call(frame_desc(binding, spp=3), last)), ("spp", call(frame_desc(binding, spp=128), last)),
        ("band", call(frame_desc(binding, bands=(0, 0, 2)), last)), ("band", call(frame_desc(binding, bands=(2, 3, 3)), last)),
        ("rows", call(frame_desc(binding, y0=5, y1=3), last)), ("rows", call(frame_desc(binding, y1=9), last)),
        ("flags", call(frame_desc(binding, flags=binding.MR_MATH_FAST), last)), ("flags", call(frame_desc(binding, flags=1 << 30), last)),
        ("aligned", call(fd, last, hits=p(2048 + 8))), ("aligned", call(fd, last, counts=p(4100))), ("aligned", call(fd, last, rgb=p(8194))),
        ("aligned", call(fd, last, sample_rgb=p(4098))), ("aligned", call(fd, last, color=p(4098))), ("aligned", call(fd, last, normal=p(4097))),
        # then the level calls'
        ("NULL", call(fd, None)),
        ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY), last)),
        ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY), spec, **queue)),
        ("children", call(fd, level_desc(binding, children=7, capacity=256), **queue)),
        ("environment", call(fd, level_desc(binding, environment=2))),
        ("path_kinds", call(fd, level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=256, kinds=0), **queue)),
        ("path_kinds", call(fd, level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=256, kinds=8), **queue)),
        ("reserved", call(fd, level_desc(binding, reserved=0))), ("reserved", call(fd, level_desc(binding, reserved=5))),
        ("output queue", call(fd, spec)), ("output queue", call(fd, path, **dict(queue, out_count=None))),
        ("output queue", call(fd, spec, **dict(queue, out_weights=None))), ("output queue", call(fd, path, **dict(queue, out_rays=None))),
        ("output queue", call(fd, spec, **dict(queue, out_pixels=None))),
        ("out_capacity", call(fd, level_desc(binding, children=binding.MR_LEVEL_SPECULAR), **queue)),
        ("out_capacity", call(fd, level_desc(binding, children=binding.MR_LEVEL_PATH), **queue)),
        ("aligned", call(fd, spec, **dict(queue, out_rays=p((1 << 16) + 4)))), ("aligned", call(fd, path, **dict(queue, out_count=p((1 << 19) + 4)))),
        ("aligned", call(fd, spec, **dict(queue, out_weights=p((1 << 17) + 3)))), ("aligned", call(fd, spec, **dict(queue, out_pixels=p((1 << 18) + 2)))),
        ("aligned", call(fd, path, **dict(queue, out_ids=p((1 << 20) + 1)))),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and NAME.encode() in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    # the order: a frame error comes before a level error, a level error before the scene's state
    st, msg = call(frame_desc(binding, spp=3), level_desc(binding, children=7))
    assert st == binding.MR_ERR_INVALID and b"spp" in msg
    st, msg = call(fd, level_desc(binding, children=7, environment=2))
    assert st == binding.MR_ERR_INVALID and b"children" in msg
    for ld, kw in ((last, {}), (spec, queue), (path, dict(queue, out_ids=p(1 << 20)))):                  # then the scene's state: never a CPU path
        st, msg = call(fd, ld, **kw)
        assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg
    both = frame_desc(binding, flags=binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT)
    odd = level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=256, octants=(1 << 22) + 1, lowres=(1 << 21) + 3)
    st, msg = call(both, odd, **queue)                                            # bytes lie anywhere; both flags are legal; ids optional
    assert st == binding.MR_ERR_STATE and b"aligned" not in msg, msg
    st, msg = call(fd, level_desc(binding, kinds=0))                              # path_kinds is read with MR_LEVEL_PATH only
    assert st == binding.MR_ERR_STATE, msg
    st, msg = call(frame_desc(binding, y0=4, y1=4), level_desc(binding, children=binding.MR_LEVEL_SPECULAR), **queue)
    assert st == binding.MR_ERR_STATE, msg                                        # an empty window needs no capacity
    unbuilt = miro.Scene()
    unbuilt.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    st, msg = call(fd, spec, scene=unbuilt.h, **queue)                            # unbuilt, and without lights
    assert st == binding.MR_ERR_STATE and b"mr_bvh_build" in msg, msg
    st, msg = call(fd, level_desc(binding, environment=2), scene=unbuilt.h)
    assert st == binding.MR_ERR_INVALID and b"environment" in msg                 # still the arguments first
    s.set_lights([])                                                              # host_only without lights: still the scene's state
    st, msg = call(fd, spec, **queue)
    assert st == binding.MR_ERR_STATE and b"HIP device" not in msg, msg
    assert s.info().n_triangles == 1                                              # the refused calls left the scene alone


def test_renderer_without_resident_rays():
    """FrameRenderer(resident_rays=False) allocates no ray, hit or shadow buffer, reports what is left and refuses every method that
    needs them; the default is unchanged: 100 bytes per sample more."""
    import torch
    from miro_amd import frame
    from test_frame_plan import DESC, LIGHTS, RecordingScene
    w, h, spp = 16, 8, 2
    sc = RecordingScene(0, False, hit=(3, 4), child=(1, 2), image=False)
    full = frame.FrameRenderer(sc, DESC, w, h, spp=spp, device=torch.device("cpu"))
    lean = frame.FrameRenderer(sc, DESC, w, h, spp=spp, device=torch.device("cpu"), resident_rays=False)
    assert full.resident_rays and not lean.resident_rays
    assert full.bytes_resident() == w * h * spp * 100 + 8 + w * h * 12
    assert lean.bytes_resident() == 8 + w * h * 12 and lean.d_rays is None and lean.d_hits is None and lean.d_shadow_rays is None
    for call in (lean.generate, lean.trace_primary, lean.make_shadow_rays, lean.trace_shadow, lean.shade, lean.step, lean.capture,
                 lambda: lean.final_gather(None), lambda: lean.render_specular(depth=1),
                 lambda: lean.render_specular(depth=1, lights=LIGHTS, fused="lights"),
                 lambda: lean.render_specular(depth=1, lights=LIGHTS, fused="frame_lights", photon_maps=(object(), None))):
        with pytest.raises(ValueError, match="resident_rays"):
            call()
    assert all(c[0] == "set_lights" for c in sc.calls)              # no launch was made


# ---- on the MI355X: helpers ------------------------------------------------------------------------------------------------
def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def window_ranges(miro, H, y0, y1, bands):
    """the row ranges [a, b) of a window, in the order the frame keeps them"""
    if bands is None:
        return [(y0, H if y1 is None else y1)]
    rows, rank, world = bands
    return [(b * rows, min(b * rows + rows, H)) for b in range(rank, (H + rows - 1) // rows, world)]


class Level0:
    """One mr_render_level_lights call on the scene as it is set, with every optional output: each per-sample and per-pixel buffer
    one sentinel row longer than the contract says, the output queue `slots` long, all filled with sentinels first"""

    def __init__(self, miro, scene, desc, W, H, spp, tiled, children, env, flags=0, y0=0, y1=None, bands=None, kinds=7, path_seed=168,
                 slots=None, capacity=None):
        import torch
        rows = sum(b - a for a, b in window_ranges(miro, H, y0, y1, bands))
        self.n, self.n_pixels, self.children = rows * W * spp, rows * W, children
        n = self.n
        slots = max(4 * n, 1) if slots is None else slots
        f32 = dict(dtype=torch.float32, device="cuda")
        self.rgb = torch.full((self.n_pixels + 1, 3), SENTINEL, **f32)
        self.hits = torch.full((n + 1, 4), SENTINEL, **f32)
        self.sample_rgb, self.color, self.normal = (torch.full((n + 1, 3), SENTINEL, **f32) for _ in range(3))
        self.counts = torch.tensor(COUNTS0 + (4242,), dtype=torch.int64, device="cuda")       # a sixth word: never touched
        self.count = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
        self.out = (torch.full((slots, 8), SENTINEL, **f32), torch.full((slots, 3), SENTINEL, **f32),
                    torch.full((slots,), PIX, dtype=torch.int32, device="cuda"), torch.full((slots,), ID, dtype=torch.int32, device="cuda"),
                    torch.full((slots,), BYTE, dtype=torch.uint8, device="cuda"))
        self.out_low = torch.full((slots,), BYTE, dtype=torch.uint8, device="cuda")
        o = self.out if children else (None,) * 5
        self.launch = lambda st=None: scene.render_level_lights(
            camera(desc), W, H, self.rgb, y0=y0, y1=y1, bands=bands, spp=spp, jitter=spp > 1, seed=168, tiled=tiled, flags=flags,
            d_hits=self.hits, d_sample_rgb=self.sample_rgb, d_sample_color=self.color, d_sample_normal=self.normal, d_counts=self.counts,
            stream=st, children=children, environment=bool(env), kinds=kinds, path_seed=path_seed, d_out_rays=o[0], d_out_weights=o[1],
            d_out_pixels=o[2], d_out_ids=o[3], d_out_count=self.count if children else None, out_capacity=capacity, d_out_octants=o[4],
            d_out_lowres=self.out_low if children else None)
        self.launch()
        torch.cuda.synchronize()
        self.read()

    def read(self):
        for t, k in ((self.rgb, self.n_pixels), (self.hits, self.n), (self.sample_rgb, self.n), (self.color, self.n), (self.normal, self.n)):
            assert bool((t[k:] == SENTINEL).all()), "written beyond the end"
        c = self.counts.cpu().numpy()
        assert int(c[5]) == 4242, "written beyond the fifth counter"
        self.counted = tuple(int(v) - v0 for v, v0 in zip(c, COUNTS0))
        self.n_children = int(self.count.item()) if self.children else 0

    def spec_rows(self, m=None):
        m = self.n_children if m is None else m
        return canon(*[o[:m].cpu().numpy() for o in self.out[:3]])

    def path_rows(self, m=None):
        return rows_of(self.out, self.n_children if m is None else m)

    def low_by_id(self, m=None):
        m = self.n_children if m is None else m
        ids, low = self.out[3][:m].cpu().numpy().view(np.uint32), self.out_low[:m].cpu().numpy()
        order = np.argsort(ids, kind="stable")
        return ids[order], low[order]

    def untouched(self, m):
        """slots [m, end) of every output column still hold the sentinels (SPECULAR: ids and the low-res byte everywhere)"""
        k = m if self.children == PATH else 0
        return (bool((self.out[0][m:] == SENTINEL).all()) and bool((self.out[1][m:] == SENTINEL).all()) and bool((self.out[2][m:] == PIX).all())
                and bool((self.out[3][k:] == ID).all()) and bool((self.out[4][m:] == BYTE).all()) and bool((self.out_low[k:] == BYTE).all()))


class EnvFrame:
    """mr_render_lights_environment on the scene as it is set: the yardstick of the frame half"""

    def __init__(self, miro, scene, desc, W, H, spp, tiled, flags=0, y0=0, y1=None, bands=None):
        import torch
        rows = sum(b - a for a, b in window_ranges(miro, H, y0, y1, bands))
        self.n, self.n_pixels = rows * W * spp, rows * W
        f32 = dict(dtype=torch.float32, device="cuda")
        self.rgb = torch.full((self.n_pixels + 1, 3), SENTINEL, **f32)
        self.hits = torch.full((self.n + 1, 4), SENTINEL, **f32)
        self.sample_rgb, self.color, self.normal = (torch.full((self.n + 1, 3), SENTINEL, **f32) for _ in range(3))
        self.counts = torch.tensor(COUNTS0, dtype=torch.int64, device="cuda")
        scene.render_lights_environment(camera(desc), W, H, self.rgb, y0=y0, y1=y1, bands=bands, spp=spp, jitter=spp > 1, seed=168,
                                        tiled=tiled, flags=flags, d_hits=self.hits, d_sample_rgb=self.sample_rgb,
                                        d_sample_color=self.color, d_sample_normal=self.normal, d_counts=self.counts)
        torch.cuda.synchronize()
        self.counted = tuple(int(v) - v0 for v, v0 in zip(self.counts.cpu().numpy(), COUNTS0))
        prim = self.hits[:self.n, 1].contiguous().view(torch.int32)
        self.n_hits = int((prim != -1).sum().item())


def assert_frame_half(fu, env_frame, open_scene=True, lit=True):
    """every output of the frame half and all five counters, bit for bit; the yardstick has hits, misses in an open scene, and
    light in its pixels (lit=False: a surface without a diffuse term may stay black)"""
    e = env_frame
    assert e.n_hits > 0 and (not open_scene or e.n_hits < e.n) and e.counted[0] == e.n and e.counted[3] == e.n - e.n_hits
    assert not lit or float(e.rgb[:e.n_pixels].max()) > 0
    assert fu.n == e.n and fu.n_pixels == e.n_pixels
    assert np.array_equal(bits(fu.hits), bits(e.hits))
    for f in ("rgb", "sample_rgb", "color", "normal"):
        assert same(getattr(fu, f), getattr(e, f)), f
    assert fu.counted == e.counted, (fu.counted, e.counted)


def eye_queue(miro, scene, desc, W, H, spp, tiled, y0=0, y1=None, bands=None):
    """the queue mr_gen_eye_rays[_tiled] makes for the window, range by range in the frame's order, and the window pixel of every
    sample: (rays, pixels, n)"""
    import torch
    from miro_amd import binding
    ranges = window_ranges(miro, H, y0, y1, bands)
    n = sum(b - a for a, b in ranges) * W * spp
    rays = torch.empty((max(n, 1), 8), dtype=torch.float32, device="cuda")
    pix, off = [], 0
    for a, b in ranges:
        k = (b - a) * W * spp
        scene.gen_eye_rays(camera(desc), W, H, rays[off:off + k], y0=a, y1=b, spp=spp, jitter=spp > 1, seed=168, tiled=tiled)
        slot = np.arange(k, dtype=np.int64) // spp
        if tiled:
            slot = binding.tile_pixel_map(W, b - a, spp).astype(np.int64)[slot]
        pix.append(slot + off // spp)
        off += k
    return rays, cuda(np.concatenate(pix).astype(np.int32)), n


def spec_level(miro, scene, desc, W, H, spp, tiled, env, flags=0, **window):
    rays, pixels, n = eye_queue(miro, scene, desc, W, H, spp, tiled, **window)
    return SpecLevel(scene, rays, None, pixels, n, spp, flags, env, True, n // spp)


def path_level(miro, scene, desc, W, H, spp, tiled, env, kinds, flags=0, path_seed=168, **window):
    rays, pixels, n = eye_queue(miro, scene, desc, W, H, spp, tiled, **window)
    return PathLevel(scene, Q(rays, None, pixels, None, None, n), spp, flags, env, n // spp, kinds=kinds, seed=path_seed, bounce=0)


def path_kinds_of(lv):
    """children of each kind 0..3 of a path level, counted from their ids (ids NULL: a parent's id is its index)"""
    got = lv.out[3][:lv.n_children].cpu().numpy().view(np.uint32)
    hit = np.nonzero(bits(lv.hits[:lv.n])[:, 1] != MISS)[0].astype(np.uint32)
    return [int(np.isin(child_id(hit, k), got).sum()) for k in range(4)]


def assert_spec_children(fu, lv):
    """the yardstick has children; then d_out_count and the sorted record sets are equal and nothing lies past the count"""
    assert lv.n_children > 0 and lv.n == fu.n
    assert fu.n_children == lv.n_children
    assert np.array_equal(fu.spec_rows(), canon(*[o.cpu().numpy() for o in lv.children()]))
    assert fu.untouched(fu.n_children)


def assert_path_children(fu, lv):
    """the yardstick has children; then d_out_count, the records by child id and the low-res bytes by id are equal"""
    assert lv.n_children > 0 and lv.n == fu.n
    assert fu.n_children == lv.n_children
    mine = fu.path_rows()
    assert len(np.unique(mine[:, 0])) == fu.n_children and np.array_equal(mine, lv.rows())
    m = lv.n_children
    ids, low = lv.out[3][:m].cpu().numpy().view(np.uint32), lv.out_low[:m].cpu().numpy()
    order = np.argsort(ids, kind="stable")
    got_ids, got_low = fu.low_by_id()
    assert np.array_equal(got_ids, ids[order]) and np.array_equal(got_low, low[order]) and set(np.unique(low)) <= {0, 1}
    assert fu.untouched(fu.n_children)


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("env", [None, "colour", "image"])
@pytest.mark.parametrize("name", ["teapot_textured", "flower", "teapot"])
def test_frame_half_is_mr_render_lights_environment(miro, name, env):
    """48 x 32 at 1, 2 and 4 spp in image and in tiled order, for both kinds of children: every output and all five counters equal
    mr_render_lights_environment's on the same descriptor.  With env None the call runs with environment == 0 on a scene whose
    environment is a colour: the yardstick is the frame of the scene with NO environment (mr_render_lights_surface's outputs, the
    misses still counted)."""
    W, H = 48, 32
    for spp in (1, 2, 4):
        for tiled in (False, True):
            scene, desc, lights = use(miro, name, env)
            want = EnvFrame(miro, scene, desc, W, H, spp, tiled)
            if env is None:
                scene.set_environment(**ENVS["colour"])          # must not show: environment == 0
            for children in (SPECULAR, PATH):
                fu = Level0(miro, scene, desc, W, H, spp, tiled, children, env)
                assert_frame_half(fu, want)
    use(miro, name, None)


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [1, 2, 3, 4, 5, 6, 7])
def test_every_kind_in_the_mixed_room(miro, kinds):
    """The closed room with glass and mirror spheres, a glossy checker plane and five texture kinds, 64 x 32 x 1: the path children
    of every path_kinds under another seed than the default, by child id; with kinds == 7 also at 2 spp in tiled order, and the
    specular children as sets."""
    scene, desc, lights = use(miro, "mixed", None)
    for W, H, spp, tiled in [(64, 32, 1, False)] + ([(48, 32, 2, True)] if kinds == 7 else []):
        lv = path_level(miro, scene, desc, W, H, spp, tiled, None, kinds, path_seed=29)
        per = path_kinds_of(lv)
        print("mixed room kinds %d %dx%dx%d tiled=%s: children per kind %s" % (kinds, W, H, spp, tiled, per))
        for bit, kind in {1: 0, 2: 2, 4: 3}.items():
            assert (per[kind] > 0) == bool(kinds & bit), (kinds, per)
        assert (per[1] > 0) == bool(kinds & 2) and sum(per) == lv.n_children
        fu = Level0(miro, scene, desc, W, H, spp, tiled, PATH, None, kinds=kinds, path_seed=29)
        assert_path_children(fu, lv)
        assert_frame_half(fu, EnvFrame(miro, scene, desc, W, H, spp, tiled), open_scene=False)
        if kinds == 7:
            sp = spec_level(miro, scene, desc, W, H, spp, tiled, None)
            assert_spec_children(Level0(miro, scene, desc, W, H, spp, tiled, SPECULAR, None), sp)


@pytest.mark.gpu
def test_fresnel_children_and_capacity_on_a_glass_sphere(miro):
    """The glass sphere (kd = 0, ks, kt = 0.9, index 1.5) seen from outside at 64 x 48 x 1, from normal to grazing incidence: every
    hit has a mirror and a refract child, and a Fresnel child where Rs > 0.01 -- parents with two and with three children both
    occur (at 1 spp a child's pixel names its parent).  Both kinds of children equal the level kernels'.  Then out_capacity =
    count - 5 into buffers three slots longer than count: d_out_count still holds count, the stored slots are members of the full
    set, each once, and every column from the capacity on keeps its sentinel; the frame half is unchanged."""
    s = glass_sphere(miro)
    W, H = 64, 48
    sp = spec_level(miro, s, GLASS_DESC, W, H, 1, False, None)
    per_parent = np.bincount(np.bincount(sp.children()[2].cpu().numpy(), minlength=W * H))
    n_hits = int((bits(sp.hits[:sp.n])[:, 1] != MISS).sum())
    print("glass sphere: %d hits of %d, parents with k children %s" % (n_hits, sp.n, per_parent.tolist()))
    assert 0 < n_hits < sp.n and len(per_parent) == 4 and per_parent[1] == 0 and per_parent[2] > 20 and per_parent[3] > 20
    fu = Level0(miro, s, GLASS_DESC, W, H, 1, False, SPECULAR, None)
    assert_spec_children(fu, sp)
    lv = path_level(miro, s, GLASS_DESC, W, H, 1, False, None, 7)
    per = path_kinds_of(lv)
    assert per[0] == n_hits and per[2] == n_hits and per[3] == 0 and 20 < per[1] < n_hits - 20, per
    fp = Level0(miro, s, GLASS_DESC, W, H, 1, False, PATH, None)
    assert_path_children(fp, lv)
    want = EnvFrame(miro, s, GLASS_DESC, W, H, 1, False)
    assert_frame_half(fu, want, lit=False)
    assert_frame_half(fp, want, lit=False)
    for children, full in ((SPECULAR, fu), (PATH, fp)):
        count = full.n_children
        part = Level0(miro, s, GLASS_DESC, W, H, 1, False, children, None, slots=count + 3, capacity=count - 5)
        assert part.n_children == count and part.untouched(count - 5)
        rows, got = (full.spec_rows(), part.spec_rows(count - 5)) if children == SPECULAR else (full.path_rows(), part.path_rows(count - 5))
        have = {row.tobytes() for row in rows}
        assert len({row.tobytes() for row in got}) == count - 5 and all(row.tobytes() in have for row in got)
        assert_frame_half(part, want, lit=False)


@pytest.mark.gpu
def test_stone_floor_children_leave_about_the_bumped_normal(miro):
    """The stone room at 48 x 32 x 1: the path children equal the level kernel's, whose own test shows that a floor hit's diffuse
    child leaves about the bumped normal; here, besides, every diffuse child's weight is its parent's looked-up colour (w0 = 1) bit
    for bit and its pixel is its parent's.  The specular children (the spheres') as sets."""
    scene, desc, lights = use(miro, "stone", None)
    W, H = 48, 32
    lv = path_level(miro, scene, desc, W, H, 1, False, None, 7)
    per = path_kinds_of(lv)
    assert per[3] > W * H // 8 and per[0] > 0, per
    fu = Level0(miro, scene, desc, W, H, 1, False, PATH, None)
    assert_path_children(fu, lv)
    rows = fu.path_rows()
    parents = np.arange(fu.n, dtype=np.uint32)
    hit = bits(fu.hits[:fu.n])[:, 1] != MISS
    want_id = child_id(parents[hit], 3)
    slot = np.searchsorted(rows[:, 0], want_id)
    found = (slot < len(rows)) & (rows[np.minimum(slot, len(rows) - 1), 0] == want_id)
    assert found.sum() == per[3]
    col = fu.color[:fu.n].cpu().numpy()[hit][found]
    assert rows[slot[found], 9:12].tobytes() == col.astype(F).view(np.uint32).tobytes()
    assert np.array_equal(rows[slot[found], 12], parents[hit][found])             # pixel = sample index at 1 spp, image order
    sp = spec_level(miro, scene, desc, W, H, 1, False, None)
    assert_spec_children(Level0(miro, scene, desc, W, H, 1, False, SPECULAR, None), sp)


@pytest.mark.gpu
def test_flower_with_drops_under_an_image(miro):
    """flower_scene(drops=True) under the 48 x 24 image at 48 x 32 x 2: hits and misses; water has kd and kt, no ks -- refract,
    Fresnel and diffuse children, whose low-res byte is 1 exactly on the diffuse ones; the specular children as sets; the frame
    half with its environment lookups."""
    scene, desc, lights = use(miro, "flower_drops", "image")
    W, H, spp = 48, 32, 2
    lv = path_level(miro, scene, desc, W, H, spp, False, ENVS["image"], 7)
    per = path_kinds_of(lv)
    print("flower with drops: children per kind", per)
    assert per[2] > 0 and per[3] > 0, per
    fu = Level0(miro, scene, desc, W, H, spp, False, PATH, "image")
    assert_path_children(fu, lv)
    ids, low = fu.low_by_id()
    hit = np.nonzero(bits(fu.hits[:fu.n])[:, 1] != MISS)[0].astype(np.uint32)
    assert np.array_equal(low == 1, np.isin(ids, child_id(hit, 3))) and 0 < int(low.sum()) < len(low)
    want = EnvFrame(miro, scene, desc, W, H, spp, False)
    assert_frame_half(fu, want)
    sp = spec_level(miro, scene, desc, W, H, spp, False, ENVS["image"])
    fs = Level0(miro, scene, desc, W, H, spp, False, SPECULAR, "image")
    assert_spec_children(fs, sp)
    assert_frame_half(fs, want)


@pytest.mark.gpu
def test_shapes_where_it_can_go_wrong(miro):
    """On the textured teapot under the image (mirror children, hits and misses), both kinds of children and the frame half at
      37 x 13 x 1   481 samples: a partial last workgroup, whose lanes past the end are neither misses nor parents;
      rows [9, 21) of 48 x 32 x 2   a window inside the image: the children's pixels index this call's d_rgb;
      bands of 5 rows, rank 1 of 3, of 48 x 32 x 2   rows 5-9 and 20-24: likewise, in band order;
      8 x 4 x 64    one pixel per wave, the butterfly at full width;
    and an empty window: MR_OK, d_out_count zeroed, nothing else written."""
    scene, desc, lights = use(miro, "teapot_textured", "image")
    cases = [(37, 13, 1, {}), (48, 32, 2, dict(y0=9, y1=21)), (48, 32, 2, dict(bands=(5, 1, 3))), (8, 4, 64, {})]
    for W, H, spp, window in cases:
        want = EnvFrame(miro, scene, desc, W, H, spp, False, **window)
        sp = spec_level(miro, scene, desc, W, H, spp, False, ENVS["image"], **window)
        lv = path_level(miro, scene, desc, W, H, spp, False, ENVS["image"], 3, **window)
        assert path_kinds_of(lv)[0] > 0
        top = int(sp.children()[2].max().item())
        assert top < want.n_pixels and (not window or top >= want.n_pixels // 2)         # window pixels, up to the window's end
        fs = Level0(miro, scene, desc, W, H, spp, False, SPECULAR, "image", **window)
        assert_frame_half(fs, want, open_scene=not window)                                # (a window may see the teapot alone)
        assert_spec_children(fs, sp)
        fp = Level0(miro, scene, desc, W, H, spp, False, PATH, "image", kinds=3, **window)
        assert_frame_half(fp, want, open_scene=not window)
        assert_path_children(fp, lv)
    assert window_ranges(miro, 32, 0, None, (5, 1, 3)) == [(5, 10), (20, 25)]
    for children in (SPECULAR, PATH):
        empty = Level0(miro, scene, desc, 48, 32, 2, False, children, "image", y0=7, y1=7, slots=8)
        assert empty.n == 0 and empty.n_children == 0 and empty.counted == (0, 0, 0, 0, 0) and empty.untouched(0)
        for t in (empty.rgb, empty.hits, empty.sample_rgb, empty.color, empty.normal):
            assert bool((t == SENTINEL).all())


@pytest.mark.gpu
def test_grid_stride_loop_and_a_partial_last_workgroup(miro):
    """64 spp on the textured teapot with two lights before the image: 385 x 351 x 64 = 8 648 640 samples are 33 783 workgroups of
    256 and three quarters of one more -- above the grid cap of 32 768, so the first workgroups take a second chunk, and the last
    chunk's fourth wave lies past the end of the window.  out_capacity = 1000.  Pixels, counters and d_out_count against
    mr_render_lights_environment and mr_trace_level_lights, compared on the device."""
    import torch
    from miro_amd import binding
    W, H, spp = 385, 351, 64
    n = W * H * spp
    assert n % 256 == 192 and n // 256 + 1 > 32768
    scene, desc, lights = use(miro, "teapot_textured", "image")
    scene.set_lights(lights[:2])
    f32 = dict(dtype=torch.float32, device="cuda")
    want_rgb, want_counts = torch.empty((W * H, 3), **f32), torch.zeros(5, dtype=torch.int64, device="cuda")
    scene.render_lights_environment(camera(desc), W, H, want_rgb, spp=spp, jitter=True, seed=168, d_counts=want_counts)
    rays = torch.empty((n, 8), **f32)
    scene.gen_eye_rays(camera(desc), W, H, rays, spp=spp, jitter=True, seed=168)
    out = (torch.empty((1000, 8), **f32), torch.empty((1000, 3), **f32), torch.empty(1000, dtype=torch.int32, device="cuda"))
    want_count, got_count = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 7, dtype=torch.int64, device="cuda")
    scene.trace_level_lights(rays, None, None, n, torch.zeros((W * H, 3), **f32), children=binding.MR_LEVEL_SPECULAR, environment=True,
                             d_out_rays=out[0], d_out_weights=out[1], d_out_pixels=out[2], d_out_count=want_count, spp=spp)
    del rays
    got_rgb, got_counts = torch.full((W * H + 1, 3), SENTINEL, **f32), torch.zeros(5, dtype=torch.int64, device="cuda")
    out[2].fill_(PIX)
    scene.render_level_lights(camera(desc), W, H, got_rgb, spp=spp, jitter=True, seed=168, d_counts=got_counts,
                              children=binding.MR_LEVEL_SPECULAR, environment=True, d_out_rays=out[0], d_out_weights=out[1],
                              d_out_pixels=out[2], d_out_count=got_count, out_capacity=1000)
    torch.cuda.synchronize()
    scene.set_lights(lights)
    c = want_counts.tolist()
    assert c[0] == n and 0 < c[3] < n and c[1] == (n - c[3]) * 2 and int(want_count.item()) > 1000 and float(want_rgb.max()) > 0
    assert torch.equal(got_rgb[:W * H], want_rgb) and bool((got_rgb[W * H] == SENTINEL).all())
    assert got_counts.tolist() == c and int(got_count.item()) == int(want_count.item())
    pix = out[2]
    assert int(pix.min().item()) >= 0 and int(pix.max().item()) < W * H               # 1000 stored children, pixels of this frame
    del want_rgb, got_rgb, out
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_level_last_is_mr_render_lights_environment(miro):
    """MR_LEVEL_LAST forwards to the existing frame: every output equal, the queue arguments ignored (d_out_count untouched)"""
    scene, desc, lights = use(miro, "teapot_textured", "image")
    for spp, tiled in ((1, False), (4, True)):
        want = EnvFrame(miro, scene, desc, 48, 32, spp, tiled)
        fu = Level0(miro, scene, desc, 48, 32, spp, tiled, 0, "image")
        assert_frame_half(fu, want)
        assert int(fu.count.item()) == 12345 and fu.untouched(0)


@pytest.mark.gpu
@pytest.mark.parametrize("children", [SPECULAR, PATH])
def test_replays_from_a_captured_graph(miro, children):
    """After one warm call outside the capture (it uploads the texture table and the image) the 48 x 32 x 2 frame of the mixed room
    under the image is captured into a torch.cuda.graph on one stream and replayed twice, every output filled with sentinels and
    d_out_count with a wrong value before each replay: the frame half and the child set equal the direct launch's, d_out_count is
    zeroed by each replay, and the counters advance by one step per replay."""
    import torch
    scene, desc, lights = use(miro, "mixed", "image")
    W, H, spp = 48, 32, 2
    want = EnvFrame(miro, scene, desc, W, H, spp, False)
    fu = Level0(miro, scene, desc, W, H, spp, False, children, "image")              # the warm call, a direct launch
    assert_frame_half(fu, want, open_scene=False)
    rows0 = fu.spec_rows() if children == SPECULAR else fu.path_rows()
    assert fu.n_children > 0 and len(rows0) == fu.n_children
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fu.launch(torch.cuda.current_stream())
    for _ in range(2):
        for t in (fu.rgb, fu.hits, fu.sample_rgb, fu.color, fu.normal, fu.out[0], fu.out[1]):
            t.fill_(SENTINEL)
        fu.out[2].fill_(PIX)
        fu.out[3].fill_(ID)
        fu.out[4].fill_(BYTE)
        fu.out_low.fill_(BYTE)
        fu.count.fill_(999999)
        fu.counts.copy_(torch.tensor(COUNTS0 + (4242,), dtype=torch.int64))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fu.read()
        assert_frame_half(fu, want, open_scene=False)
        assert np.array_equal(fu.spec_rows() if children == SPECULAR else fu.path_rows(), rows0) and fu.untouched(fu.n_children)


def frames(miro, name, env, w, h, spp, depth, route, tiled=False, **kw):
    """render_specular(fused="frame_" + route), on a renderer without resident rays, and fused=route: (per_level, pixels) of each"""
    import torch
    from miro_amd import frame
    scene, desc, lights = use(miro, name, env)
    out = []
    for fused, resident in (("frame_" + route, False), (route, True)):
        fr = frame.FrameRenderer(scene, desc, w, h, spp=spp, tiled=tiled, resident_rays=resident)
        if resident:
            fr.generate()
        per_level = fr.render_specular(depth=depth, lights=lights, environment=ENVS[env], fused=fused, **kw)
        torch.cuda.synchronize()
        out.append((per_level, fr.d_rgb.clone()))
        if not resident:
            assert fr.bytes_resident() == 8 + w * h * 12 * (2 if fr.tiled else 1) + (w * h * 8 if fr.tiled else 0)
    return out


WHOLE = [("stone", None, 2), ("flower_drops", "colour", 3), ("teapot_textured", "image", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["lights", "lights_path"])
@pytest.mark.parametrize("name,env,depth", WHOLE)
def test_whole_frames(miro, name, env, depth, route):
    """render_specular(fused="frame_lights") against "lights" and "frame_lights_path" against "lights_path" (kinds 7, the same seed)
    at 48 x 32 x 2 in image order, and once more in tiled order: the same rays and shadow rays per level, pixels within 2e-5 of the
    largest value -- the whole-frame bound of tests/test_level_lights.py for the order of the float atomics; level 0 differs only by
    a pairwise mean against an atomic sum of 2 terms and needs no more.  At 1 spp and depth 0 the level-0 pixels are equal exactly.
    Measured on the MI355X, the largest |difference| / largest value of each case, over both orders (bound 2e-5): stone 3.0e-10
    ("lights") and 6.0e-8 ("lights_path"), flower with drops under a colour 6.5e-9 and 0, teapot under the image 1.5e-8 and 1.1e-7."""
    kw = dict(path_tracing=True, path_kinds=7, path_seed=29) if route == "lights_path" else {}
    worst = 0.0
    for tiled in (False, True):
        (levels_f, rgb_f), (levels_b, rgb_b) = frames(miro, name, env, 48, 32, 2, depth, route, tiled=tiled, **kw)
        print("per_level", levels_b, "max", float(rgb_b.max()))
        assert len(levels_b) >= 2 and all(n > 0 and s > 0 for n, s in levels_b) and levels_b[0][0] == 48 * 32 * 2
        assert levels_f == levels_b
        top = float(rgb_b.abs().max())
        worst = max(worst, float((rgb_f - rgb_b).abs().max()) / top)
        assert top > 0 and float((rgb_f - rgb_b).abs().max()) <= 2e-5 * top, float((rgb_f - rgb_b).abs().max()) / top
    print("whole frame %s %s %s: max |difference| / largest value %.3g" % (name, env, route, worst))
    (l0_f, rgb0_f), (l0_b, rgb0_b) = frames(miro, name, env, 48, 32, 1, 0, route, **kw)
    assert l0_f == l0_b and len(l0_b) == 1 and float(rgb0_b.max()) > 0 and same(rgb0_f, rgb0_b)


@pytest.mark.gpu
def test_photon_maps_on_the_frame_route(miro):
    """The stone room (bumped normals: the frame hands mr_gather_level its d_sample_normal) with a global and a caustic map from the
    product's own surface walk, depth 1, at 48 x 32 x 2 and on rows [9, 21) at 1 spp: fused="frame_lights" with photon_maps against
    fused="lights" with the same maps -- level 0's gather reads generate()'s rays and adds to the pixel ray index // spp of d_rgb,
    which must be the frame's own pixel, also in a window that does not start at row 0.  The same counts per level, pixels within
    the whole-frame bound; on the level route alone the maps change the picture, so the term is not empty."""
    import torch
    from miro_amd import frame
    from test_photon_walk import K_GATHER, MAX_DIST, product_trace
    scene, desc, lights = use(miro, "stone", None)
    maps = []
    for caustic, target in ((False, 6000), (True, 2500)):
        m, res, _ = product_trace(miro, scene, desc, target, 400000, caustic, target + 64, target + 64, surface=True)
        assert res["stored"] >= target
        m.balance()
        maps.append(m)
    for spp, bands in ((2, None), (1, [(9, 21)])):
        got = {}
        for fused, kw in (("lights", dict(photon_maps=None)), ("lights", {}), ("frame_lights", {})):
            fr = frame.FrameRenderer(scene, desc, 48, 32, spp=spp, tiled=False, bands=bands)
            fr.generate()
            args = dict(depth=1, lights=lights, fused=fused, photon_maps=tuple(maps), nphotons=K_GATHER, max_dist=MAX_DIST)
            args.update(kw)
            per_level = fr.render_specular(**args)
            torch.cuda.synchronize()
            got[(fused, "photon_maps" in kw)] = (per_level, fr.d_rgb.clone())
        (plain_levels, plain), (want_levels, want), (levels, rgb) = got[("lights", True)], got[("lights", False)], got[("frame_lights", False)]
        top = float(want.abs().max())
        term = float((want - plain).abs().max())
        print("spp %d bands %s: per_level %s, the photon term reaches %.3g of %.3g" % (spp, bands, want_levels, term, top))
        assert want_levels == plain_levels and len(want_levels) == 2 and term > 1e-3 * top
        assert levels == want_levels
        assert float((rgb - want).abs().max()) <= 2e-5 * top, float((rgb - want).abs().max()) / top
