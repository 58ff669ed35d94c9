"""mr_trace_level_lights_path -- one level of Scene::traceScene's recursion of a PATH_TRACING build in one launch on ANY scene
(csrc/mr_level_lights_path.hip): mr_trace_level_lights' per-ray steps, then the children of mr_gen_path_rays_surface -- lobe-sampled
mirror / Fresnel / refract children and Ray::random's diffuse bounce about the bumped normal, the diffuse child with the looked-up
colour -- with the path tracer's ray ids and the byte that marks a ray made by Ray::random (a miss of such a ray reads the low-res
environment image, Scene.cpp:678-681).

The yardstick everywhere is the batched chain on the same queue, seed, bounce and kinds,

    trace -> hit_surface -> shade_lights_surface(d_ray_rgb) || shade_environment(the same flags and d_lowres, d_ray_rgb)
    -> gen_path_rays_surface(that chain's colour and normal)

which tests/test_procedural.py, tests/test_lights.py, tests/test_environment.py and tests/test_path_surface.py hold against the
oracle and the restatements.  Per-ray outputs and counters are compared EXACTLY, the children as sets of (id, ray, weight, pixel,
octant) records sorted by child id, d_out_count exactly, the pixel sums within the bound of tests/test_level_lights.py (float
atomics: rtol 1e-5, atol 1e-6 x max; whole frames 2e-5 x max).  Every comparison first asserts on the batched side alone that
the case is not empty.

Not reachable at test size and not tested: the kernel's grid-stride loop, which starts at 8.4 M rays."""
import collections
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
from test_frame_lights import scene_of as plain_scene_of  # noqa: E402
from test_frame_lights_environment import BG, ROTATION, image  # noqa: E402
from test_level_lights import use  # noqa: E402
from test_path_surface import PLANE_BIT, child_id  # noqa: E402

F = np.float32
NAME = "mr_trace_level_lights_path"
COUNTS0 = (1000, 5, 77, 31, 9)                          # what d_counts holds before a call: the call does not zero it
ENVS = {None: None, "colour": dict(bg_color=BG), "image": dict(pixels=image(168), rotation=ROTATION)}
PIX, ID, BYTE = 0x7A7A7A7A, 0x5B5B5B5B, 0xEE            # the sentinels of an int32 pixel / id column and of a byte column
ALL_KINDS = 7
KIND_OF_BIT = {1: 0, 2: 2, 4: 3}                        # MR_PATH_MIRROR / _REFRACT / _DIFFUSE -> the child kind that only it emits

# rays, optional weights / pixels / ids / low-res bytes (None: 1, ray index // spp, ray index, not isDiffuse), the number of rays
Q = collections.namedtuple("Q", "rays weights pixels ids low n")


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_trace_level_lights_path_is_exported_declared_and_bound(miro):
    from miro_amd import binding

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return re.search(r"\bmr_status\s+%s\s*\(" % NAME, src) is not None

    assert hasattr(miro.lib(), NAME)
    assert declared("miro_hip_frame.h") and not declared("miro_hip.h") and not declared("miro_hip_surface.h")
    assert NAME in binding.FRAME_SYMBOLS and NAME not in binding.SURFACE_SYMBOLS and NAME not in miro.EXPORTED_SYMBOLS
    assert len(binding.FRAME_SYMBOLS) == len(set(binding.FRAME_SYMBOLS)) == 3
    assert len(miro.EXPORTED_SYMBOLS) == 69 and len(binding.SURFACE_SYMBOLS) == 9
    assert getattr(miro.lib(), NAME).restype is C.c_int32
    assert hasattr(miro.Scene, "trace_level_lights_path") and C.sizeof(binding.LevelLightsPathDesc) == 80
    assert binding.LevelLightsPathDesc.d_out_octants.offset == 56 and binding.LevelLightsPathDesc.d_out_lowres.offset == 72


def test_level_lights_path_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_level_lights_path.hip: no dynamic stack; at least four waves per SIMD; no more spilled VGPRs, no more
    scratch per lane and no fewer waves than BOTH its own record (tests/golden/kernel_budget_level_lights_path.json, written from
    the build whose GPU run of this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.
    Twelve level kernels, one per traversal variant of with_trace_variant (six) and children (none, path tracing): the
    environment, the texture table and the masks are wave-uniform branches.  The unit has no other kernel: the one-word store
    that zeroes d_out_count is mr_level_lights.hip's, held to that unit's record."""
    cur = kernel_budget.unit_kernels("mr_level_lights_path")
    level = [k for k in cur if "level_lights_path_kernel" in k]
    assert len(level) == 6 * 2 and sorted(set(cur) - set(level)) == []
    assert not any("frame_kernel" in k or "trace_kernel" in k for k in cur)
    for var in (1818, 826, 267, 43, 88, 73):                   # kTraceExact, ExactObj, Product, ProductObj, Vote, VoteProduct
        for children in (0, 1):
            assert sum("ILi%dELi%dEE" % (var, children) in k for k in cur) == 1, (var, children)
    assert not any(v["dynamic_stack"] for v in cur.values())
    assert all(v["waves_per_simd"] >= 4 for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_level_lights_path.json", also_main=True)


def level_desc(binding, spp=1, flags=0, children=0, environment=0, capacity=0, reserved=None, kinds=ALL_KINDS, lowres=None, out_lowres=None,
               octants=None):
    ld = binding.LevelLightsPathDesc()
    ld.spp, ld.flags, ld.children, ld.environment = spp, flags, children, environment
    ld.path_kinds, ld.seed, ld.bounce = kinds, 168, 0
    ld.out_capacity_lo, ld.out_capacity_hi = capacity & 0xFFFFFFFF, capacity >> 32
    ld.d_lowres, ld.d_out_lowres, ld.d_out_octants = lowres, out_lowres, octants
    if reserved is not None:
        ld.reserved[reserved] = 1
    return ld


def test_argument_errors_come_before_the_scene_and_the_device(miro):
    """Every MR_ERR_INVALID case on a host_only one-triangle scene: answered from the arguments alone, under this call's name,
    before any device call, so "no HIP device" and "host_only" may not be what comes back.  The two byte masks and the octant
    bytes take any address: at odd addresses the call gets as far as the scene's state.  Then MR_ERR_STATE for that scene, for an
    unbuilt one and for one without lights."""
    from miro_amd import binding
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.build(4, host_only=True)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    base = dict(scene=s.h, rays=p(4096), weights=None, pixels=None, ids=None, n=64, rgb=p(8192), hits=None, ray_rgb=None, color=None,
                normal=None, out_rays=None, out_weights=None, out_pixels=None, out_ids=None, out_count=None, counts=None)
    queue = dict(out_rays=p(1 << 16), out_weights=p(1 << 17), out_pixels=p(1 << 18), out_count=p(1 << 19))

    def call(ld, **kw):
        a = dict(base, **kw)
        st = getattr(L, NAME)(a["scene"], C.byref(ld) if ld is not None else None, a["rays"], a["weights"], a["pixels"], a["ids"], a["n"],
                              a["rgb"], a["hits"], a["ray_rgb"], a["color"], a["normal"], a["out_rays"], a["out_weights"],
                              a["out_pixels"], a["out_ids"], a["out_count"], a["counts"], None)
        return st, L.mr_last_error()

    ok = level_desc(binding)
    path = level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=256)
    invalid = [
        ("NULL", call(ok, scene=None)), ("NULL", call(None)), ("NULL", call(ok, rays=None)),
        ("d_ray_rgb", call(ok, rgb=None)),
        ("spp", call(level_desc(binding, spp=0))),
        ("flags", call(level_desc(binding, flags=binding.MR_TRACE_ANY))), ("flags", call(level_desc(binding, flags=binding.MR_MATH_FAST))),
        ("flags", call(level_desc(binding, flags=1 << 30))),
        ("mr_trace_level_lights'", call(level_desc(binding, children=binding.MR_LEVEL_SPECULAR, capacity=256), **queue)),
        ("children", call(level_desc(binding, children=7, capacity=256), **queue)),
        ("environment", call(level_desc(binding, environment=2))),
        ("path_kinds", call(level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=256, kinds=0), **queue)),
        ("path_kinds", call(level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=256, kinds=8), **queue)),
        ("reserved", call(level_desc(binding, reserved=0))), ("reserved", call(level_desc(binding, reserved=4))),
        ("output queue", call(path)), ("output queue", call(path, **dict(queue, out_count=None))),
        ("output queue", call(path, **dict(queue, out_weights=None))),
        ("out_capacity", call(level_desc(binding, children=binding.MR_LEVEL_PATH), **queue)),
        ("aligned", call(ok, rays=p(4096 + 8))), ("aligned", call(path, **dict(queue, out_rays=p((1 << 16) + 4)))),
        ("aligned", call(ok, hits=p(2048 + 8))), ("aligned", call(ok, counts=p(4100))),
        ("aligned", call(path, **dict(queue, out_count=p((1 << 19) + 4)))),
        ("aligned", call(ok, rgb=p(8194))), ("aligned", call(ok, ray_rgb=p(4098))), ("aligned", call(ok, color=p(4098))),
        ("aligned", call(ok, normal=p(4097))), ("aligned", call(ok, weights=p(4098))), ("aligned", call(ok, pixels=p(4097))),
        ("aligned", call(ok, ids=p(4098))), ("aligned", call(path, **dict(queue, out_ids=p((1 << 20) + 1)))),
        ("aligned", call(path, **dict(queue, out_pixels=p((1 << 18) + 2)))), ("aligned", call(path, **dict(queue, out_weights=p((1 << 17) + 3)))),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and NAME.encode() in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    st, msg = call(ok)                                                            # then the scene's state: never a CPU path
    assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg
    st, msg = call(ok, rgb=None, ray_rgb=p(4096))                                 # d_rgb may be NULL when d_ray_rgb is given
    assert st == binding.MR_ERR_STATE, msg
    odd = level_desc(binding, children=binding.MR_LEVEL_PATH, capacity=256, lowres=4097, out_lowres=(1 << 21) + 3, octants=(1 << 22) + 1,
                     flags=binding.MR_ENV_LOWRES | binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT)
    st, msg = call(odd, **dict(queue, out_ids=p(1 << 20), ids=p(1 << 23)))        # bytes lie anywhere; all three flags are legal
    assert st == binding.MR_ERR_STATE and b"aligned" not in msg, msg
    st, msg = call(level_desc(binding, kinds=0))                                  # path_kinds is read with children only
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


# ---- on the MI355X: helpers ------------------------------------------------------------------------------------------------
def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def eye_queue(scene, desc, w, h, spp=1):
    import torch
    rays = torch.empty((w * h * spp, 8), dtype=torch.float32, device="cuda")
    scene.gen_eye_rays(camera(desc), w, h, rays, spp=spp, jitter=spp > 1, seed=168)
    return Q(rays, None, None, None, None, w * h * spp)


def explicit(q, seed, n=None, n_pixels=1000):
    """`n` rays of q drawn without order (a seeded permutation), with explicit seeded weights, pixels and ids"""
    rng = np.random.RandomState(seed)
    n = q.n if n is None else n
    pick = cuda(rng.permutation(q.n)[:n].astype(np.int64))
    return Q(q.rays[pick].contiguous(), cuda(rng.rand(n, 3).astype(F)), cuda(rng.randint(0, n_pixels, n).astype(np.int32)),
             cuda(rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)),
             None if q.low is None else q.low[pick].contiguous(), n)


def parent_ids(q):
    return np.arange(q.n, dtype=np.uint32) if q.ids is None else q.ids.cpu().numpy().view(np.uint32)


def rows_of(out, m):
    """slots [0, m) of (rays, weights, pixels, ids, octants) as rows of uint32, id first, in lexicographic order"""
    rays, w, pix, ids, octs = (o[:m].cpu().numpy() for o in out)
    t = np.concatenate([ids.view(np.uint32)[:, None], rays.view(np.uint32).reshape(m, 8), w.view(np.uint32).reshape(m, 3),
                        pix.view(np.uint32)[:, None], octs.astype(np.uint32)[:, None]], axis=1)
    return t[np.lexsort(t.T[::-1])]


def env_flags(binding, all_lowres):
    return binding.MR_ENV_LOWRES if all_lowres else 0


class Chain:
    """The batched chain of one level: hit records, the surface pass's colour and normal (rows of rays that missed keep the
    sentinel), the expected per-ray L (the light chain's row of a hit, the environment chain's row of a miss, 0 without an
    environment), the pixel sums, the counters, and the children of gen_path_rays_surface fed that colour and normal"""

    def __init__(self, scene, n_lights, q, spp, flags, env, n_pixels, kinds=ALL_KINDS, children=True, seed=168, bounce=0,
                 all_lowres=False):
        import torch
        from miro_amd import binding
        f32 = dict(dtype=torch.float32, device="cuda")
        i64 = dict(dtype=torch.int64, device="cuda")
        n = self.n = q.n
        self.q = q
        self.hits = torch.empty((n, 4), **f32)
        self.color, self.normal, lights_rgb, env_rgb = (torch.full((n, 3), SENTINEL, **f32) for _ in range(4))
        self.rgb = torch.zeros((n_pixels, 3), **f32)
        undefined, shadow, envc, count = torch.zeros(1, **i64), torch.zeros(1, **i64), torch.zeros(2, **i64), torch.zeros(1, **i64)
        scene.trace_device(q.rays, n, self.hits, flags)
        scene.hit_surface(q.rays, self.hits, n, self.color, self.normal, d_counts=undefined)
        scene.shade_lights_surface(q.rays, self.hits, self.color, self.normal, n, self.rgb, d_weights=q.weights, d_pixels=q.pixels, spp=spp,
                                   flags=flags, d_ray_rgb=lights_rgb, d_counts=shadow)
        if env:
            scene.shade_environment(q.rays, self.hits, n, self.rgb, d_weights=q.weights, d_pixels=q.pixels, d_lowres=q.low, spp=spp,
                                    flags=env_flags(binding, all_lowres), d_ray_rgb=env_rgb, d_counts=envc)
        self.out = None
        if children:
            self.out = (torch.empty((4 * n, 8), **f32), torch.empty((4 * n, 3), **f32), torch.empty(4 * n, dtype=torch.int32, device="cuda"),
                        torch.empty(4 * n, dtype=torch.int32, device="cuda"), torch.empty(4 * n, dtype=torch.uint8, device="cuda"))
            scene.gen_path_rays_surface(q.rays, self.hits, self.color, self.normal, q.weights, q.pixels, q.ids, n, self.out[0], self.out[1],
                                        self.out[2], self.out[3], count, spp=spp, seed=seed, bounce=bounce, kinds=kinds,
                                        d_out_octants=self.out[4])
        torch.cuda.synchronize()
        self.hit_rows = self.hits[:, 1].contiguous().view(torch.int32) != -1
        self.n_hits = int(self.hit_rows.sum().item())
        self.ray_rgb = torch.where(self.hit_rows[:, None], lights_rgb, env_rgb if env else torch.zeros_like(env_rgb))
        assert int(shadow.item()) == self.n_hits * n_lights
        if env:
            assert int(envc[0].item()) == n - self.n_hits
        self.counted = (n, int(shadow.item()), int(undefined.item()), n - self.n_hits, int(envc[1].item()))
        self.n_children = int(count.item())
        self.rows = rows_of(self.out, self.n_children) if children else None
        self.kinds = kinds

    def per_kind(self):
        """children of each kind 0..3, counted from their ids (a child's id is child_id(parent id, kind))"""
        got = self.rows[:, 0]
        hit = self.hit_rows.cpu().numpy()
        return [int(np.isin(child_id(parent_ids(self.q)[hit], k), got).sum()) for k in range(4)]

    def assert_not_empty(self, env=False, has=ALL_KINDS):
        """children of every requested kind that a material of the scene has (`has`); hits and misses where an environment is set"""
        per = self.per_kind()
        for bit, kind in KIND_OF_BIT.items():
            assert (per[kind] > 0) == bool(self.kinds & has & bit), (self.kinds, per)
        assert (per[1] > 0) == bool(self.kinds & has & 2), (self.kinds, per)                             # Fresnel children come with refraction
        assert sum(per) == self.n_children and len(np.unique(self.rows[:, 0])) == self.n_children        # ids are unique per child
        assert self.n_hits > 0 and (not env or self.n_hits < self.n)
        return per


class Fused:
    """One mr_trace_level_lights_path call with every optional output, each per-ray buffer n + 1 rows long (a sentinel row past
    the end) and the output queue `slots` long, all filled with sentinels first"""

    def __init__(self, scene, q, spp, flags, env, n_pixels, kinds=ALL_KINDS, children=True, seed=168, bounce=0, all_lowres=False,
                 slots=None, capacity=None, rgb=True, stream=None):
        import torch
        from miro_amd import binding
        f32 = dict(dtype=torch.float32, device="cuda")
        n = self.n = q.n
        slots = 4 * n if slots is None else slots
        self.rgb = torch.zeros((n_pixels, 3), **f32) if rgb else None
        self.hits = torch.full((n + 1, 4), SENTINEL, **f32)
        self.ray_rgb, self.color, self.normal = (torch.full((n + 1, 3), SENTINEL, **f32) for _ in range(3))
        self.counts = torch.tensor(COUNTS0, dtype=torch.int64, device="cuda")
        self.count = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
        self.out = self.out_low = None
        if children:
            self.out = (torch.full((slots, 8), SENTINEL, **f32), torch.full((slots, 3), SENTINEL, **f32),
                        torch.full((slots,), PIX, dtype=torch.int32, device="cuda"), torch.full((slots,), ID, dtype=torch.int32, device="cuda"),
                        torch.full((slots,), BYTE, dtype=torch.uint8, device="cuda"))
            self.out_low = torch.full((slots,), BYTE, dtype=torch.uint8, device="cuda")
        o = self.out or (None,) * 5
        self.launch = lambda st=stream: scene.trace_level_lights_path(
            q.rays, q.weights, q.pixels, q.ids, n, self.rgb, children=binding.MR_LEVEL_PATH if children else binding.MR_LEVEL_LAST,
            environment=bool(env), d_hits=self.hits, d_ray_rgb=self.ray_rgb, d_color=self.color, d_normal=self.normal, d_out_rays=o[0],
            d_out_weights=o[1], d_out_pixels=o[2], d_out_ids=o[3], d_out_count=self.count if children else None, d_counts=self.counts,
            spp=spp, flags=flags | env_flags(binding, all_lowres), seed=seed, bounce=bounce, kinds=kinds, stream=st, out_capacity=capacity,
            d_out_octants=o[4], d_lowres=q.low, d_out_lowres=self.out_low)
        self.launch()
        torch.cuda.synchronize()
        for t in (self.hits, self.ray_rgb, self.color, self.normal):
            assert bool((t[n:] == SENTINEL).all()), "written beyond the end"
        self.counted = tuple(int(c) - c0 for c, c0 in zip(self.counts.cpu().numpy(), COUNTS0))
        self.n_children = int(self.count.item()) if children else 0

    def rows(self, m=None):
        return rows_of(self.out, self.n_children if m is None else m)

    def untouched(self, m):
        """slots [m, end) of every output column still hold the sentinels"""
        return (bool((self.out[0][m:] == SENTINEL).all()) and bool((self.out[1][m:] == SENTINEL).all()) and bool((self.out[2][m:] == PIX).all())
                and bool((self.out[3][m:] == ID).all()) and bool((self.out[4][m:] == BYTE).all()) and bool((self.out_low[m:] == BYTE).all()))

    def lowres_is_the_diffuse_children(self, q):
        """d_out_lowres is 1 exactly on the stored children whose id is child_id(parent, 3), 0 on the others"""
        m = self.n_children
        ids = self.out[3][:m].cpu().numpy().view(np.uint32)
        low = self.out_low[:m].cpu().numpy()
        return set(np.unique(low)) <= {0, 1} and np.array_equal(low == 1, np.isin(ids, child_id(parent_ids(q), 3)))

    def next_queue(self):
        m = self.n_children
        return Q(self.out[0][:m].contiguous(), self.out[1][:m].contiguous(), self.out[2][:m].contiguous(), self.out[3][:m].contiguous(),
                 self.out_low[:m].contiguous(), m)


def assert_level_is_the_chain(fu, ch, exact_rgb=False):
    """hit records on their bits; colour and normal, the rows of misses untouched; per-ray L; all five counters; d_out_count and
    the children as sets sorted by child id; nothing written past the count; the pixel sums within the float-atomic bound of
    tests/test_level_lights.py -- nothing left out"""
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
        assert np.array_equal(fu.rows(), ch.rows)
        assert fu.untouched(fu.n_children) and fu.lowres_is_the_diffuse_children(ch.q)
    if fu.rgb is not None:
        scale = float(ch.rgb.abs().max())
        if exact_rgb:
            assert same(fu.rgb, ch.rgb)
        assert torch.allclose(fu.rgb, ch.rgb, rtol=1e-5, atol=1e-6 * scale), float((fu.rgb - ch.rgb).abs().max())


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [1, 2, 3, 4, 5, 6, 7])
def test_every_kind_in_the_mixed_room(miro, kinds):
    """The closed room with glass and mirror spheres, a glossy checker plane and five texture kinds under a disc and a point light.
    Two queues: the 2 048 eye rays of a 64 x 32 frame with weights, pixels and ids NULL at bounce 0, and 515 of them in seeded
    order with explicit weights, pixels and ids at bounce 2 under another seed -- two workgroups and 3 lanes of a third."""
    scene, desc, lights = use(miro, "mixed", None)
    eye = eye_queue(scene, desc, 64, 32)
    for q, n_pixels, kw in ((eye, 64 * 32, dict()), (explicit(eye, 11, 515), 1000, dict(seed=9, bounce=2))):
        ch = Chain(scene, len(lights), q, 1, 0, None, n_pixels, kinds=kinds, **kw)
        per = ch.assert_not_empty()
        fu = Fused(scene, q, 1, 0, None, n_pixels, kinds=kinds, **kw)
        print("mixed room kinds %d, %d rays: %d hits, children per kind %s, counters %s" % (kinds, q.n, ch.n_hits, per, ch.counted))
        assert_level_is_the_chain(fu, ch)


def glass_sphere(miro):
    """the glass sphere of tests/test_path_surface.py (kd = 0, ks, kt = 0.9, index 1.5) under one point light"""
    s = miro.Scene(0)
    s.add_triangle([40, 0, 40, 41, 0, 40, 40, 1, 40], [0, 0, 1] * 3)                          # far away: a scene needs one bounded object
    s.add_sphere((0.0, 0.0, 0.0), 1.0)
    s.set_materials([((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 1.0, 1.0), ((0.0, 0.0, 0.0), (0.05, 0.05, 0.05), (0.9, 0.9, 0.9), 80.0, 1.5)], [0, 1])
    s.build(4)
    s.set_lights([dict(position=(3.0, 4.0, 5.0), wattage=50.0)])
    return s


@pytest.mark.gpu
def test_slot_accounting_on_a_glass_sphere(miro):
    """1 100 parallel rays onto the sphere from normal to grazing incidence, so that Rs falls on both sides of 0.01 and a parent
    has 2 or 3 children, and 700 rays from seeded points INSIDE it in seeded directions, a share of which meet the surface beyond
    the critical angle (sin > 1 / 1.5): their refract child is the total internal reflection.  The whole set equals the chain's;
    then out_capacity = count - 5 into buffers three slots longer than count: d_out_count still holds count, the stored slots are
    members of the full set, each once, and every column from the capacity on -- ids, octants and the low-res byte included --
    keeps its sentinel."""
    s = glass_sphere(miro)
    rng = np.random.RandomState(47)
    n_out, n_in = 1100, 700
    r, az = np.sqrt(rng.rand(n_out)) * 1.05, rng.uniform(0, 2 * np.pi, n_out)
    o = np.stack([r * np.cos(az), r * np.sin(az), np.full(n_out, 5.0)], 1)
    d = np.tile(np.array([0.0, 0.0, -1.0]), (n_out, 1))
    oi = rng.randn(n_in, 3)
    oi *= (rng.uniform(0.3, 0.95, n_in) / np.linalg.norm(oi, axis=1))[:, None]
    di = rng.randn(n_in, 3)
    di /= np.linalg.norm(di, axis=1)[:, None]
    rays = np.zeros((n_out + n_in, 8), F)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = np.concatenate([o, oi]), np.concatenate([d, di]), 1e12
    q = Q(cuda(rays), None, None, None, None, n_out + n_in)
    ch = Chain(s, 1, q, 1, 0, None, q.n)
    per = ch.per_kind()
    hits = ch.hits.cpu().numpy()
    inside = np.arange(q.n) >= n_out
    P = rays[:, 0:3].astype(np.float64) + hits[:, 0:1].astype(np.float64) * rays[:, 4:7]
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - (rays[:, 4:7] * P).sum(1) ** 2))               # the sphere's normal at P is P
    tir = inside & ch.hit_rows.cpu().numpy() & (1.5 * sin_t > 1.05)
    print("glass sphere: %d hits of %d rays, children per kind %s, %d total internal reflections" % (ch.n_hits, q.n, per, tir.sum()))
    assert per[0] == ch.n_hits and per[2] == ch.n_hits and per[3] == 0                    # ks and kt everywhere, kd = 0
    assert 50 < per[1] < ch.n_hits - 50                                                   # Rs on both sides of 0.01
    assert len(np.unique(ch.rows[:, 0])) == ch.n_children == sum(per)
    assert tir.sum() > 20 and 0 < ch.n - ch.n_hits
    fu = Fused(s, q, 1, 0, None, q.n)
    assert_level_is_the_chain(fu, ch)
    count = ch.n_children
    part = Fused(s, q, 1, 0, None, q.n, slots=count + 3, capacity=count - 5)
    assert part.n_children == count and part.untouched(count - 5)
    want = {row.tobytes() for row in ch.rows}
    got = part.rows(count - 5)
    assert len(np.unique(got[:, 0])) == count - 5 and all(row.tobytes() in want for row in got)
    assert set(np.unique(part.out_low[:count - 5].cpu().numpy())) == {0}
    assert same(part.ray_rgb[:q.n], ch.ray_rgb) and part.counted == ch.counted


@pytest.mark.gpu
def test_stone_floor_children_leave_about_the_bumped_normal(miro):
    """The stone room, 48 x 32 eye rays with explicit weights: the level is the chain's; every diffuse child of a floor hit carries
    w0 x the looked-up stone colour bit for bit; and, against the same generator fed the GEOMETRIC normal of mr_hit_attrs
    (normalised), at least half of the floor's diffuse children leave in another direction."""
    import torch
    scene, desc, lights = use(miro, "stone", None)
    eye = eye_queue(scene, desc, 48, 32)
    rng = np.random.RandomState(3)
    q = eye._replace(weights=cuda(rng.uniform(0.2, 1.0, (eye.n, 3)).astype(F)))
    ch = Chain(scene, len(lights), q, 1, 0, None, q.n)
    ch.assert_not_empty()
    fu = Fused(scene, q, 1, 0, None, q.n)
    assert_level_is_the_chain(fu, ch)
    prim = bits(ch.hits)[:, 1]
    floor = np.nonzero((prim != MISS) & ((prim & np.uint32(PLANE_BIT)) != 0))[0]
    assert len(floor) > q.n // 8
    P, N = torch.empty((q.n, 3), dtype=torch.float32, device="cuda"), torch.empty((q.n, 3), dtype=torch.float32, device="cuda")
    scene.hit_attrs(ch.hits, q.n, P, N, d_rays=q.rays)
    flat = N / N.norm(dim=1, keepdim=True)
    geo = (torch.empty((4 * q.n, 8), dtype=torch.float32, device="cuda"), torch.empty((4 * q.n, 3), dtype=torch.float32, device="cuda"),
           torch.empty(4 * q.n, dtype=torch.int32, device="cuda"), torch.empty(4 * q.n, dtype=torch.int32, device="cuda"),
           torch.empty(4 * q.n, dtype=torch.uint8, device="cuda"))
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    scene.gen_path_rays_surface(q.rays, ch.hits, ch.color, flat.contiguous(), q.weights, None, None, q.n, *geo[:4], cnt, d_out_octants=geo[4])
    torch.cuda.synchronize()
    geo_rows = rows_of(geo, int(cnt.item()))
    got = fu.rows()
    want_id = child_id(floor, 3)                                # ids NULL: a ray's id is its index

    def at(rows):
        slot = np.minimum(np.searchsorted(rows[:, 0], want_id), len(rows) - 1)
        assert np.array_equal(rows[slot, 0], want_id)
        return rows[slot]

    mine, theirs = at(got), at(geo_rows)
    differ = (mine[:, 5:8] != theirs[:, 5:8]).any(axis=1).mean()
    print("stone room: %d floor hits; share of their diffuse children that the geometric normal sends elsewhere %.3f" % (len(floor), differ))
    assert differ >= 0.5
    w0, col = q.weights.cpu().numpy()[floor], ch.color.cpu().numpy()[floor]
    assert mine[:, 9:12].tobytes() == (w0 * col).astype(F).view(np.uint32).tobytes()


def run_levels(miro, name, env, kinds, levels, w=48, h=32, spp=2, all_lowres=False, has=ALL_KINDS):
    """`levels` levels on the same queues, the fused queue (with its low-res byte) feeding the next level of both routes;
    returns per level the Chain"""
    from miro_amd import binding
    scene, desc, lights = use(miro, name, env)
    q = eye_queue(scene, desc, w, h, spp)
    seen = []
    for level in range(levels):
        fl = binding.MR_TRACE_INCOHERENT if level > 0 else 0
        low_all = all_lowres and level > 0
        if low_all:
            q = q._replace(low=None)                            # the flag alone says it
        ch = Chain(scene, len(lights), q, spp, fl, ENVS[env], w * h, kinds=kinds, bounce=level, all_lowres=low_all)
        fu = Fused(scene, q, spp, fl, ENVS[env], w * h, kinds=kinds, bounce=level, all_lowres=low_all)
        low = np.zeros(q.n, bool) if q.low is None else q.low.cpu().numpy() != 0
        miss = ~ch.hit_rows.cpu().numpy()
        print("%s env=%s kinds=%d level %d: %d rays, %d hits, children per kind %s, counters %s; misses of diffuse rays %d, of others %d" %
              (name, env, kinds, level, q.n, ch.n_hits, ch.per_kind(), ch.counted, (miss & low).sum(), (miss & ~low).sum()))
        ch.assert_not_empty(env=ENVS[env] is not None, has=has)
        assert_level_is_the_chain(fu, ch)
        seen.append((ch, int((miss & low).sum()), int((miss & ~low).sum())))
        q = fu.next_queue()
    return seen


@pytest.mark.gpu
def test_flower_with_drops_under_an_image_carries_the_lowres_byte(miro):
    """flower_scene(drops=True) under a 48 x 24 image, kinds = MIRROR | REFRACT | DIFFUSE, 48 x 32 x 2 eye rays and the two levels
    after them.  At every level d_out_lowres is 1 exactly on the children whose id is child_id(parent, 3) (assert_level_is_the_chain)
    -- the id set of a kinds = DIFFUSE run, asserted here at the first level -- and the next level is fed that mask: its misses
    equal mr_shade_environment with the same d_lowres, low-res lookups and full ones both occurring."""
    seen = run_levels(miro, "flower_drops", "image", ALL_KINDS, 3, has=6)      # water: kd and kt, no ks
    assert seen[0][1] == 0 and seen[0][2] > 0                                     # eye rays are never isDiffuse
    assert seen[1][1] > 0 and seen[1][2] + seen[2][2] > 0                         # diffuse rays that miss, and others that do
    scene, desc, lights = use(miro, "flower_drops", "image")
    first = seen[0][0]
    only = Chain(scene, len(lights), first.q, 2, 0, ENVS["image"], 48 * 32, kinds=4)
    diffuse_ids = first.rows[np.isin(first.rows[:, 0], child_id(parent_ids(first.q)[first.hit_rows.cpu().numpy()], 3)), 0]
    assert np.array_equal(np.sort(diffuse_ids), only.rows[:, 0]) and len(diffuse_ids) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["image", "colour"])
def test_all_diffuse_queues_take_the_flag(miro, env):
    """kinds = DIFFUSE on the flower: every ray after the first level is isDiffuse, said by MR_ENV_LOWRES instead of a mask -- the
    chain's mr_shade_environment takes the same flag.  Under the image every miss of level 1 reads the low-res copy; under a
    colour the flag changes nothing."""
    seen = run_levels(miro, "flower_drops", env, 4, 2, all_lowres=True)
    assert seen[1][0].n - seen[1][0].n_hits > 0


@pytest.mark.gpu
def test_without_a_texture_table_the_children_are_the_plain_generators(miro):
    """The untextured room with glass and mirror spheres (disc + point light), kinds = MIRROR | REFRACT: the level is the chain's,
    and the children are mr_gen_path_rays' set on the same hits, with explicit weights, pixels and ids."""
    import torch
    scene, desc, lights = plain_scene_of(miro, "photon_room_two_lights")
    scene.set_lights(lights)
    scene.set_environment()
    assert not scene.n_textures
    q = explicit(eye_queue(scene, desc, 48, 32), 5)
    ch = Chain(scene, len(lights), q, 1, 0, None, 1000, kinds=3, bounce=1)
    ch.assert_not_empty()
    fu = Fused(scene, q, 1, 0, None, 1000, kinds=3, bounce=1)
    assert_level_is_the_chain(fu, ch)
    plain = (torch.empty((4 * q.n, 8), dtype=torch.float32, device="cuda"), torch.empty((4 * q.n, 3), dtype=torch.float32, device="cuda"),
             torch.empty(4 * q.n, dtype=torch.int32, device="cuda"), torch.empty(4 * q.n, dtype=torch.int32, device="cuda"),
             torch.empty(4 * q.n, dtype=torch.uint8, device="cuda"))
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    scene.gen_path_rays(q.rays, ch.hits, q.weights, q.pixels, q.ids, q.n, *plain[:4], cnt, bounce=1, kinds=3, d_out_octants=plain[4])
    torch.cuda.synchronize()
    assert int(cnt.item()) == fu.n_children and np.array_equal(rows_of(plain, fu.n_children), fu.rows())


@pytest.mark.gpu
def test_one_ray_per_pixel_is_one_add_per_pixel(miro):
    """teapot_textured under the image at 1 spp, NULL weights and pixels: every pixel receives one addition, so d_rgb is the
    chain's bit for bit.  With d_rgb NULL the per-ray outputs are unchanged."""
    scene, desc, lights = use(miro, "teapot_textured", "image")
    q = eye_queue(scene, desc, 48, 32)
    ch = Chain(scene, len(lights), q, 1, 0, ENVS["image"], q.n, kinds=3)
    assert ch.per_kind()[0] > 0 and 0 < ch.n_hits < ch.n and float(ch.rgb.max()) > 0
    fu = Fused(scene, q, 1, 0, ENVS["image"], q.n, kinds=3)
    assert_level_is_the_chain(fu, ch, exact_rgb=True)
    no_rgb = Fused(scene, q, 1, 0, ENVS["image"], q.n, kinds=3, children=False, rgb=False)
    assert same(no_rgb.ray_rgb, fu.ray_rgb) and np.array_equal(bits(no_rgb.hits), bits(fu.hits)) and no_rgb.counted == fu.counted


@pytest.mark.gpu
def test_an_empty_queue(miro):
    """n == 0 is MR_OK, launches nothing and zeroes d_out_count on a level with children"""
    import torch
    from miro_amd import binding
    scene, desc, lights = use(miro, "mixed", None)
    rays = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
    rgb = torch.zeros((64, 3), dtype=torch.float32, device="cuda")
    out = (torch.empty((256, 8), dtype=torch.float32, device="cuda"), torch.empty((256, 3), dtype=torch.float32, device="cuda"),
           torch.empty(256, dtype=torch.int32, device="cuda"))
    count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
    counts = torch.zeros(5, dtype=torch.int64, device="cuda")
    scene.trace_level_lights_path(rays, None, None, None, 0, rgb, children=binding.MR_LEVEL_PATH, d_out_rays=out[0], d_out_weights=out[1],
                                  d_out_pixels=out[2], d_out_count=count, d_counts=counts)
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and counts.tolist() == [0] * 5 and float(rgb.abs().max()) == 0.0
    scene.set_lights([])
    with pytest.raises(miro.MiroError) as e:
        scene.trace_level_lights_path(rays, None, None, None, 64, rgb)
    assert e.value.status == binding.MR_ERR_STATE and "no lights" in str(e.value) and NAME in str(e.value)
    scene.set_lights(lights)


@pytest.mark.gpu
def test_replays_from_a_captured_graph(miro):
    """After one warm call outside the capture (it uploads the texture table) one level of the mixed room with children is captured
    into a torch.cuda.graph on one stream and replayed twice, the outputs filled with sentinels and d_out_count with a wrong value
    before each replay: per-ray outputs and the child set equal the direct launch, d_out_count is zeroed by each replay."""
    import torch
    scene, desc, lights = use(miro, "mixed", None)
    q = eye_queue(scene, desc, 64, 32)
    ch = Chain(scene, len(lights), q, 1, 0, None, q.n)
    ch.assert_not_empty()
    fu = Fused(scene, q, 1, 0, None, q.n)                        # the warm call, a direct launch
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
        fu.out[3].fill_(ID)
        fu.out[4].fill_(BYTE)
        fu.out_low.fill_(BYTE)
        fu.count.fill_(999999)
        fu.rgb.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fu.n_children = int(fu.count.item())
        assert_level_is_the_chain(fu, ch)


def frames(miro, name, env, w, h, spp, depth, kinds):
    """render_specular(fused="lights_path") and the batched route with surface_children=True: (per_level, pixels) of each"""
    import torch
    from miro_amd import frame
    scene, desc, lights = use(miro, name, env)
    fr = frame.FrameRenderer(scene, desc, w, h, spp=spp, tiled=False)
    fr.generate()
    out = []
    for kw in (dict(fused="lights_path"), dict(fused=False, surface_children=True)):
        per_level = fr.render_specular(depth=depth, lights=lights, environment=ENVS[env], path_tracing=True, path_kinds=kinds, path_seed=29,
                                       **kw)
        torch.cuda.synchronize()
        out.append((per_level, fr.d_rgb.clone()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,kinds,depth", [("stone", None, ALL_KINDS, 2), ("flower_drops", "colour", ALL_KINDS, 3),
                                                  ("teapot_textured", "image", 3, 2), ("flower_drops", "image", 4, 2)])
def test_whole_frames(miro, name, env, kinds, depth):
    """render_specular(fused="lights_path") against fused=False, surface_children=True with the same seed at 48 x 32 x 2: the same
    rays and shadow rays per level, pixels within 2e-5 of the largest value (the whole-frame bound of tests/test_level_lights.py).
    Under an image the batched driver serves specular kinds (full image) and kinds = DIFFUSE (MR_ENV_LOWRES) only."""
    (levels_f, rgb_f), (levels_b, rgb_b) = frames(miro, name, env, 48, 32, 2, depth, kinds)
    print("per_level", levels_b, "max", float(rgb_b.max()))
    assert levels_f == levels_b and len(levels_b) == depth + 1 and all(n > 0 for n, _ in levels_b)
    top = float(rgb_b.abs().max())
    assert top > 0 and float((rgb_f - rgb_b).abs().max()) <= 2e-5 * top, float((rgb_f - rgb_b).abs().max()) / top


@pytest.mark.gpu
def test_mixed_kinds_frame_under_an_image_against_launches_by_hand(miro):
    """The flower with drops under an image with kinds = MIRROR | REFRACT | DIFFUSE: the batched driver refuses it (ValueError),
    fused="lights_path" renders it.  The batched launches are made by hand, level by level, with the mask a level's children
    need -- 1 where the child's id is child_id(parent, 3): the same rays and shadow rays per level, both kinds of miss occur,
    pixels within the whole-frame bound."""
    import torch
    from miro_amd import binding, frame
    scene, desc, lights = use(miro, "flower_drops", "image")
    w, h, spp, depth = 48, 32, 2, 2
    fr = frame.FrameRenderer(scene, desc, w, h, spp=spp, tiled=False)
    fr.generate()
    kw = dict(depth=depth, lights=lights, environment=ENVS["image"], path_tracing=True, path_kinds=ALL_KINDS, path_seed=29)
    with pytest.raises(ValueError):
        fr.render_specular(fused=False, surface_children=True, **kw)
    per_level = fr.render_specular(fused="lights_path", **kw)
    torch.cuda.synchronize()
    got = fr.d_rgb.clone()
    f32 = dict(dtype=torch.float32, device="cuda")
    rgb = torch.zeros((w * h, 3), **f32)
    q = Q(fr.d_rays, None, None, None, None, fr.n)
    by_hand, low_misses, full_misses = [], 0, 0
    for level in range(depth + 1):
        n = q.n
        fl = binding.MR_TRACE_INCOHERENT if level > 0 else 0
        hits, color, normal = torch.empty((n, 4), **f32), torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
        cnt, cnt2 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        scene.trace_device(q.rays, n, hits, fl)
        scene.shade_environment(q.rays, hits, n, rgb, d_weights=q.weights, d_pixels=q.pixels, d_lowres=q.low, spp=spp)
        scene.hit_surface(q.rays, hits, n, color, normal)
        scene.shade_lights_surface(q.rays, hits, color, normal, n, rgb, d_weights=q.weights, d_pixels=q.pixels, spp=spp, flags=fl, d_counts=cnt)
        by_hand.append((n, int(cnt.item())))
        miss = bits(hits)[:, 1] == MISS
        low = np.zeros(n, bool) if q.low is None else q.low.cpu().numpy() != 0
        low_misses, full_misses = low_misses + int((miss & low).sum()), full_misses + int((miss & ~low).sum())
        if level == depth:
            break
        out = (torch.empty((4 * n, 8), **f32), torch.empty((4 * n, 3), **f32), torch.empty(4 * n, dtype=torch.int32, device="cuda"),
               torch.empty(4 * n, dtype=torch.int32, device="cuda"))
        scene.gen_path_rays_surface(q.rays, hits, color, normal, q.weights, q.pixels, q.ids, n, *out, cnt2, spp=spp, seed=29, bounce=level,
                                    kinds=ALL_KINDS)
        m = int(cnt2.item())
        mask = np.isin(out[3][:m].cpu().numpy().view(np.uint32), child_id(parent_ids(q), 3)).astype(np.uint8)
        q = Q(out[0][:m], out[1][:m], out[2][:m], out[3][:m], cuda(mask), m)
    torch.cuda.synchronize()
    print("per_level", by_hand, "misses of diffuse rays", low_misses, "of others", full_misses)
    assert per_level == by_hand and len(by_hand) == depth + 1 and low_misses > 0 and full_misses > 0
    top = float(rgb.abs().max())
    assert top > 0 and float((got - rgb).abs().max()) <= 2e-5 * top, float((got - rgb).abs().max()) / top
