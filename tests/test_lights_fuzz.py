"""Differential fuzzing of the light-list kernels -- mr_shade_lights, mr_render_lights[_surface|_environment],
mr_trace_level_lights[_path], mr_render_level_lights, mr_render_recursion -- on the tie and special-value scenes of
tests/test_gpu_fuzz.py: grid soups with exact ties, duplicated and zero-area triangles, radius-0 spheres, planes, leaf sizes
1 to 8, and here besides a tenth of every mesh's triangles with ZERO vertex normals (NaN hit normals), random material tables,
3 to 8 mixed point and disc lights (one point light exactly on a mesh vertex, disc normals neither unit nor axis-aligned),
windows narrower than a wave, environments and texture tables.

Two yardsticks, neither of which is the code under test:
  * the ORACLE and the RESTATEMENT of Phong.cpp:78-156 (tests/test_lights.py: restate_shade, RTOL, ATOL_OF_MAX), which see the
    code that every light-list kernel shares (mr_phong.h, mr_light_loop.h, mr_surface.h) and that a fused-against-batched
    comparison cannot see;
  * the BATCHED CHAINS of tests/test_frame_lights*.py, tests/test_level_lights*.py, tests/test_frame_level_lights.py and
    tests/test_recursion_device.py (imported, not copied), bit for bit, NaN compared by position.

No tolerance of its own: shaded values RTOL / ATOL_OF_MAX x max, atomic pixel sums rtol 1e-5 / atol 1e-6 x max, everything else
exact.  A (ray, light) pair is left out of the comparison with the restatement only where the restatement itself is fragile or
non-finite; test_the_reference_can_carry_the_comparison counts those pairs over the default seeds and caps them.

MIRO_FUZZ_SEEDS / MIRO_FUZZ_BASE as in tests/test_gpu_fuzz.py; the scenes are those of seed BASE + OFFSET + k."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_frame_lights as FL  # noqa: E402
import test_frame_lights_environment as FE  # noqa: E402
import test_frame_lights_surface as FS  # noqa: E402
from test_frame_lights import MISS, SENTINEL, bits, camera, same  # noqa: E402
from test_gpu_fuzz import BASE, SEEDS, make_scene, replay  # noqa: E402
from test_lights import ATOL_OF_MAX, RTOL, Room, restate_shade  # noqa: E402
from test_specular import clamp_like_phong_ctor  # noqa: E402

F = np.float32
OFFSET = 3000000                                        # the scenes of this file: seeds BASE + OFFSET + k
DEFAULT_BASE = 1680                                     # MIRO_FUZZ_BASE's default: the census and the regression case name their seeds
NONE = 0xFFFFFFFF
INF = float("inf")
ENVIRONMENTS = (None, "colour", "image")               # none; bg_color; the 48 x 24 seeded image of test_frame_lights_environment
BRANCHES = ("lit_inside", "outside", "opaque", "refractive")
MAX_SAMPLES = 4096                                      # of the largest window: sixteen workgroups and a ragged one
FRAGILE_CAP, NONFINITE_CAP, LIT_FLOOR = 1e-3, 0.10, 0.05


# ---- the case generator ----------------------------------------------------------------------------------------------------
class FuzzRoom(Room):
    """tests/test_lights.py's Room over an oracle scene that is already built: the material of a hit as restate_shade asks"""

    def __init__(self, po, scene, mats, prim_mat, n_planes):
        self.po, self.scene = po, scene
        self.mats = clamp_like_phong_ctor(mats)
        self.prim_mat = np.asarray(prim_mat, np.uint32)
        self.plane_mat = np.zeros(n_planes, np.uint32)  # add_plane's default material


def zero_some_normals(rng, steps):
    """a tenth of each mesh's triangles get (0, 0, 0) at all three vertex normals: HitInfo::N is 0 there, normalised NaN"""
    out = []
    for st in steps:
        if st[0] == "mesh":
            _, v, n, f = st
            n = n.copy()
            tris = rng.choice(len(f), max(1, len(f) // 10), replace=False)
            n[f[tris].reshape(-1)] = 0.0
            st = ("mesh", v, n, f)
        out.append(st)
    return out


def random_materials(rng):
    n_mat = int(rng.integers(1, 6))
    mats = []
    for _ in range(n_mat):
        kd = tuple(float(x) for x in rng.random(3))
        ks = tuple(float(x) for x in rng.random(3) * rng.choice([0.0, 0.6]))
        kt = tuple(float(x) for x in rng.random(3) * rng.choice([0.0, 0.9]))
        mats.append((kd, ks, kt, float(rng.choice([1.0, 5.0, 200.0, INF])), float(rng.choice([1.0, 1.33, 1.5]))))
    if not any(max(m[2]) > 0 for m in mats):            # the refractive variant has a refractive material
        kd, ks, _, sh, ri = mats[-1]
        mats[-1] = (kd, ks, tuple(float(x) for x in 0.05 + rng.random(3) * 0.85), sh, ri)
    return mats


def random_window(rng, accept):
    while True:
        W, H, spp = int(rng.integers(1, 49)), int(rng.integers(1, 33)), int(rng.choice([1, 4, 64]))
        if accept(W * H * spp):
            return W, H, spp


def point_candidate(rng, extent):
    return dict(position=tuple(float(x) for x in ((rng.random(3) - 0.5) * 3 * extent).astype(F)),
                color=tuple(float(x) for x in (0.2 + 0.8 * rng.random(3)).astype(F)), wattage=float(rng.choice([10.0, 80.0, 700.0])))


def disc_candidate(rng, extent, verts):
    """a disc somewhere around the scene that faces one of its vertices; the normal has a random length in [0.3, 2.5] (the
    shadow ray's tMax, Phong.cpp:97) and, being a difference of generic points, no zero component"""
    pos = ((rng.random(3) - 0.5) * 3 * extent).astype(F)
    to = verts[int(rng.integers(0, len(verts)))] - pos + (rng.random(3) - 0.5).astype(F) * F(0.01 * extent)
    nrm = (to / np.linalg.norm(to) * (0.3 + 2.2 * rng.random())).astype(F)
    assert np.all(nrm != 0) and abs(float(np.linalg.norm(nrm)) - 1.0) > 1e-3
    return dict(position=tuple(float(x) for x in pos), normal=tuple(float(x) for x in nrm),
                color=tuple(float(x) for x in (0.2 + 0.8 * rng.random(3)).astype(F)), wattage=float(rng.choice([10.0, 80.0, 700.0])),
                radius=float(F(extent * (0.3 + 1.2 * rng.random()))))


class Case:
    """Everything seed k decides, and the oracle's side of it: the construction steps, two material tables (as drawn, and with
    kt = 0 everywhere), the light list, three cameras with one window each, an environment, on half of the seeds a texture
    table (the odd seeds); the oracle scene, its eye rays and hit records per camera, and the restatement of every light on them."""

    def __init__(self, oracle, seed):
        self.seed = seed
        rng = np.random.default_rng(self.seed)
        steps, self.leaf, extent = make_scene(rng)
        self.steps, self.extent = zero_some_normals(rng, steps), extent
        self.verts = np.concatenate([st[1] for st in self.steps if st[0] == "mesh"])
        self.n_tris = sum(len(st[3]) for st in self.steps if st[0] == "mesh")
        self.n_prims = self.n_tris + sum(1 for st in self.steps if st[0] == "sphere")
        self.n_planes = sum(1 for st in self.steps if st[0] == "plane")
        self.mats = random_materials(rng)
        self.mats_opaque = [(kd, ks, (0.0, 0.0, 0.0), sh, ri) for kd, ks, _, sh, ri in self.mats]
        self.prim_mat = rng.integers(0, len(self.mats), self.n_prims).astype(np.uint32)
        # ---- three cameras, one window each: less than a wave; more than a workgroup and ragged; the 5 x 1 x 64 shape
        shapes = [random_window(rng, lambda n: n < 64), random_window(rng, lambda n: 256 < n <= MAX_SAMPLES and n % 256 != 0), (5, 1, 64)]
        self.views = []
        for W, H, spp in shapes:
            eye = ((rng.random(3) - 0.5) * 4 * extent).astype(F)
            desc = dict(eye=[float(x) for x in eye], lookat=[float(x) for x in (rng.random(3) - 0.5) * extent], up=[0.0, 1.0, 0.0],
                        fov=float(rng.choice([20.0, 45.0, 90.0, 140.0])))
            self.views.append(dict(desc=desc, W=W, H=H, spp=spp, tiled=bool(rng.random() < 0.5), flags=int(rng.choice([0, 1, 2, 3])),
                                   y0=int(rng.integers(0, H)), band=int(rng.integers(1, 9)), kinds=int(rng.integers(1, 8)),
                                   path_seed=int(rng.integers(0, 2 ** 31))))
        for v in self.views:
            v["y1"] = int(rng.integers(v["y0"] + 1, v["H"] + 1))
        self.environment = ENVIRONMENTS[seed % 3]       # by the seed, not drawn: any three seeds in a row have all three
        # ---- the oracle's scene, rays and records
        self.scene = replay(oracle.Scene(), self.steps, self.leaf)
        self.room = FuzzRoom(oracle, self.scene, self.mats, self.prim_mat, self.n_planes)
        for v in self.views:
            d = v["desc"]
            v["rays"] = oracle.eye_rays(oracle.make_camera(d["eye"], d["lookat"], d["up"], d["fov"]), v["W"], v["H"], spp=v["spp"],
                                        jitter=v["spp"] > 1, seed=168)
            v["hits"] = self.scene.trace(v["rays"])
        self.all_rays = np.concatenate([v["rays"] for v in self.views])
        self.all_hits = np.concatenate([v["hits"] for v in self.views])
        # ---- the lights: a point and a disc light that light something, a point light ON a mesh vertex, then random ones
        n_lights = int(rng.integers(3, 9))
        if seed % 4 == 0:                               # every fourth seed: a full list, MR_MAX_LIGHTS
            n_lights = 8
        self.lights = [self.choose(rng, lambda: point_candidate(rng, extent)), self.choose(rng, lambda: disc_candidate(rng, extent, self.verts)),
                       dict(point_candidate(rng, extent), position=tuple(float(x) for x in self.verts[int(rng.integers(0, len(self.verts)))]))]
        while len(self.lights) < n_lights:
            self.lights.append(point_candidate(rng, extent) if rng.random() < 0.5 else disc_candidate(rng, extent, self.verts))
        order = rng.permutation(n_lights)
        self.lights = [self.lights[i] for i in order]
        self.textures = self.random_textures(rng) if seed % 2 == 1 else None
        self._restated = {}

    def choose(self, rng, draw):
        """the first of up to 8 candidates for which the restatement, with the oracle alone, lights at least 5 % of the rays that
        hit; the best of the 8 otherwise"""
        n_hit = max(1, int((self.all_hits["prim"] != MISS).sum()))
        best, best_lit = None, -1
        for _ in range(8):
            light = draw()
            L, _ = restate_shade(self.room, self.all_rays, self.all_hits, light)
            with np.errstate(invalid="ignore"):
                lit = int((np.nan_to_num(L, nan=0.0, posinf=1.0).max(axis=1) > 0).sum())
            if lit > best_lit:
                best, best_lit = light, lit
            if lit >= LIT_FLOOR * n_hit:
                break
        return best

    def random_textures(self, rng):
        """(textures, material_texture, texcoords, tidx): the three UVW kinds on a random subset of the materials, a CHECKER and a
        STEM over random grid-valued texture coordinates on every mesh triangle, STONE only on a material with ks = kt = 0"""
        e = self.extent
        pivot = lambda: tuple(float(x) for x in ((rng.random(3) - 0.5) * e).astype(F))          # noqa: E731
        textures = [dict(petal=(pivot(), float(F(e * (0.5 + rng.random()))))), dict(leaf=float(rng.choice([0.5, 2.0, 7.0]))),
                    dict(flower_center=(pivot(), float(F(e * (0.5 + rng.random()))))),
                    dict(color1=(0.9, 0.8, 0.7), color2=(0.2, 0.3, 0.5), scale=float(rng.choice([0.5, 1.0, 2.0]))),
                    dict(stem=float(rng.choice([1.0, 7.5]))),
                    dict(stone=float(rng.choice([3.0, 20.0])))]
        material_texture = []
        for kd, ks, kt, sh, ri in self.mats:
            diffuse_only = max(ks) == 0 and max(kt) == 0
            pick = int(rng.integers(0, 7))              # 6: plain Phong
            if pick == 5 and not diffuse_only:
                pick = int(rng.integers(0, 5))
            material_texture.append(NONE if pick == 6 else pick)
        texcoords = (rng.integers(-4, 5, (3 * self.n_tris, 2)) * 0.5).astype(F)
        tidx = np.full((self.n_prims, 3), NONE, np.uint32)
        at, prim = 0, 0
        for st in self.steps:                           # addObject order: a mesh's triangles, then the spheres that follow it
            if st[0] == "mesh":
                for _ in range(len(st[3])):
                    tidx[prim] = (at, at + 1, at + 2)
                    at, prim = at + 3, prim + 1
            elif st[0] == "sphere":
                prim += 1
        return textures, np.asarray(material_texture, np.uint32), texcoords, tidx

    def environment_args(self):
        return {None: {}, "colour": dict(bg_color=FE.BG), "image": dict(pixels=FE.image(self.seed), rotation=FE.ROTATION)}[self.environment]

    def restated(self, view, light):
        """restate_shade of light `light` of the list on the rays of view `view`, computed once"""
        if (view, light) not in self._restated:
            v = self.views[view]
            self._restated[view, light] = restate_shade(self.room, v["rays"], v["hits"], self.lights[light])
        return self._restated[view, light]


_CASES, _PRODUCT = {}, {}


def case_of(oracle, k, base=None):
    """the case of seed BASE + OFFSET + k (base: of another first seed than MIRO_FUZZ_BASE's), made once"""
    seed = (BASE if base is None else base) + OFFSET + k
    if seed not in _CASES:
        _CASES[seed] = Case(oracle, seed)
    return _CASES[seed]


def product_of(miro, case, opaque=False, textured=False):
    """the product's scene of a case: the same construction steps, the material table as drawn or with kt = 0, with or without
    the case's texture table; the lights set; the environment NOT set (the tests that want it set it)"""
    key = (case.seed, opaque, textured and case.textures is not None)
    if key not in _PRODUCT:
        s = replay(miro.Scene(0), case.steps, case.leaf)
        mats = case.mats_opaque if opaque else case.mats
        if key[2]:
            textures, material_texture, texcoords, tidx = case.textures
            s.set_texcoords(texcoords, tidx)
            s.set_materials(mats, case.prim_mat)
            s.set_textures(textures, material_texture)
        else:
            s.set_materials(mats, case.prim_mat)
        s.set_lights(case.lights)
        _PRODUCT[key] = s
    return _PRODUCT[key]


def miro_max_lights():
    from miro_amd import binding
    return binding.MR_MAX_LIGHTS


def finite_rows(a):
    return np.isfinite(a).all(axis=1)


# ---- 1. without a GPU: the reference can carry the comparison --------------------------------------------------------------
def test_the_reference_can_carry_the_comparison(oracle):
    """The oracle and the restatement alone, over the default 8 seeds (whatever MIRO_FUZZ_SEEDS and MIRO_FUZZ_BASE say), every light of every list
    on every view's rays.  The unit is the (ray, light) pair, which is what the GPU comparison leaves out or keeps:
      * fragile pairs (disc test within 1e-5 radius^2 of its threshold, a refractive occluder's dot(N, l) within 1e-6 of 0 or
        epsilon) are at most 0.1 % of the pairs -- tests/test_lights.py's own figure;
      * pairs whose restated L is not finite are more than 0 and at most 10 % (a light on the surface: falloff = 0; a refractive
        occluder with a NaN normal: intensity = NaN);
      * pairs with L > 0 are at least 5 % of the pairs whose ray hit;
      * every branch occurs: lit inside the disc, outside it, opaque-occluded, refractive-occluded.
    The figures it prints are recorded in DESIGN.md section 5."""
    pairs = hit_pairs = fragile = nonfinite = lit = nan_normals = 0
    seen = dict.fromkeys(BRANCHES, 0)
    for k in range(8):
        case = case_of(oracle, k, base=DEFAULT_BASE)
        per_seed = [0, 0]
        for vi, v in enumerate(case.views):
            n_hit = int((v["hits"]["prim"] != MISS).sum())
            hit = v["hits"]["prim"] != MISS
            if n_hit:
                _, N = case.scene.hit_attrs(v["hits"][hit], v["rays"][hit])
                nan_normals += int((~(N != 0).any(axis=1)).sum())
            for li in range(len(case.lights)):
                L, info = case.restated(vi, li)
                bad = ~finite_rows(L)
                pairs, hit_pairs = pairs + len(L), hit_pairs + n_hit
                fragile, nonfinite = fragile + int(info["fragile"].sum()), nonfinite + int(bad.sum())
                per_seed = [per_seed[0] + len(L), per_seed[1] + int(bad.sum())]
                with np.errstate(invalid="ignore"):
                    lit += int((np.nan_to_num(L, nan=0.0, posinf=1.0).max(axis=1) > 0).sum())
                assert (L[~hit] == 0).all()
                for b in BRANCHES:
                    seen[b] += int(info[b].sum())
        print("seed %d: %d lights, %s, environment %s, textures %s, %d of %d pairs non-finite" % (
            case.seed, len(case.lights), [(v["W"], v["H"], v["spp"]) for v in case.views], case.environment, case.textures is not None,
            per_seed[1], per_seed[0]))
    print("census: %d pairs (%d on rays that hit, %d rays with a zero normal); fragile %d; non-finite %d; lit %d; branches %s" % (
        pairs, hit_pairs, nan_normals, fragile, nonfinite, lit, seen))
    assert fragile <= FRAGILE_CAP * pairs
    assert 0 < nonfinite <= NONFINITE_CAP * pairs
    assert lit >= LIT_FLOOR * hit_pairs
    assert all(v > 0 for v in seen.values()), seen


def test_the_generator_keeps_its_promises(oracle):
    """Every case: 3 to 8 lights of both kinds, one point light exactly on a mesh vertex, every disc normal neither unit nor
    axis-aligned; a window below a wave, one above a workgroup and ragged, the 5 x 1 x 64 shape; zero normals in every mesh; a
    refractive material in the table as drawn and none in the kt = 0 variant; the environment by seed % 3 and the texture table
    by seed % 2, so that the 8 default seeds hold all six combinations."""
    for k in range(SEEDS):
        c = case_of(oracle, k)
        assert 3 <= len(c.lights) <= 8
        points, discs = [l for l in c.lights if "normal" not in l], [l for l in c.lights if "normal" in l]
        assert points and discs
        assert any((c.verts == np.asarray(l["position"], F)).all(axis=1).any() for l in points)
        for l in discs:
            n = np.asarray(l["normal"], F)
            assert (n != 0).all() and abs(float(np.linalg.norm(n)) - 1.0) > 1e-3 and l["radius"] > 0
        sizes = [v["W"] * v["H"] * v["spp"] for v in c.views]
        assert sizes[0] < 64 and 256 < sizes[1] <= MAX_SAMPLES and sizes[1] % 256 != 0
        assert (c.views[2]["W"], c.views[2]["H"], c.views[2]["spp"]) == (5, 1, 64)
        assert all(1 <= v["W"] <= 48 and 1 <= v["H"] <= 32 and 0 <= v["y0"] < v["y1"] <= v["H"] for v in c.views)
        assert all((st[2][st[3].reshape(-1)] == 0).all(axis=1).any() for st in c.steps if st[0] == "mesh")
        assert any(max(m[2]) > 0 for m in c.mats) and not any(max(m[2]) > 0 for m in c.mats_opaque)
        assert (c.textures is not None) == (c.seed % 2 == 1) and c.environment == ENVIRONMENTS[c.seed % 3]
    # the default campaign: no environment, a colour and the image each meet a scene with and one without a texture table
    default = [case_of(oracle, k, base=DEFAULT_BASE) for k in range(8)]
    assert max(len(c.lights) for c in default) == 8 == miro_max_lights()
    assert {(c.environment, c.textures is not None) for c in default} == {(e, t) for e in ENVIRONMENTS for t in (False, True)}


# ---- 2. the light loop against the restatement -----------------------------------------------------------------------------
def device_view(scene, v, flags=0):
    """the product's own eye rays and hit records of a view, resident on the device"""
    import torch
    n = v["W"] * v["H"] * v["spp"]
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    scene.gen_eye_rays(camera(v["desc"]), v["W"], v["H"], rays, spp=v["spp"], jitter=v["spp"] > 1, seed=168)
    scene.trace_device(rays, n, hits, flags)
    return rays, hits, n


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(SEEDS))
def test_light_loop_matches_the_restatement(oracle, miro, seed):
    """mr_shade_lights, one light at a time, on the product's own eye rays and hit records -- which are first the oracle's bytes --
    against restate_shade: every (ray, light) pair that is neither fragile nor non-finite in the restatement within RTOL and
    ATOL_OF_MAX x the light's largest value; where the restatement is not finite the device is not finite in the same
    components; the shadow counter is the restatement's; a miss is exactly 0.  Then the whole list is the float32 sum of the
    single-light results in list order."""
    from test_lights import shade_lights
    case = case_of(oracle, seed)
    scene = product_of(miro, case)
    left_out = compared = 0
    try:                                                # shade_lights sets one-light lists on the shared scene
        for vi, v in enumerate(case.views):
            rays, hits, n = device_view(scene, v)
            assert rays.cpu().numpy().tobytes() == v["rays"].tobytes() and hits.cpu().numpy().tobytes() == v["hits"].tobytes()
            miss = v["hits"]["prim"] == MISS
            total = np.zeros((n, 3), F)
            shadow = 0
            for li, light in enumerate(case.lights):
                want, info = case.restated(vi, li)
                _, got, counted = shade_lights(scene, rays, hits, n, [light])
                bad = ~finite_rows(want)
                keep = ~info["fragile"] & ~bad
                scale = float(want[keep].max()) if keep.any() else 0.0
                if keep.any():
                    err = np.abs(got[keep].astype(np.float64) - want[keep]) - RTOL * np.abs(want[keep])
                    print("seed %d view %d light %d (%s): %d of %d left out, scale %.4g, worst excess over rtol %.3g (atol %.3g)" % (
                        case.seed, vi, li, "disc" if "normal" in light else "point", (~keep).sum(), n, scale, err.max(), ATOL_OF_MAX * scale))
                assert counted == info["shadow_rays"], (vi, li)
                assert np.isfinite(got[keep]).all() and np.allclose(got[keep], want[keep], rtol=RTOL, atol=ATOL_OF_MAX * scale), (vi, li)
                assert np.array_equal(np.isfinite(got[bad]), np.isfinite(want[bad])), (vi, li)
                assert (got[miss] == 0).all()
                with np.errstate(invalid="ignore"):
                    total = (total + got).astype(F)
                shadow += counted
                left_out, compared = left_out + int((~keep).sum()), compared + int(keep.sum())
            _, whole, counted = shade_lights(scene, rays, hits, n, case.lights)
            assert counted == shadow
            assert np.array_equal(whole, total, equal_nan=True), vi
    finally:
        scene.set_lights(case.lights)
    print("seed %d: %d pairs compared, %d left out" % (case.seed, compared, left_out))
    assert compared > 0


# ---- 3. the fused frames ---------------------------------------------------------------------------------------------------
def sorted_rows(a):
    a = np.ascontiguousarray(a)
    return a[np.lexsort(a.T[::-1])]


def assert_hits_are_the_oracles(fu, v):
    """the frame's primary records against oracle.trace(oracle.eye_rays(...)): in image order directly, in tiled order as a
    multiset (the tiled order permutes whole pixels)"""
    got, want = bits(fu.hits[:fu.n]), v["hits"].view(np.uint32).reshape(-1, 4)
    if v["tiled"]:
        assert np.array_equal(sorted_rows(got), sorted_rows(want))
    else:
        assert np.array_equal(got, want)


def assert_frame_is_the_chain(fu, ch, n_lights, kind):
    """hit records on their bits; per-sample colour and normal (surface and environment frames), the rows of misses untouched;
    per-sample L with NaN by position; pixels against the chain's pairwise tree; every counter.  The sentinel row after each
    buffer is checked by the Fused classes themselves."""
    assert fu.n == ch.n
    assert np.array_equal(bits(fu.hits[:fu.n]), bits(ch.hits))
    if kind != "plain":
        rows = ch.hit_rows
        assert same(fu.color[:fu.n][rows], ch.color[rows]) and same(fu.normal[:fu.n][rows], ch.normal[rows])
        assert bool((fu.color[:fu.n][~rows] == SENTINEL).all()) and bool((fu.normal[:fu.n][~rows] == SENTINEL).all())
    assert same(fu.sample_rgb[:fu.n], ch.ray_rgb)
    assert same(fu.rgb[:fu.n_pixels], ch.rgb)
    want = (ch.n, ch.n_hits * n_lights)
    if kind != "plain":
        want += (ch.undefined,)
    if kind == "environment":
        assert ch.env_counts[0] == ch.n - ch.n_hits
        want += ch.env_counts
    assert fu.counted == want, (fu.counted, want)


def fused(kind, scene, v, lights, flags, **window):
    """the Fused of the kind's own test file on a view; the environment frame takes the scene's lights as they are set"""
    d, W, H, spp, tiled = v["desc"], v["W"], v["H"], v["spp"], v["tiled"]
    scene.set_lights(lights)
    if kind == "environment":
        return FE.Fused(scene, d, W, H, spp, tiled, flags, **window)
    return (FL if kind == "plain" else FS).Fused(scene, d, lights, W, H, spp, tiled, flags, **window)


def chain(miro, kind, scene, v, lights, flags):
    """the batched Chain of the kind's own test file on a view"""
    d, W, H, spp, tiled = v["desc"], v["W"], v["H"], v["spp"], v["tiled"]
    scene.set_lights(lights)
    if kind == "plain":
        return FL.Chain(miro, scene, d, lights, W, H, spp, tiled, flags)
    return FS.Chain(scene, d, lights, W, H, spp, tiled, flags) if kind == "surface" else FE.Chain(scene, d, W, H, spp, tiled, flags)


KINDS = ("plain", "surface", "environment")
PER_SAMPLE = {"plain": ("sample_rgb",), "surface": ("sample_rgb", "color", "normal"), "environment": ("sample_rgb", "color", "normal")}


def assert_same_frame(a, b, kind):
    assert same(a.rgb, b.rgb) and np.array_equal(bits(a.hits), bits(b.hits)) and a.counted == b.counted
    for f in PER_SAMPLE[kind]:
        assert same(getattr(a, f), getattr(b, f)), f


def assert_any_hit_windows_and_bands(miro, kind, scene, opaque, v, lights, flags, fu):
    """MR_TRACE_ANY on the kt = 0 variant is its closest-hit frame in every output and counter (and kt does not enter the primary
    records); rows [y0, y1) and the two ranks' interleaved bands of a random height are those rows of the full frame `fu`"""
    from miro_amd import binding
    W, H, spp, tiled = v["W"], v["H"], v["spp"], v["tiled"]
    # ---- any-hit shadow rays
    closest = fused(kind, opaque, v, lights, flags)
    assert_same_frame(fused(kind, opaque, v, lights, flags | binding.MR_TRACE_ANY), closest, kind)
    assert np.array_equal(bits(closest.hits), bits(fu.hits))                       # kt does not enter the primary records
    # ---- a row window and two ranks' interleaved bands, put back together
    y0, y1, band = v["y0"], v["y1"], v["band"]
    win = fused(kind, scene, v, lights, flags, y0=y0, y1=y1)
    assert same(win.rgb[:win.n_pixels], fu.rgb[y0 * W:y1 * W])
    shards = [fused(kind, scene, v, lights, flags, bands=(band, r, 2), rows=miro.band_rows_of(H, band, r, 2)) for r in range(2)]
    assert sum(s.n_pixels for s in shards) == W * H
    for y in range(H):
        r, j = miro.band_locate(H, band, 2, y)
        assert same(shards[r].rgb[j * W:(j + 1) * W], fu.rgb[y * W:(y + 1) * W]), y
    assert tuple(a + b for a, b in zip(shards[0].counted, shards[1].counted)) == fu.counted
    if not tiled:                                       # image order: the per-sample outputs of a row are that row's
        k = W * spp
        assert np.array_equal(bits(win.hits[:win.n]), bits(fu.hits[y0 * k:y1 * k]))
        for f in PER_SAMPLE[kind]:
            assert same(getattr(win, f)[:win.n], getattr(fu, f)[y0 * k:y1 * k]), f
            for y in range(H):
                r, j = miro.band_locate(H, band, 2, y)
                assert same(getattr(shards[r], f)[j * k:(j + 1) * k], getattr(fu, f)[y * k:(y + 1) * k]), (f, y)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(SEEDS))
def test_fused_frames_match_oracle_and_chain(oracle, miro, seed):
    """mr_render_lights on the scene without a texture table, mr_render_lights_surface and mr_render_lights_environment on the
    scene with the case's table (where it has one) and environment, each view with its own window, sample order and flags:
    primary records against the oracle (exact arithmetic; the product form may differ on ties), everything against the batched
    chain of the kind's own test file; MR_TRACE_ANY on the kt = 0 variant is the closest-hit frame, on the table as drawn
    MR_ERR_STATE; a row window and a two-rank band split reassemble to the full frame (these three on one frame kind per view,
    every kind once per seed: the scenes are slow to trace)."""
    from miro_amd import binding
    case = case_of(oracle, seed)
    lights, n_lights = case.lights, len(case.lights)
    for vi, v in enumerate(case.views):
        W, H, spp, tiled, flags = v["W"], v["H"], v["spp"], v["tiled"], v["flags"]
        flags = (binding.MR_MATH_PRODUCT if flags & 1 else 0) | (binding.MR_TRACE_INCOHERENT if flags & 2 else 0)
        for kind in KINDS:
            textured = kind != "plain"
            scene, opaque = product_of(miro, case, textured=textured), product_of(miro, case, opaque=True, textured=textured)
            for s in (scene, opaque):
                s.set_environment(**(case.environment_args() if kind == "environment" else {}))
            fu, ch = fused(kind, scene, v, lights, flags), chain(miro, kind, scene, v, lights, flags)
            print("seed %d view %d %s %dx%dx%d tiled=%s flags=%d: %d hits, %s" % (case.seed, vi, kind, W, H, spp, tiled, flags, ch.n_hits,
                                                                                  fu.counted))
            if not flags & binding.MR_MATH_PRODUCT:
                assert_hits_are_the_oracles(fu, v)
            assert_frame_is_the_chain(fu, ch, n_lights, kind)
            with pytest.raises(miro.MiroError) as e:    # any-hit shadow rays and a refractive material: refused, nothing launched
                fused(kind, scene, v, lights, flags | binding.MR_TRACE_ANY)
            assert e.value.status == binding.MR_ERR_STATE and "refractive" in str(e.value)
            if kind == KINDS[(vi + seed) % 3]:          # every kind once per seed, every view once: the scenes are slow to trace
                assert_any_hit_windows_and_bands(miro, kind, scene, opaque, v, lights, flags, fu)
            for s in (scene, opaque):
                s.set_environment()


# ---- 4. levels ---------------------------------------------------------------------------------------------------------------
def canonical_nans(*tensors):
    """every NaN of the float tensors becomes the same NaN, in place: queues are then compared by NaN position and bits"""
    import torch
    for t in tensors:
        if t is not None and t.dtype == torch.float32:
            t[torch.isnan(t)] = float("nan")


def finite_pixel_rows(fu, ch):
    """equal finite masks of the two pixel sums; the rows that are not finite are then zeroed on both sides, so that the bound of
    the existing assert_level_is_the_chain (rtol 1e-5, atol 1e-6 x max) applies to the rows that are finite on both"""
    import torch
    a, b = torch.isfinite(fu.rgb).all(dim=1), torch.isfinite(ch.rgb).all(dim=1)
    assert torch.equal(a, b)
    fu.rgb[~a] = 0.0
    ch.rgb[~a] = 0.0
    return int((~a).sum().item())


def level_view(v, binding):
    flags = (binding.MR_MATH_PRODUCT if v["flags"] & 1 else 0) | (binding.MR_TRACE_INCOHERENT if v["flags"] & 2 else 0)
    return v["desc"], v["W"], v["H"], v["spp"], v["tiled"], flags


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(SEEDS))
def test_levels_match_their_chains(oracle, miro, seed):
    """Two levels of mr_trace_level_lights and of mr_trace_level_lights_path (the view's kinds and path seed) on the eye queue of
    each view, the BATCHED queue feeding level 1, each against its chain with the assert_level_is_the_chain of its own test
    file: per-ray outputs and the five counters exact, children as canonical sets by NaN position and bits, pixel sums on the
    rows that are finite on both sides with equal finite masks.  Then mr_render_level_lights: its frame half is
    mr_render_lights_environment's frame, its children are the level kernel's set."""
    import torch
    from miro_amd import binding
    import test_frame_level_lights as FLL
    import test_level_lights as LL
    import test_level_lights_path as PL
    case = case_of(oracle, seed)
    scene = product_of(miro, case, textured=True)
    scene.set_lights(case.lights)
    scene.set_environment(**case.environment_args())
    env, n_lights = case.environment, len(case.lights)
    for vi, v in enumerate(case.views):
        desc, W, H, spp, tiled, flags = level_view(v, binding)
        kinds, path_seed = v["kinds"], v["path_seed"]
        rays, pixels, n = FLL.eye_queue(miro, scene, desc, W, H, spp, tiled)
        # ---- specular children
        q, level0 = (rays, None, pixels, n), {}
        for level in range(2):
            fl = flags | (binding.MR_TRACE_INCOHERENT if level else 0)
            ch = LL.Chain(scene, n_lights, q[0], q[1], q[2], q[3], spp, fl, env, True, W * H)
            fu = LL.Fused(scene, q[0], q[1], q[2], q[3], spp, fl, env, True, W * H)
            canonical_nans(*ch.out[:2], *fu.out[:2])
            dropped = finite_pixel_rows(fu, ch)
            print("seed %d view %d specular level %d: %d rays, counters %s, %d children, %d pixels not finite" % (
                case.seed, vi, level, q[3], ch.counted, ch.n_children, dropped))
            LL.assert_level_is_the_chain(fu, ch)
            assert bool((fu.out[0][fu.n_children:] == SENTINEL).all()) and bool((fu.out[2][fu.n_children:] == LL.PIX).all())
            if level == 0:
                level0["specular"] = fu
            if ch.n_children == 0:
                break
            q = (ch.out[0], ch.out[1], ch.out[2], ch.n_children)
        # ---- path-traced children
        pq = PL.Q(rays, None, pixels, None, None, n)
        for level in range(2):
            fl = flags | (binding.MR_TRACE_INCOHERENT if level else 0)
            ch = PL.Chain(scene, n_lights, pq, spp, fl, env, W * H, kinds=kinds, seed=path_seed, bounce=level)
            fu = PL.Fused(scene, pq, spp, fl, env, W * H, kinds=kinds, seed=path_seed, bounce=level)
            canonical_nans(*ch.out[:2], *fu.out[:2])
            ch.rows = PL.rows_of(ch.out, ch.n_children)
            dropped = finite_pixel_rows(fu, ch)
            print("seed %d view %d path kinds %d level %d: %d rays, counters %s, %d children, %d pixels not finite" % (
                case.seed, vi, kinds, level, pq.n, ch.counted, ch.n_children, dropped))
            PL.assert_level_is_the_chain(fu, ch)
            if level == 0:
                level0["path"] = fu
            m = ch.n_children
            if m == 0:
                break
            ids = ch.out[3][:m].cpu().numpy().view(np.uint32)
            low = np.isin(ids, PL.child_id(PL.parent_ids(pq), 3)).astype(np.uint8)             # ray.isDiffuse: the diffuse bounce's children
            pq = PL.Q(ch.out[0][:m].contiguous(), ch.out[1][:m].contiguous(), ch.out[2][:m].contiguous(), ch.out[3][:m].contiguous(),
                      PL.cuda(low), m)
        # ---- the fused frame that emits level 1
        frame = FE.Fused(scene, desc, W, H, spp, tiled, flags)
        for name, children in (("specular", binding.MR_LEVEL_SPECULAR), ("path", binding.MR_LEVEL_PATH)):
            lv = level0[name]
            fu = FLL.Level0(miro, scene, desc, W, H, spp, tiled, children, env, flags=flags, kinds=kinds, path_seed=path_seed)
            assert fu.n == frame.n and fu.n_pixels == frame.n_pixels and fu.counted == frame.counted
            assert np.array_equal(bits(fu.hits), bits(frame.hits))
            for f in ("rgb", "sample_rgb", "color", "normal"):
                assert same(getattr(fu, f), getattr(frame, f)), (name, f)
            assert fu.n_children == lv.n_children, name
            canonical_nans(*fu.out[:2])
            if name == "specular":
                assert np.array_equal(fu.spec_rows(), LL.rows_of(lv.children()))
            else:
                mine = fu.path_rows()
                assert len(np.unique(mine[:, 0])) == fu.n_children and np.array_equal(mine, lv.rows())
                got_ids, got_low = fu.low_by_id()
                want_ids, want_low = lv.out[3][:lv.n_children].cpu().numpy().view(np.uint32), lv.out_low[:lv.n_children].cpu().numpy()
                order = np.argsort(want_ids, kind="stable")
                assert np.array_equal(got_ids, want_ids[order]) and np.array_equal(got_low, want_low[order])
            assert fu.untouched(fu.n_children)
    scene.set_environment()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_a_child_with_a_nan_weight_that_leaves_the_scene(oracle, miro):
    """The regression case these tests found: seed 3001683 (1680 + OFFSET + 3), view 1 (11 x 31 x 1, no environment), specular
    children.  A refractive hit with a NaN normal has a NaN Fresnel coefficient, so its refraction child carries the weight
    kt (1 - Rs) = NaN (Scene.cpp:316-334); the child leaves the scene, traceScene answers m_bgColor = 0 for it and returns true
    (Scene.cpp:338-342), and the parent adds NaN * 0 = NaN to the pixel.  mr_trace_level_lights did that; mr_shade_lights[_surface]
    skipped every miss and left the pixel finite (store_shaded, csrc/mr_lights_body.h: fixed to form the product for a miss too).
    Level 1 of the batched queue: such rays exist, their pixels are not finite on both sides, and the finite masks agree."""
    import torch
    import test_frame_level_lights as FLL
    import test_level_lights as LL
    from miro_amd import binding
    case = case_of(oracle, 3, base=DEFAULT_BASE)
    assert case.seed == 3001683 and case.environment is None
    scene = product_of(miro, case, textured=True)
    scene.set_lights(case.lights)
    scene.set_environment()
    v = case.views[1]
    desc, W, H, spp, tiled, flags = level_view(v, binding)
    rays, pixels, n = FLL.eye_queue(miro, scene, desc, W, H, spp, tiled)
    ch0 = LL.Chain(scene, len(case.lights), rays, None, pixels, n, spp, flags, None, True, W * H)
    assert ch0.n_children > 0
    q = (ch0.out[0], ch0.out[1], ch0.out[2], ch0.n_children)
    fl = flags | binding.MR_TRACE_INCOHERENT
    ch = LL.Chain(scene, len(case.lights), q[0], q[1], q[2], q[3], spp, fl, None, True, W * H)
    fu = LL.Fused(scene, q[0], q[1], q[2], q[3], spp, fl, None, True, W * H)
    lost = ~ch.hit_rows & ~torch.isfinite(q[1]).all(dim=1)
    assert int(lost.sum()) > 0                          # the case is what it says
    at = q[2][lost].to(torch.int64)
    assert not bool(torch.isfinite(ch.rgb[at]).all(dim=1).any()) and not bool(torch.isfinite(fu.rgb[at]).all(dim=1).any())
    assert torch.equal(torch.isfinite(fu.rgb), torch.isfinite(ch.rgb))


# ---- 5. the one-call recursion ---------------------------------------------------------------------------------------------
DEPTH = 2


def recursion_frames(miro, case, scene, v, children, capacity):
    """test_recursion_device.frames -- render_specular(fused="frame_lights[_path]") and the one call -- on a scene of this file,
    under the case's own environment.  frames() renders in image order with its own path seed (29) and no traversal flags: of
    the view it takes the camera, the window, the samples per pixel and the kinds of path-traced children."""
    import test_recursion_device as RD
    own = (scene, v["desc"], case.lights, case.environment_args() or None)
    return RD.frames(miro, None, None, children, v["spp"], kinds=v["kinds"], depth=DEPTH, capacity=capacity, window=(v["W"], v["H"]), own=own)


def assert_finite_pixels_close(ref, dev):
    """the bound of test_recursion_device.assert_pixels_close on the rows that are finite on both sides, with equal finite masks"""
    import torch
    a, b = torch.isfinite(ref.rgb).all(dim=1), torch.isfinite(dev.rgb).all(dim=1)
    assert torch.equal(a, b)
    x, y = ref.rgb[a], dev.rgb[a]
    scale = float(x.abs().max()) if x.numel() else 0.0
    assert torch.allclose(y, x, rtol=1e-5, atol=1e-6 * scale), float((y - x).abs().max())
    return int((~a).sum().item())


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(SEEDS))
def test_one_call_recursion_matches_the_level_by_level_frame(oracle, miro, seed):
    """mr_render_recursion at depth 2 on each view (specular and path-traced children on the window of more than a workgroup, one
    of the two on each of the others: the scenes are slow to trace), against render_specular(fused=
    "frame_lights[_path]") as tests/test_recursion_device.py's frames() runs the two: words 0 to 5 of every level exact and a
    level's children the next level's rays (assert_counts), pixels within the atomic bound on the rows that are finite on both
    sides with equal finite masks.  queue_capacity = fan^depth x samples: nothing truncates.  With ks = kt = 0 everywhere the
    queue dies: the rows of levels 1 and 2 are all zero and the pixels are level 0's bits."""
    import test_recursion_device as RD
    from miro_amd import binding
    case = case_of(oracle, seed)
    scene = product_of(miro, case, textured=True)
    for vi, v in enumerate(case.views):
        n = v["W"] * v["H"] * v["spp"]
        both = ((binding.MR_LEVEL_SPECULAR, 3), (binding.MR_LEVEL_PATH, 4))
        for children, fan in (both if vi == 1 else both[(vi + seed) % 2:][:1]):   # the ragged window: both; the others: one each
            ref, dev = recursion_frames(miro, case, scene, v, children, fan ** DEPTH * n)
            RD.assert_counts(ref, dev, depth=DEPTH)
            dropped = assert_finite_pixels_close(ref, dev)
            print("seed %d view %d children %d: per level %s, %d pixels not finite" % (case.seed, vi, children, ref.per_level, dropped))
            assert all(row[5] <= fan ** DEPTH * n for row in dev.counts)
    # ---- a queue that dies out
    key = (case.seed, "diffuse")
    if key not in _PRODUCT:
        s = replay(miro.Scene(0), case.steps, case.leaf)
        s.set_materials([(kd, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), sh, ri) for kd, _, _, sh, ri in case.mats], case.prim_mat)
        _PRODUCT[key] = s
    v = case.views[1]
    ref, dev = recursion_frames(miro, case, _PRODUCT[key], v, binding.MR_LEVEL_SPECULAR, 9 * v["W"] * v["H"] * v["spp"])
    assert len(ref.per_level) == 1 and dev.per_level == ref.per_level
    assert dev.counts[0][:6] == ref.counts[0][:6] and dev.counts[0][5] == 0
    assert dev.counts[1:] == [[0] * 8] * DEPTH
    assert same(dev.rgb, ref.rgb)
    scene.set_environment()
