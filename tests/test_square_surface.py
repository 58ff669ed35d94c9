"""mr_shade_square_lights_surface (csrc/mr_square_surface.hip, body in csrc/mr_square_body.h) -- Phong::shade over SquareLights
(SquareLight.h:6-58, Phong.cpp:66-157) with the hit's diffuseColor and N read from the two buffers of mr_hit_surface, the form
of mr_shade_square_lights for a scene with a texture table.

The checker is tests/test_distribution.py's numpy restatement of the square light, generalised to a per-hit colour
(term = color_light * (diff * dc * m_diffuse) * intensity, Phong.cpp:146) and a per-hit N (Phong.cpp:139,151): float32, one
operation per rounding, shadow rays traced by mr_trace.  It is used on scenes whose occluders are all opaque, so the refractive
arm of Phong.cpp:99-113 is not restated here; that arm is covered by comparing with mr_shade_square_lights itself on the scene
with the glass sphere.  Tolerance for shaded values: the project's, RTOL = 1e-5 and ATOL_OF_MAX = 1e-7 times the largest
expected value (tests/test_lights.py:27; powf on the device against pow in the checker needs it)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402
from test_distribution import (ATOL_OF_MAX, EPS, LIGHT_A, LIGHT_B, MISS, PI, RTOL, SquareScene, dot3, host_scene,  # noqa: E402
                               normalised_rows, rays_of, tangents_np)

F = np.float32
NAME = "mr_shade_square_lights_surface"
PLANE_BIT = 0x80000000
NONE = 0xFFFFFFFF


# ---- the restatement -----------------------------------------------------------------------------------------------------
def pairs(n, n_lights, samples, seed):
    """seeded pairs in [0, 1), exactly representable: [n, lights, samples, 2]"""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 1 << 24, size=(n, n_lights, samples, 2)).astype(F) * F(1.0 / 16777216.0)).astype(F)


def restate(scene, ray_dtype, rays, P, N, dc, mt, lights, samples, uv):
    """Phong::shade (Phong.cpp:66-157) over SquareLights for m hits, every occluder opaque: rays [m] the records of the rays that
    hit, P / N / dc [m, 3] the hit point, the normal and the diffuseColor as given, mt [m, 11] the hits' material records,
    uv [m, lights, samples, 2].  Returns (L [m, 3], occluded samples per hit and light [m, lights])."""
    m = len(P)
    L = np.zeros((m, 3), F)
    blocked = np.zeros((m, len(lights)), np.int64)
    e = -np.stack([rays["dx"], rays["dy"], rays["dz"]], 1).astype(F)                        # :49
    shiny = mt[:, 9] < np.inf
    fs = F(samples)
    for j, lt in enumerate(lights):
        pos, color, watt = np.asarray(lt["position"], F), np.asarray(lt.get("color", (1.0, 1.0, 1.0)), F), F(lt["wattage"])
        t1, t2 = tangents_np(lt["normal"])                                                  # SquareLight::preCalc
        dims = np.asarray(lt["dimensions"], F)
        side_length = np.sqrt(F(samples))                                                   # SquareLight.h:27-29
        du, dv = dims[0] / side_length, dims[1] / side_length
        for i in range(samples):
            sx, sy = i % int(side_length), i // int(side_length)                            # :32-33
            u = ((du * uv[:, j, i, 0]) + F(sx) * du) - dims[0] / F(2.0)                     # :35-36
            v = ((dv * uv[:, j, i, 1]) + F(sy) * dv) - dims[1] / F(2.0)
            origin = np.stack([(pos[c] + u * t1[c]) + v * t2[c] for c in range(3)], 1).astype(F)       # :38
            l = (origin - P).astype(F)                                                      # PointLight.h:42
            falloff = dot3(l, l)                                                            # Phong.cpp:85
            length = np.sqrt(falloff)
            l = (l * (F(1) / length)[:, None]).astype(F)                                    # :88
            sh = scene.trace(rays_of(ray_dtype, (P + l * EPS).astype(F), l, length))        # :92, :97: closest hit
            skip = sh["prim"] != MISS                                                       # :99-113, an opaque occluder
            blocked[:, j] += skip
            nDotL = dot3(N, l)                                                              # :139, hit.N
            f2 = F(1.0) / (falloff * F(4.0) * PI * PI)                                      # :140
            diff = np.maximum(F(0), nDotL * f2 * watt / fs)                                 # :146
            term = (color[None, :] * (diff[:, None] * dc * mt[:, 0:3])).astype(F)           # diffuseColor * m_diffuse
            two = 2 * dot3(l, N)
            rv = (-l + two[:, None] * N).astype(F)                                          # :151, hit.N
            edr = np.power(np.maximum(F(0), np.minimum(F(1), dot3(e, rv))), F(500)).astype(F)          # :152
            high = np.where(shiny, np.maximum(F(0), edr * f2 * watt / fs), F(0)).astype(F)  # :154
            keep = ~skip
            L[keep] = (L[keep] + term[keep]).astype(F)                                      # :146, then :155
            L[keep] = (L[keep] + high[keep, None]).astype(F)
    return L, blocked


def surface_of(scene, d_rays, d_hits, n):
    """(d_color, d_normal) of mr_hit_surface; the rows of a miss hold NaN"""
    import torch
    color = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    normal = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    scene.hit_surface(d_rays, d_hits, n, color, normal)
    torch.cuda.synchronize()
    return color, normal


def shade_surface(scene, lights, samples, d_rays, d_hits, d_color, d_normal, n, uv=None, seed=168, weights=None, pixels=None, spp=1,
                  n_pixels=None, flags=0, rgb_fill=0.0):
    """(d_rgb, d_ray_rgb [n], shadow rays) of mr_shade_square_lights_surface as numpy; d_ray_rgb has one sentinel row after n"""
    import torch
    rgb = torch.full((n // spp if n_pixels is None else n_pixels, 3), rgb_fill, dtype=torch.float32, device="cuda")
    ray_rgb = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_uv = torch.from_numpy(np.ascontiguousarray(uv)).cuda() if uv is not None else None
    scene.shade_square_lights_surface(lights, samples, d_rays, d_hits, d_color, d_normal, n, rgb, seed=seed, d_weights=weights,
                                      d_pixels=pixels, d_uv_in=d_uv, spp=spp, flags=flags, d_ray_rgb=ray_rgb, d_counts=cnt)
    torch.cuda.synchronize()
    out = ray_rgb.cpu().numpy()
    assert (out[n] == -7.0).all(), "d_ray_rgb was written beyond 3n floats"
    return rgb.cpu().numpy(), out[:n].copy(), int(cnt.item())


def close(got, want, scale):
    return np.abs(got.astype(np.float64) - want) <= RTOL * np.abs(want) + ATOL_OF_MAX * scale


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_the_surface_square_entry_is_exported_and_declared_outside_miro_hip_h(miro):
    from miro_amd import binding
    L = miro.lib()

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return re.search(r"\b%s\s*\(" % NAME, src) is not None

    assert hasattr(L, NAME) and NAME in binding.SURFACE_SYMBOLS and NAME not in miro.EXPORTED_SYMBOLS
    assert declared("miro_hip_surface.h") and not declared("miro_hip.h")
    assert NAME in open(os.path.join(ROOT, "include", "miro_hip.h")).read()                  # documented there
    assert hasattr(miro.Scene, "shade_square_lights_surface")


def test_surface_square_light_argument_errors(miro):
    """Every MR_ERR_INVALID case of test_square_light_argument_errors gives the same status through the new call, and so do NULL
    or odd-address d_color / d_normal; valid arguments on a host_only or unbuilt scene: MR_ERR_STATE, never a CPU path."""
    from miro_amd import binding
    L = miro.lib()
    s = host_scene(miro)
    dummy = C.c_void_p(64)

    def light(**kw):
        d = binding.square_light_desc(dict(LIGHT_A, **{k: v for k, v in kw.items() if k != "reserved"}))
        d.reserved[:] = kw.get("reserved", (0, 0, 0, 0))
        return d

    def arr(*ls):
        a = (binding.SquareLightDesc * len(ls))()
        for i, l in enumerate(ls):
            a[i] = l
        return a

    def call(lights, n_lights, samples=4, scene=s.h, rays=dummy, hits=dummy, color=dummy, normal=dummy, rgb=dummy, spp=1, flags=0, n=4,
             uv=None):
        return getattr(L, NAME)(scene, lights, n_lights, samples, 168, rays, hits, color, normal, None, None, uv, n, spp, flags, rgb, None,
                                None, None)

    inf, nan = float("inf"), float("nan")
    ok = light()
    for bad in (dict(color=None), dict(normal=None)):
        assert call(arr(ok), 1, **bad) == -1 and b"NULL" in L.mr_last_error(), bad
    for bad in (dict(color=C.c_void_p(66)), dict(normal=C.c_void_p(65)), dict(color=C.c_void_p(67))):
        assert call(arr(ok), 1, **bad) == -1 and b"aligned" in L.mr_last_error(), bad
    assert call(arr(ok), 1, color=C.c_void_p(68), normal=C.c_void_p(76)) == -5                # 4-byte aligned is enough
    assert call(arr(ok), 1, scene=None) == -1 and b"NULL" in L.mr_last_error()
    assert call(None, 1) == -1 and b"NULL" in L.mr_last_error()
    assert call(arr(ok), 0) == -1 and call(arr(*[ok] * 9), 9) == -1 and b"at most" in L.mr_last_error()
    for bad, word in ((light(reserved=(0, 1, 0, 0)), b"reserved"), (light(position=(0, nan, 0)), b"finite"), (light(color=(inf, 1, 1)), b"finite"),
                      (light(wattage=nan), b"finite"), (light(normal=(0, 0, 0)), b"normal"), (light(normal=(0, nan, 0)), b"normal"),
                      (light(dimensions=(-1.0, 1.0)), b"dimensions"), (light(dimensions=(1.0, inf)), b"dimensions"),
                      (light(dimensions=(nan, 1.0)), b"dimensions")):
        assert call(arr(ok, bad), 2) == -1, word
        assert word in L.mr_last_error() and NAME.encode() in L.mr_last_error(), (word, L.mr_last_error())
    for samples in (0, 2, 3, 5, 8, 48, 50, 63, 65, 81, 100):
        assert call(arr(ok), 1, samples=samples) == -1 and b"perfect square" in L.mr_last_error(), samples
    assert call(arr(ok), 1, rays=None) == -1 and call(arr(ok), 1, hits=None) == -1 and call(arr(ok), 1, rgb=None) == -1
    assert call(arr(ok), 1, spp=0) == -1 and call(arr(ok), 1, flags=binding.MR_MATH_FAST) == -1 and call(arr(ok), 1, n=1 << 32) == -1
    assert call(arr(ok), 1, rays=C.c_void_p(8)) == -1 and call(arr(ok), 1, uv=C.c_void_p(4)) == -1 and b"aligned" in L.mr_last_error()
    for samples in (1, 4, 9, 16, 25, 36, 49, 64):                                             # valid, but nothing is on a device
        assert call(arr(ok, light(dimensions=(0.0, 0.0))), 2, samples=samples) == -5, samples
    assert b"CPU" in L.mr_last_error() or b"device" in L.mr_last_error()
    t = miro.Scene()
    t.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    assert call(arr(ok), 1, scene=t.h) == -5 and b"mr_bvh_build" in L.mr_last_error()


def test_square_surface_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_square_surface.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer waves
    per SIMD than BOTH its own record (tests/golden/kernel_budget_square_surface.json, written from the build whose GPU run of
    this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json."""
    cur = kernel_budget.unit_kernels("mr_square_surface")
    assert len(cur) == 12 and all("shade_square_lights_surf_kernel" in k for k in cur)
    for variant in ("ILi1818ELb0E", "ILi1818ELb1E", "ILi826ELb0E", "ILi826ELb1E"):            # triangles / objects, closest / any hit
        assert sum("shade_square_lights_surf_kernel" + variant in k for k in cur) == 1, variant
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_square_surface.json")


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain(miro):
    return SquareScene(miro, sphere=False)


@pytest.fixture(scope="module")
def glass(miro):
    return SquareScene(miro, sphere=True)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["plain", "glass"])
def test_surface_form_reproduces_the_plain_call(request, which):
    """d_color / d_normal from mr_hit_surface on the untextured scene: 2 lights, 4 samples, explicit pairs, weights and a pixel
    permutation at spp = 2 -- d_ray_rgb and d_rgb match mr_shade_square_lights within RTOL / ATOL_OF_MAX, d_counts is equal; with
    d_uv_in NULL and one seed likewise, so the generated pairs are the plain call's.  The glass scene runs the objects variant
    and the refractive arm of Phong.cpp:99-113."""
    sc = request.getfixturevalue(which)
    torch = sc.torch
    n, spp, lights = sc.n, 2, [LIGHT_A, LIGHT_B]
    color, normal = surface_of(sc.scene, sc.d_rays, sc.d_hits, n)
    rng = np.random.RandomState(3)
    w = torch.from_numpy(rng.rand(n, 3).astype(F)).cuda()
    perm = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    for uv, seed in ((sc.uv(2, 4), 168), (None, 7)):
        want_rgb, want, want_cnt = sc.shade(lights, 4, uv=uv, seed=seed, weights=w, pixels=perm, spp=spp, n_pixels=n)
        got_rgb, got, got_cnt = shade_surface(sc.scene, lights, 4, sc.d_rays, sc.d_hits, color, normal, n, uv=uv, seed=seed, weights=w,
                                              pixels=perm, spp=spp, n_pixels=n)
        scale = float(want.max())
        print("%s, %s pairs: largest |difference| per ray %.3g, per pixel %.3g (scale %.4g); %d shadow rays" % (
            which, "explicit" if uv is not None else "generated", np.abs(got - want).max(), np.abs(got_rgb - want_rgb).max(), scale, got_cnt))
        assert scale > 0 and got_cnt == want_cnt == len(sc.idx) * 2 * 4
        assert close(got, want, scale).all() and close(got_rgb, want_rgb, float(want_rgb.max())).all()
        assert (got[sc.hits["prim"] == MISS] == 0).all()
    if which == "glass":
        assert (sc.hits["prim"] == 3).sum() > 0


class Buffers:
    """Seeded colours in [0, 1) and the true normals rotated by a seeded angle of up to 0.3 rad for the hits of a SquareScene,
    NaN at every miss; and the restatement fed them, once per (lights, samples)."""

    def __init__(self, sc):
        rng = np.random.RandomState(11)
        m = len(sc.idx)
        self.sc = sc
        self.dc = rng.rand(m, 3).astype(F)
        N = sc.N.astype(np.float64)
        t = np.cross(N, rng.randn(m, 3))
        t /= np.linalg.norm(t, axis=1)[:, None]
        ang = rng.uniform(0.0, 0.3, m)
        self.N = (N * np.cos(ang)[:, None] + t * np.sin(ang)[:, None]).astype(F)
        self.turned = np.arccos(np.clip((self.N.astype(np.float64) * N).sum(axis=1), -1, 1))
        self.color_full, self.normal_full = np.full((sc.n, 3), np.nan, F), np.full((sc.n, 3), np.nan, F)
        self.color_full[sc.idx], self.normal_full[sc.idx] = self.dc, self.N
        self.d_color, self.d_normal = sc.torch.from_numpy(self.color_full).cuda(), sc.torch.from_numpy(self.normal_full).cuda()
        self._done = {}

    def want(self, lights, samples):
        key = (len(lights), samples)
        if key not in self._done:
            sc = self.sc
            uv = pairs(sc.n, len(lights), samples, 2000 * len(lights) + samples)
            mt = sc.mats[sc.prim_mat[sc.hits["prim"][sc.idx]]]
            L, blocked = restate(sc.scene, sc.miro.RAY_DTYPE, sc.rays[sc.idx], sc.P, self.N, self.dc, mt, lights, samples, uv[sc.idx])
            full, blocked_full = np.zeros((sc.n, 3), F), np.zeros((sc.n, len(lights)), np.int64)
            full[sc.idx], blocked_full[sc.idx] = L, blocked
            self._done[key] = (uv, full, blocked_full)
        return self._done[key]


@pytest.fixture(scope="module")
def buffers(plain):
    assert (plain.mats[:2, 6:9] == 0).all()                                                   # no refractive occluder: restate() holds
    return Buffers(plain)


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [1, 4, 49])
@pytest.mark.parametrize("n_lights", [1, 2])
def test_only_the_buffers_are_read(plain, buffers, samples, n_lights):
    """Random colours and rotated normals in the buffers, NaN at every miss: d_ray_rgb is the generalised restatement's; a miss is
    exactly 0, every output finite, d_counts[0] == hits x lights x samples; and it is not what mr_shade_square_lights gives."""
    lights = [LIGHT_A, LIGHT_B][:n_lights]
    uv, want, blocked = buffers.want(lights, samples)
    rgb, got, counted = shade_surface(plain.scene, lights, samples, plain.d_rays, plain.d_hits, buffers.d_color, buffers.d_normal, plain.n,
                                      uv=uv)
    hit = plain.hits["prim"] != MISS
    scale = float(want.max())
    err = np.abs(got.astype(np.float64) - want) - RTOL * np.abs(want)
    _, material, _ = plain.shade(lights, samples, uv=uv)                                       # the plain call: the material's own light
    print("samples %d, lights %d: %d hits of %d, normals turned by up to %.3f rad, scale %.4g, worst excess over rtol %.3g (atol %.3g); "
          "umbra %d, lit %d" % (samples, n_lights, hit.sum(), plain.n, buffers.turned.max(), scale, err.max(), ATOL_OF_MAX * scale,
                                (hit & (blocked[:, 0] == samples)).sum(), (hit & (blocked[:, 0] == 0)).sum()))
    assert counted == int(hit.sum()) * n_lights * samples and 0 < hit.sum() < plain.n
    assert scale > 0 and buffers.turned.max() > 0.25
    assert (hit & (blocked[:, 0] == samples)).sum() > 0 and (hit & (blocked[:, 0] == 0)).sum() > 0
    assert np.isfinite(got).all() and np.isfinite(rgb).all()
    assert (got[~hit] == 0).all() and (rgb[~hit] == 0).all()
    assert close(got, want, scale).all()
    assert (~close(material, want, scale).all(axis=1))[hit].mean() > 0.5                      # the buffers matter


@pytest.mark.gpu
def test_a_partial_last_workgroup_stays_inside_the_batch(plain, buffers):
    """n = 200 of the 256 rays (kTraceBlock lanes round n up): the sentinel row after d_ray_rgb[n] and rows n.. of a pre-filled
    d_rgb are untouched, rows below n carry fill + L."""
    lights, samples, n = [LIGHT_A, LIGHT_B], 4, 200
    uv, want, _ = buffers.want(lights, samples)
    rgb, got, counted = shade_surface(plain.scene, lights, samples, plain.d_rays, plain.d_hits, buffers.d_color, buffers.d_normal, n,
                                      uv=uv[:n], n_pixels=plain.n, rgb_fill=0.25)
    hit = plain.hits["prim"][:n] != MISS
    scale = float(want.max())
    assert 0 < hit.sum() < n and counted == int(hit.sum()) * 2 * samples
    assert close(got, want[:n], scale).all() and (got[~hit] == 0).all()
    assert (rgb[n:] == 0.25).all()
    assert np.array_equal(rgb[:n], (F(0.25) + got).astype(F))


# ---- the stone floor of assignment1.cpp:229-233 under an opaque sphere -----------------------------------------------------
STONE_CAMERA = dict(eye=(1.0, 4.0, 3.5), lookat=(1.0, -0.5, -2.0), up=(0.0, 1.0, 0.0), fov=30.0)
STONE_SPHERE = ((1.0, 1.5, -2.0), 0.8)
STONE_LIGHT = dict(position=(1.0, 5.0, -2.0), normal=(0.0, -1.0, 0.0), color=(1.0, 0.95, 0.9), wattage=1500.0, dimensions=(1.0, 1.0))
STONE_MATERIALS = [((1.0, 1.0, 1.0), (0, 0, 0), (0, 0, 0), 20.0, 1.0), ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 20.0, 1.0)]
STONE_W = STONE_H = 16


@pytest.mark.gpu
def test_stone_floor_takes_the_bumped_normal(miro):
    """A plane at y = -0.5 with TexturedPhong(StoneTexture(3), ks = 0) and an opaque sphere above it, one square light, 9 samples,
    a 16 x 16 eye batch: shading from mr_hit_surface's buffers equals the generalised restatement fed those buffers; umbra and
    lit floor rays are both present; and fed the normalised geometric normal instead, restatement and device both differ by more
    than the tolerance on at least a tenth of the lit floor rays -- the bump reaches the shade."""
    import torch
    from miro_amd import binding
    from test_procedural import Traced
    s = miro.Scene(0)
    s.add_triangle([40, 0, 40, 41, 0, 40, 40, 1, 40], [0, 0, 1] * 3)                          # far away: a scene needs one bounded object
    s.add_sphere(*STONE_SPHERE)
    s.add_plane((0, 1, 0), (0, -0.5, 0), 0)
    s.build(4)
    s.set_materials(STONE_MATERIALS, [1, 1])
    s.set_textures([dict(stone=3.0)], [0, NONE])
    n, samples = STONE_W * STONE_H, 9
    d_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    s.gen_eye_rays(binding.make_camera(STONE_CAMERA["eye"], STONE_CAMERA["lookat"], STONE_CAMERA["up"], STONE_CAMERA["fov"]), STONE_W, STONE_H,
                   d_rays)
    torch.cuda.synchronize()
    t = Traced(miro, s, d_rays.cpu().numpy().view(miro.RAY_DTYPE).reshape(-1))
    color, normal = surface_of(s, t.rays, t.hits, n)
    idx = np.nonzero(t.hit)[0]
    floor = (t.prim[idx] & PLANE_BIT) != 0
    rows = np.array([list(kd) + list(ks) + list(kt) + [sh, ri] for kd, ks, kt, sh, ri in STONE_MATERIALS], F)
    mt = rows[np.where(floor, 0, 1)]
    uv = pairs(n, 1, samples, 9)
    dc, bumped = color.cpu().numpy()[idx], normal.cpu().numpy()[idx]
    flat = normalised_rows(t.N[idx])
    want, blocked = restate(s, miro.RAY_DTYPE, t.rays_np[idx], t.P[idx], bumped, dc, mt, [STONE_LIGHT], samples, uv[idx])
    want_flat, _ = restate(s, miro.RAY_DTYPE, t.rays_np[idx], t.P[idx], flat, dc, mt, [STONE_LIGHT], samples, uv[idx])
    _, got, counted = shade_surface(s, [STONE_LIGHT], samples, t.rays, t.hits, color, normal, n, uv=uv)
    d_flat = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    d_flat[torch.from_numpy(idx).cuda()] = torch.from_numpy(flat).cuda()
    _, got_flat, _ = shade_surface(s, [STONE_LIGHT], samples, t.rays, t.hits, color, d_flat, n, uv=uv)
    scale = float(want.max())
    umbra, lit = floor & (blocked[:, 0] == samples), floor & (blocked[:, 0] == 0)
    share_want = (~close(want_flat, want, scale).all(axis=1))[lit].mean()
    share_got = (~close(got_flat[idx], got[idx], scale).all(axis=1))[lit].mean()
    print("stone floor: %d hits (%d on the floor, %d on the sphere), umbra %d, lit %d, scale %.4g, largest |difference| %.3g; lit floor "
          "rays that the geometric normal shades differently: restatement %.3f, device %.3f" % (
              len(idx), floor.sum(), (~floor).sum(), umbra.sum(), lit.sum(), scale, np.abs(got[idx] - want).max(), share_want, share_got))
    assert s.procedural and counted == len(idx) * samples and floor.sum() > n // 2 and (~floor).sum() > 0
    assert umbra.sum() > 0 and lit.sum() > 0 and (got[idx][umbra] == 0).all()
    assert close(got[idx], want, scale).all() and (got[~t.hit] == 0).all() and np.isfinite(got).all()
    assert close(got_flat[idx], want_flat, scale).all()
    assert share_want > 0.1 and share_got > 0.1


# ---- frames --------------------------------------------------------------------------------------------------------------
FLOWER_SQUARE = dict(position=(3.0, 14.0, 8.0), normal=(0.0, -1.0, 0.0), color=(1.0, 0.9, 0.8), wattage=4000.0, dimensions=(3.0, 3.0))


@pytest.mark.gpu
def test_flower_frame_with_a_square_light(miro):
    """flower_scene() at 24 x 16, 1 spp, render_specular(depth=1, lights=...) with one square light of 4 samples: it no longer
    raises; d_rgb equals, byte for byte, the same launches made by hand in the driver's order (trace, mr_hit_surface,
    mr_shade_lights_surface, mr_shade_square_lights_surface(seed + level), mr_gen_secondary_rays; two levels at the most); and it
    differs from the frame without the square light."""
    import torch
    from miro_amd import binding, frame, scenes
    s = miro.Scene(0)
    desc = scenes.flower_setup(s)
    W, H = 24, 16
    n = W * H
    without = frame.FrameRenderer(s, desc, W, H, spp=1)
    without.generate()
    without.render_specular(depth=1, lights=desc["lights"])
    fr = frame.FrameRenderer(s, desc, W, H, spp=1, square_lights=[FLOWER_SQUARE], square_samples=4)
    fr.generate()
    per_level = fr.render_specular(depth=1, lights=desc["lights"])
    torch.cuda.synchronize()
    got, base = fr.d_rgb.cpu().numpy().copy(), without.d_rgb.cpu().numpy().copy()
    f32 = dict(dtype=torch.float32, device="cuda")
    rgb = torch.zeros((n, 3), **f32)
    rays, weights, pixels, m = fr.d_rays, None, None, n
    by_hand = []
    for level in range(2):
        if m == 0:
            break
        fl = binding.MR_TRACE_INCOHERENT if level > 0 else 0
        hits, color, normal = torch.empty((m, 4), **f32), torch.empty((m, 3), **f32), torch.empty((m, 3), **f32)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        s.trace_device(rays, m, hits, fl)
        s.hit_surface(rays, hits, m, color, normal)
        s.shade_lights_surface(rays, hits, color, normal, m, rgb, d_weights=weights, d_pixels=pixels, spp=1, flags=fl, d_counts=cnt)
        s.shade_square_lights_surface([FLOWER_SQUARE], 4, rays, hits, color, normal, m, rgb, seed=fr.seed + level, d_weights=weights,
                                      d_pixels=pixels, spp=1, flags=fl, d_counts=cnt)
        by_hand.append((m, int(cnt.item())))
        if level == 1:
            break
        out_rays, out_w = torch.empty((3 * m, 8), **f32), torch.empty((3 * m, 3), **f32)
        out_pix, cnt2 = torch.empty(3 * m, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        s.gen_secondary_rays(rays, hits, weights, pixels, m, out_rays, out_w, out_pix, cnt2, spp=1)
        m = int(cnt2.item())
        rays, weights, pixels = out_rays[:m], out_w[:m], out_pix[:m]
    torch.cuda.synchronize()
    want = rgb.cpu().numpy()
    print("flower with a square light: rays and shadow rays per level %s; brightest pixel %.4g, without the square light %.4g; "
          "%d of %d pixels differ" % (per_level, got.max(), base.max(), (got != base).any(axis=1).sum(), n))
    assert per_level == by_hand and per_level[0][0] == n and per_level[0][1] % 5 == 0         # 1 disc + 4 square shadow rays per hit
    assert np.isfinite(got).all() and got.tobytes() == want.tobytes()
    assert (got != base).any(axis=1).sum() > n // 20 and (got >= base).all()


def checker_room():
    """photon_room with a checker on its floor plane and another on the wall z = -2 (the one with texture coordinates); no
    procedural texture, so only the square light needs the surface pass."""
    from miro_amd import scenes
    d = scenes.photon_room_mixed()
    d["textures"] = [dict(color1=(0.9, 0.2, 0.1), color2=(0.1, 0.2, 0.9), scale=1.0), dict(color1=(0.9, 0.8, 0.7), color2=(0.3, 0.35, 0.4), scale=2.0)]
    d["material_texture"] = [NONE, NONE, NONE, 0, NONE, 1, NONE, NONE]
    return d


@pytest.mark.gpu
def test_checker_room_renders_with_a_square_light(miro):
    """A scene whose texture table holds checkers only: mr_shade_square_lights still refuses it (MR_ERR_STATE), and
    FrameRenderer(square_lights=...) renders it -- the level's other calls stay the textured ones, mr_hit_surface runs for the
    square light alone -- where render_specular used to end in that MR_ERR_STATE."""
    import torch
    from miro_amd import binding, frame, scenes
    s = miro.Scene(0)
    desc = scenes.textured_room_setup(s, checker_room())
    assert s.n_textures == 2 and not s.procedural
    sq = dict(position=(0.0, 3.3, 0.0), normal=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0), wattage=200.0, dimensions=(1.0, 1.0))
    W, H = 24, 16
    without = frame.FrameRenderer(s, desc, W, H, spp=1)
    without.generate()
    without.render_specular(depth=1)
    fr = frame.FrameRenderer(s, desc, W, H, spp=1, square_lights=[sq], square_samples=4)
    fr.generate()
    calls = []
    for name in ("hit_surface", "shade_square_lights_surface", "shade_square_lights", "shade_accumulate", "shade_accumulate_surface"):
        setattr(s, name, (lambda f, name: lambda *a, **k: (calls.append(name), f(*a, **k))[1])(getattr(s, name), name))
    per_level = fr.render_specular(depth=1)
    torch.cuda.synchronize()
    got, base = fr.d_rgb.cpu().numpy(), without.d_rgb.cpu().numpy()
    print("checker room: rays and shadow rays per level %s, calls %s, brightest pixel %.4g (%.4g without the square light)" % (
        per_level, calls, got.max(), base.max()))
    assert len(per_level) >= 1 and calls == ["hit_surface", "shade_accumulate", "shade_square_lights_surface"] * len(per_level)
    assert np.isfinite(got).all() and (got != base).any(axis=1).sum() > W * H // 4
    with pytest.raises(miro.MiroError) as e:
        s.shade_square_lights([sq], 4, fr.d_rays, fr.d_hits, fr.n, fr.d_rgb)
    assert e.value.status == binding.MR_ERR_STATE


@pytest.mark.gpu
def test_untextured_teapot_keeps_the_plain_call(miro):
    """No texture table: FrameRenderer(square_lights=...) still calls mr_shade_square_lights, adds no mr_hit_surface launch, and
    the frame equals, byte for byte, one assembled by hand from the batched calls."""
    import torch
    from miro_amd import frame, scenes
    desc = scenes.SCENES["teapot"]
    s = miro.Scene(0)
    scenes.populate(s, desc)
    s.build(4)
    W = H = 24
    sq = dict(position=(0.0, 8.0, 0.0), normal=(0.0, -1.0, 0.0), wattage=300.0, dimensions=(2.0, 2.0))
    fr = frame.FrameRenderer(s, desc, W, H, spp=2, square_lights=[sq], square_samples=4)
    fr.generate()
    calls = []
    for name in ("hit_surface", "shade_square_lights_surface", "shade_square_lights"):
        setattr(s, name, (lambda f, name: lambda *a, **k: (calls.append(name), f(*a, **k))[1])(getattr(s, name), name))
    fr.render_specular(depth=0)
    torch.cuda.synchronize()
    got = fr.d_rgb.cpu().numpy().copy()
    assert calls == ["shade_square_lights"]
    n = fr.n
    f32 = dict(dtype=torch.float32, device="cuda")
    hits, sh_rays, sh_hits = torch.empty((n, 4), **f32), torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
    src, cnt = torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    rgb = torch.zeros((W * H, 3), **f32)
    s.trace_device(fr.d_rays, n, hits)
    s.gen_shadow_rays(fr.d_rays, hits, n, desc["light"], sh_rays, src, cnt)
    s.trace_indirect(sh_rays, cnt, n, sh_hits)
    s.shade_accumulate(fr.d_rays, hits, None, None, n, sh_rays, sh_hits, src, cnt, desc["light"], desc["wattage"], rgb, spp=2)
    s.shade_square_lights([sq], 4, fr.d_rays, hits, n, rgb, seed=fr.seed, spp=2, d_counts=cnt)
    torch.cuda.synchronize()
    want = rgb.cpu().numpy()
    assert want.max() > 0 and got.tobytes() == want.tobytes()
