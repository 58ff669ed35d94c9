"""mr_scene_set_lights / mr_shade_lights -- Phong::shade (Phong.cpp:44-160) over the scene's light list, point lights
(PointLight.h) and disc lights (DirectionalAreaLight.h), in one launch (csrc/mr_lights.hip).

The checker for the disc light is a restatement of Phong.cpp:78-156 written here in numpy float32, one operation per
rounding.  It uses the oracle only for what the oracle is already tested for (Scene.trace for the shadow hits, hit_attrs for
P / N) and imports nothing from the product; scene descriptions (data) come from miro_amd.scenes.  PARITY UNPINNED: the
checker is a restatement written from the cited lines of the reference.

The point light is checked against the product's own batched chain (mr_gen_shadow_rays -> mr_trace_indirect ->
mr_shade_accumulate), which tests/test_specular.py holds to the oracle: one point light must give the chain's bits."""
import ctypes as C
import os
import re
import sys
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402
F = np.float32
EPS = F(1e-4)                                                   # Miro.h:9
PI = F(3.1415926535897932384626433832795028841972)              # Miro.h:10
MISS, PLANE_BIT = 0xFFFFFFFF, 0x80000000
RTOL, ATOL_OF_MAX = 1e-5, 1e-7                                  # the project's tolerance for shaded values (test_specular.py:133)


# ---- the restatement -----------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalised(N):                                              # Scene.cpp:262
    with np.errstate(divide="ignore", invalid="ignore"):                        # a zero-length N: 0 * inf = NaN, as in the reference
        return (N * (F(1) / np.sqrt(dot3(N, N)))[:, None]).astype(F)


def std_max(a, b):
    """std::max(a, b) = (a < b) ? b : a.  A NaN b gives a, where np.maximum gives NaN: Phong.cpp:146-154 call it with the literal
    first, so a NaN normal (a zero-length HitInfo::N, normalised) leaves a diffuse term of 0 and a clamped e.r of 1"""
    with np.errstate(invalid="ignore"):
        return np.where(a < b, b, a).astype(F)


def std_min(a, b):
    """std::min(a, b) = (b < a) ? b : a"""
    with np.errstate(invalid="ignore"):
        return np.where(b < a, b, a).astype(F)


def rays_of(po, o, d, tmax):
    r = np.zeros(len(o), po.RAY_DTYPE)
    r["ox"], r["oy"], r["oz"], r["tmin"] = o[:, 0], o[:, 1], o[:, 2], 0.0
    r["dx"], r["dy"], r["dz"], r["tmax"] = d[:, 0], d[:, 1], d[:, 2], tmax
    return r


class Room:
    """An oracle scene of a description with its material table (11 floats per material, as the Phong constructor leaves them)."""

    def __init__(self, po, desc):
        from miro_amd import scenes
        self.po, self.scene = po, po.Scene()
        scenes.populate(self.scene, desc)
        self.scene.build(4)
        self.mats = np.array([list(kd) + list(ks) + list(kt) + [sh, ri] for kd, ks, kt, sh, ri in desc["materials"]], F)
        self.prim_mat = np.asarray(desc["prim_material"], np.uint32)
        self.plane_mat = np.asarray([o[3] if len(o) > 3 else 0 for o in desc["objects"] if o[0] == "plane"], np.uint32)

    def material_of(self, prim):
        is_plane = (prim & np.uint32(PLANE_BIT)) != 0
        plane_id = self.plane_mat[np.where(is_plane, prim & np.uint32(0x7FFFFFFF), 0)] if len(self.plane_mat) else np.zeros(len(prim), np.uint32)
        return self.mats[np.where(is_plane, plane_id, self.prim_mat[np.where(is_plane, 0, prim)])]


def restate_shade(room, rays, hits, light):
    """Phong::shade's loop body (Phong.cpp:78-156) for ONE light and every ray: returns (L [n,3] float32, info).  light: dict
    with position, color, wattage and -- a DirectionalAreaLight -- normal, radius.  info: per-ray masks of the branches taken
    and `fragile`, the rays whose branch a last-bit difference could flip."""
    po, n = room.po, len(rays)
    L = np.zeros((n, 3), F)
    info = dict(lit_inside=np.zeros(n, bool), outside=np.zeros(n, bool), opaque=np.zeros(n, bool), refractive=np.zeros(n, bool),
                fragile=np.zeros(n, bool), shadow_rays=0)
    idx = np.nonzero(hits["prim"] != MISS)[0]
    if len(idx) == 0:
        return L, info
    r, h = rays[idx], hits[idx]
    P, N = room.scene.hit_attrs(h, r)
    N = normalised(N)
    e = -np.stack([r["dx"], r["dy"], r["dz"]], 1).astype(F)                            # :49
    mt = room.material_of(h["prim"])
    color, watt = np.asarray(light.get("color", (1, 1, 1)), F), F(light["wattage"])
    disc = "normal" in light
    pos = np.asarray(light["position"], F)
    if disc:
        nrm = np.asarray(light["normal"], F)
        l = np.repeat((-nrm)[None, :], len(idx), axis=0).astype(F)                      # DirectionalAreaLight.h:25-29
    else:
        l = (pos[None, :] - P).astype(F)                                                # PointLight::getLightDirection
    falloff = dot3(l, l)                                                                # :85
    length = np.sqrt(falloff)
    l = (l * (F(1) / length)[:, None]).astype(F)                                        # :88 (Vector3::operator/=)
    # ---- the shadow ray (:92-113)
    sr = rays_of(po, (P + l * EPS).astype(F), l, length)
    sh = room.scene.trace(sr)
    info["shadow_rays"] = len(idx)
    intensity = np.ones(len(idx), F)
    skip = np.zeros(len(idx), bool)
    occ = np.nonzero(sh["prim"] != MISS)[0]
    if len(occ):
        om = room.material_of(sh["prim"][occ])
        refr = (om[:, 6] > 0) | (om[:, 7] > 0) | (om[:, 8] > 0)                        # Phong::isRefractive
        _, Ns = room.scene.hit_attrs(sh[occ], sr[occ])
        dn = dot3(normalised(Ns), l[occ])
        through = refr & ~(dn < 0) & ~(dn < EPS)
        intensity[occ[through]] = dn[through]
        skip[occ[~through]] = True
        info["opaque"][idx[occ[~refr]]] = True
        info["refractive"][idx[occ[refr]]] = True
        info["fragile"][idx[occ[refr & ((np.abs(dn) <= 1e-6) | (np.abs(dn - EPS) <= 1e-6))]]] = True
    # ---- the light's terms (:119-156)
    if disc:
        nDotL = dot3(N, np.repeat((-nrm)[None, :], len(idx), axis=0).astype(F))        # :128
        t = dot3(np.repeat(nrm[None, :], len(idx), axis=0), (pos[None, :] - P).astype(F)) / F(-1.0)      # :132
        q = ((P - t[:, None] * nrm[None, :]).astype(F) - pos[None, :]).astype(F)
        q2, r2 = dot3(q, q), F(light["radius"]) * F(light["radius"])
        out_of_disc = q2 > r2                                                           # :133
        info["fragile"][idx[np.abs(q2 - r2) <= F(1e-5) * r2]] = True
        info["outside"][idx[~skip & out_of_disc]] = True
        skip = skip | out_of_disc
        f2 = np.full(len(idx), F(1.0) / PI, F)                                          # :135
    else:
        nDotL = dot3(N, l)                                                              # :139
        f2 = F(1.0) / (falloff * F(4.0) * PI * PI)                                      # :140
    diff = std_max(F(0), nDotL * f2 * watt)
    out = color[None, :] * (diff[:, None] * mt[:, 0:3] * mt[:, 0:3]) * intensity[:, None]              # :146
    shiny = mt[:, 9] < np.inf                                                           # :149
    two = 2 * dot3(l, N)
    rv = (-l + two[:, None] * N).astype(F)                                              # :151
    edr = np.power(std_max(F(0), std_min(F(1), dot3(e, rv))), F(500)).astype(F)         # :152
    high = np.where(shiny, std_max(F(0), edr * f2 * watt), F(0)).astype(F)              # :154
    out = (out + high[:, None]).astype(F)
    out[skip] = 0
    L[idx] = out
    info["lit_inside"][idx[~skip & (out.max(axis=1) > 0)]] = disc
    return L, info


# a DirectionalAreaLight whose normal is neither of unit length nor axis-aligned: tMax = |normal| != 1 and the un-normalised
# nDotL are both exercised (photon_room's geometry)
TILTED = dict(position=(0.1, 3.9, -0.1), normal=(0.2, -1.05, 0.1), color=(1.0, 0.9, 0.8), wattage=80.0, radius=1.0)
W_DISC = 256


def disc_cases():
    from miro_amd import scenes
    return [("photon_room", scenes.SCENES["photon_room"]["lights"][0]), ("photon_room_diffuse", scenes.SCENES["photon_room_diffuse"]["lights"][0]),
            ("photon_room", TILTED)]


def primary(oracle, room, name, W, H, spp=1):
    from helpers import camera_of
    rays = oracle.eye_rays(camera_of(oracle, name), W, H, spp=spp, jitter=spp > 1, seed=168)
    return rays, room.scene.trace(rays)


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_the_light_list_entries_are_exported_and_declared(miro, tmp_path):
    from miro_amd import binding
    L = miro.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "miro_hip.h")).read(), flags=re.S)
    for name in ("mr_scene_set_lights", "mr_shade_lights"):
        assert hasattr(L, name) and name in miro.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, src), name
    assert binding.MR_LIGHT_POINT == 0 and binding.MR_LIGHT_DISC == 1 and binding.MR_MAX_LIGHTS == 8
    assert re.search(r"#define\s+MR_MAX_LIGHTS\s+8\b", src)
    # sizeof(mr_light_desc) as the C compiler sees the header = the ctypes structure
    prog = '#include "miro_hip.h"\n#include <stdio.h>\nint main(void) { printf("%d\\n", (int)sizeof(mr_light_desc)); return 0; }\n'
    exe = str(tmp_path / "sizeof_light_desc")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=prog.encode(), check=True)
    assert int(subprocess.check_output([exe])) == C.sizeof(binding.LightDesc) == 64


def test_light_list_argument_errors(miro):
    """Every invalid argument: MR_ERR_INVALID with a message, before any device call (a host_only scene); mr_shade_lights on
    such a scene: MR_ERR_STATE, never a CPU path."""
    from miro_amd import binding
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.build(4, host_only=True)

    def light(kind=binding.MR_LIGHT_DISC, **kw):
        ld = binding.LightDesc()
        ld.kind = kind
        ld.position[:] = kw.get("position", (0, 1, 0))
        ld.normal[:] = kw.get("normal", (0, -1, 0))
        ld.color[:] = kw.get("color", (1, 1, 1))
        ld.wattage, ld.radius = kw.get("wattage", 10.0), kw.get("radius", 0.5)
        ld.reserved[:] = kw.get("reserved", (0, 0, 0, 0))
        return ld

    def arr(*ls):
        a = (binding.LightDesc * len(ls))()
        for i, l in enumerate(ls):
            a[i] = l
        return a

    inf, nan = float("inf"), float("nan")
    ok = light()
    assert L.mr_scene_set_lights(None, arr(ok), 1) == -1 and b"NULL" in L.mr_last_error()
    assert L.mr_scene_set_lights(s.h, None, 1) == -1 and b"NULL" in L.mr_last_error()
    assert L.mr_scene_set_lights(s.h, arr(*[ok] * 9), 9) == -1 and b"at most" in L.mr_last_error()
    for bad, word in ((light(kind=2), b"kind"), (light(reserved=(0, 0, 1, 0)), b"reserved"), (light(position=(0, nan, 0)), b"finite"),
                      (light(color=(inf, 1, 1)), b"finite"), (light(wattage=nan), b"finite"), (light(radius=0.0), b"radius"),
                      (light(radius=-1.0), b"radius"), (light(radius=inf), b"radius"), (light(normal=(0, 0, 0)), b"normal"),
                      (light(normal=(0, nan, 0)), b"normal"), (light(kind=binding.MR_LIGHT_POINT, wattage=inf), b"finite")):
        assert L.mr_scene_set_lights(s.h, arr(ok, bad), 2) == -1, word
        assert word in L.mr_last_error(), (word, L.mr_last_error())
    dummy = C.c_void_p(16)
    # a refused list leaves the scene without lights; a scene without lights and a host_only scene: MR_ERR_STATE
    assert L.mr_shade_lights(s.h, dummy, dummy, None, None, 4, 1, 0, dummy, None, None, None) == -5
    assert L.mr_shade_lights(None, dummy, dummy, None, None, 4, 1, 0, dummy, None, None, None) == -1
    # a point light ignores normal and radius; the list is replaced and cleared
    assert L.mr_scene_set_lights(s.h, arr(ok, light(kind=binding.MR_LIGHT_POINT, radius=-1.0, normal=(0, 0, 0))), 2) == 0
    assert L.mr_shade_lights(s.h, dummy, dummy, None, None, 4, 1, 0, dummy, None, None, None) == -5
    assert b"CPU" in L.mr_last_error() or b"device" in L.mr_last_error()
    assert L.mr_scene_set_lights(s.h, None, 0) == 0
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0), dict(position=(0, 1, 0), normal=(0, -1, 0), wattage=5.0, radius=1.0)])
    t = miro.Scene()
    t.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    t.set_lights([dict(position=(0, 1, 0), wattage=5.0)])                                       # before the build
    assert L.mr_shade_lights(t.h, dummy, dummy, None, None, 4, 1, 0, dummy, None, None, None) == -5     # not built


def test_scene_table_carries_the_light_lists():
    from miro_amd import scenes
    for name in ("photon_room", "photon_room_diffuse"):
        d = scenes.SCENES[name]
        assert d["lights"] == [d["disc_light"]] and "light" in d and "wattage" in d
    two = scenes.SCENES["photon_room_two_lights"]
    assert two["lights"][0] == scenes.SCENES["photon_room"]["disc_light"]
    assert tuple(two["lights"][1]["position"]) == tuple(scenes.SCENES["photon_room"]["light"]) and "normal" not in two["lights"][1]
    assert two["objects"] == scenes.SCENES["photon_room"]["objects"]


def test_lights_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_lights.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer waves per
    SIMD than BOTH its own record (tests/golden/kernel_budget_lights.json, written from the build whose GPU tests were green)
    AND the worst value among the kernels of tests/golden/kernel_budget.json.  The unit's remarks live in
    build/mr_lights.remarks.txt, which test_build_budget.py does not read."""
    cur = kernel_budget.unit_kernels("mr_lights")
    assert len(cur) >= 6 and all("shade_lights_kernel" in k for k in cur)
    assert not any("trace_kernel" in k or "frame_kernel" in k for k in cur)
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_lights.json")


def test_restatement_leaves_few_rays_out_and_takes_every_branch(oracle):
    """With the oracle alone, at the resolution of the GPU comparison: the restatement's own fragile rays (disc test within
    1e-5 radius^2 of its threshold, a refractive occluder's dot(N, l) within 1e-6 of 0 / epsilon) are fewer than 0.1 % of any
    case, and over the set of cases every branch occurs: lit inside the cylinder, outside it, opaque- and refractive-occluded."""
    from miro_amd import scenes
    seen = dict(lit_inside=0, outside=0, opaque=0, refractive=0)
    for name, light in disc_cases():
        room = Room(oracle, scenes.SCENES[name])
        rays, hits = primary(oracle, room, name, W_DISC, W_DISC)
        L, info = restate_shade(room, rays, hits, light)
        print("%s |n|=%.3f: fragile %d of %d; %s" % (name, float(np.linalg.norm(light["normal"])), info["fragile"].sum(), len(rays),
                                                     {k: int(info[k].sum()) for k in seen}))
        assert info["fragile"].sum() <= 1e-3 * len(rays) and np.isfinite(L).all() and L.max() > 0
        for k in seen:
            seen[k] += int(info[k].sum())
    assert all(v > 0 for v in seen.values()), seen


def test_restatement_of_a_point_light_is_the_oracles_recursion_at_depth_0(oracle):
    """The restatement against something that is not itself: for a point light, Scene::traceScene at depth 0 is exactly
    Phong::shade of the primary hit (the oracle's restated recursion, which the specular tests pin)."""
    from miro_amd import scenes
    d = scenes.SCENES["photon_room"]
    room = Room(oracle, d)
    rays, hits = primary(oracle, room, "photon_room", 96, 96)
    L, _ = restate_shade(room, rays, hits, dict(position=d["light"], color=(1, 1, 1), wattage=d["wattage"]))
    want, _ = room.scene.trace_scene(room.mats, room.prim_mat, rays, d["light"], d["wattage"], depth=0)
    assert want.max() > 0 and np.allclose(L, want, rtol=RTOL, atol=ATOL_OF_MAX * float(want.max()))


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
def product_scene_of(miro, name):
    from miro_amd import scenes
    desc = scenes.SCENES[name]
    s = miro.Scene(0)
    scenes.populate(s, desc)
    if "materials" in desc:
        s.set_materials(desc["materials"], desc["prim_material"])
    s.build(4)
    return s, desc


class Traced:
    """Primary rays of a description, generated and traced by the product, resident on the device."""

    def __init__(self, miro, scene, desc, W, H, spp=1, flags=0):
        import torch
        from miro_amd import binding
        self.n = W * H * spp
        self.rays = torch.empty((self.n, 8), dtype=torch.float32, device="cuda")
        self.hits = torch.empty((self.n, 4), dtype=torch.float32, device="cuda")
        cam = binding.make_camera(desc["eye"], desc["lookat"], desc["up"], desc["fov"])
        scene.gen_eye_rays(cam, W, H, self.rays, spp=spp, jitter=spp > 1, seed=168)
        scene.trace_device(self.rays, self.n, self.hits, flags)


def chain(scene, rays, hits, n, light_pos, wattage, flags, n_pixels, weights=None, pixels=None, spp=1, color=(1.0, 1.0, 1.0)):
    """The batched shadow chain for one point light: (d_rgb, shadow rays traced)"""
    import torch
    sh_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    sh_hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rgb = torch.zeros((n_pixels, 3), dtype=torch.float32, device="cuda")
    scene.gen_shadow_rays(rays, hits, n, light_pos, sh_rays, src, cnt)
    scene.trace_indirect(sh_rays, cnt, n, sh_hits, flags)
    scene.shade_accumulate(rays, hits, weights, pixels, n, sh_rays, sh_hits, src, cnt, light_pos, wattage, rgb, spp=spp, color=color)
    torch.cuda.synchronize()
    return rgb, int(cnt.item())


def shade_lights(scene, rays, hits, n, lights, n_pixels=None, flags=0, weights=None, pixels=None, spp=1):
    """(d_rgb, d_ray_rgb, shadow rays traced) of mr_shade_lights, as numpy arrays"""
    import torch
    scene.set_lights(lights)
    n_pixels = n // spp if n_pixels is None else n_pixels
    rgb = torch.zeros((n_pixels, 3), dtype=torch.float32, device="cuda")
    ray_rgb = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device="cuda")                 # one sentinel row after the end
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    scene.shade_lights(rays, hits, n, rgb, d_weights=weights, d_pixels=pixels, spp=spp, flags=flags, d_ray_rgb=ray_rgb, d_counts=cnt)
    torch.cuda.synchronize()
    out = ray_rgb.cpu().numpy()
    assert (out[n] == -7.0).all(), "d_ray_rgb was written beyond 3n floats"
    return rgb.cpu().numpy(), out[:n].copy(), int(cnt.item())


@pytest.mark.gpu
@pytest.mark.parametrize("name,W,H", [("photon_room", 192, 160), ("bunny", 256, 192)])
def test_one_point_light_is_the_chain_bit_for_bit(miro, name, W, H):
    """Primary rays at 1 spp in image order, d_pixels NULL, d_rgb zeroed: every pixel receives exactly one addition on both
    sides, so the order of the atomics cannot enter -- d_rgb of mr_shade_lights with one point light equals, as uint32, d_rgb of
    mr_gen_shadow_rays -> mr_trace_indirect -> mr_shade_accumulate; with MR_MATH_PRODUCT on both sides too; same shadow count."""
    from miro_amd import binding
    scene, desc = product_scene_of(miro, name)
    light = dict(position=desc["light"], color=(1.0, 0.9, 0.7), wattage=desc["wattage"])
    for flags in (0, binding.MR_MATH_PRODUCT):
        tr = Traced(miro, scene, desc, W, H, flags=flags)
        want, n_shadow = chain(scene, tr.rays, tr.hits, tr.n, desc["light"], desc["wattage"], flags, W * H, color=light["color"])
        got, per_ray, counted = shade_lights(scene, tr.rays, tr.hits, tr.n, [light], flags=flags)
        want = want.cpu().numpy()
        print("%s flags=%d: %d shadow rays, max %.4g" % (name, flags, n_shadow, want.max()))
        assert want.max() > 0 and 0 < n_shadow == counted
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(per_ray, got)                                    # weight 1, spp 1: the pixel IS the ray's L
    if desc.get("materials"):                                                  # the glass sphere: any-hit shadow rays are refused
        with pytest.raises(miro.MiroError) as e:
            shade_lights(scene, tr.rays, tr.hits, tr.n, [light], flags=binding.MR_TRACE_ANY)
        assert e.value.status == binding.MR_ERR_STATE
    else:                                                                      # opaque occluders only: any hit scales the light to 0
        any_rgb, _, _ = shade_lights(scene, tr.rays, tr.hits, tr.n, [light], flags=binding.MR_MATH_PRODUCT | binding.MR_TRACE_ANY)
        assert np.array_equal(any_rgb.view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
def test_lights_add_in_list_order(miro):
    """[A, B] gives fl32(LA + LB) of the two single-light results, [B, A] the same bits, [A, B, C] fl32(fl32(LA + LB) + LC)."""
    scene, desc = product_scene_of(miro, "photon_room")
    tr = Traced(miro, scene, desc, 160, 128)
    A = dict(position=desc["light"], color=(1.0, 1.0, 1.0), wattage=desc["wattage"])
    B = dict(position=(1.2, 2.5, 1.0), color=(0.2, 0.9, 0.4), wattage=37.0)
    Cc = dict(position=(-1.5, 0.4, 1.5), color=(0.9, 0.3, 0.1), wattage=211.0)
    single = {k: shade_lights(scene, tr.rays, tr.hits, tr.n, [lt])[1] for k, lt in (("A", A), ("B", B), ("C", Cc))}
    assert all(v.max() > 0 for v in single.values())
    ab = shade_lights(scene, tr.rays, tr.hits, tr.n, [A, B])
    ba = shade_lights(scene, tr.rays, tr.hits, tr.n, [B, A])
    abc = shade_lights(scene, tr.rays, tr.hits, tr.n, [A, B, Cc])
    cba = shade_lights(scene, tr.rays, tr.hits, tr.n, [Cc, B, A])
    hits = int((tr.hits[:, 1].view(__import__("torch").int32) != -1).sum().item())
    assert ab[2] == ba[2] == 2 * hits and abc[2] == 3 * hits
    assert np.array_equal(ab[1], (single["A"] + single["B"]).astype(F))
    assert np.array_equal(ba[1], (single["B"] + single["A"]).astype(F))
    assert np.array_equal(abc[1], ((single["A"] + single["B"]).astype(F) + single["C"]).astype(F))
    assert np.array_equal(cba[1], ((single["C"] + single["B"]).astype(F) + single["A"]).astype(F))
    assert not np.array_equal(abc[1], cba[1])                                  # the order is visible in the last bits


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 2], ids=["room", "diffuse-room", "tilted-normal"])
def test_disc_light_matches_the_restatement(oracle, miro, case):
    """d_ray_rgb of a disc light against the restatement of Phong.cpp:78-156, rtol 1e-5, atol 1e-7 x max (powf on the device vs
    pow in the checker is what needs it).  Rays left out: only the restatement's own fragile ones, at most 0.1 % of the case."""
    from miro_amd import scenes
    name, light = disc_cases()[case]
    room = Room(oracle, scenes.SCENES[name])
    rays, hits = primary(oracle, room, name, W_DISC, W_DISC)
    want, info = restate_shade(room, rays, hits, light)
    scene, desc = product_scene_of(miro, name)
    tr = Traced(miro, scene, desc, W_DISC, W_DISC)
    assert tr.rays.cpu().numpy().tobytes() == rays.tobytes() and tr.hits.cpu().numpy().tobytes() == hits.tobytes()
    _, got, counted = shade_lights(scene, tr.rays, tr.hits, tr.n, [light])
    keep = ~info["fragile"]
    scale = float(want.max())
    err = np.abs(got[keep].astype(np.float64) - want[keep]) - RTOL * np.abs(want[keep])
    print("%s: %d of %d rays left out, scale %.4g, worst excess over rtol %.3g (atol %.3g); branches %s" % (
        name, (~keep).sum(), len(rays), scale, err.max(), ATOL_OF_MAX * scale,
        {k: int(info[k].sum()) for k in ("lit_inside", "outside", "opaque", "refractive")}))
    assert (~keep).sum() <= 1e-3 * len(rays) and scale > 0
    assert counted == info["shadow_rays"]
    assert np.allclose(got[keep], want[keep], rtol=RTOL, atol=ATOL_OF_MAX * scale)
    assert (got[hits["prim"] == MISS] == 0).all()
    if case == 0:
        assert info["lit_inside"].any() and info["outside"].any() and info["opaque"].any() and info["refractive"].any()


@pytest.mark.gpu
def test_weights_pixels_and_spp_of_a_bounce_queue(miro):
    """The children of mr_gen_secondary_rays on photon_room (their weights and pixels) shaded by [disc, point]: d_rgb against
    sum(weight * d_ray_rgb / spp) scattered on the host in float64."""
    import torch
    scene, desc = product_scene_of(miro, "photon_room")
    W, H, spp = 128, 96, 2
    tr = Traced(miro, scene, desc, W, H, spp=spp)
    n = tr.n
    kids = torch.empty((3 * n, 8), dtype=torch.float32, device="cuda")
    kw = torch.empty((3 * n, 3), dtype=torch.float32, device="cuda")
    kp = torch.empty(3 * n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    scene.gen_secondary_rays(tr.rays, tr.hits, None, None, n, kids, kw, kp, cnt, spp=spp)
    m = int(cnt.item())
    assert 1000 < m <= 3 * n
    kids, kw, kp = kids[:m].contiguous(), kw[:m].contiguous(), kp[:m].contiguous()
    khits = torch.empty((m, 4), dtype=torch.float32, device="cuda")
    scene.trace_device(kids, m, khits, miro.MR_TRACE_INCOHERENT)
    from miro_amd import scenes
    lights = scenes.SCENES["photon_room_two_lights"]["lights"]
    rgb, per_ray, counted = shade_lights(scene, kids, khits, m, lights, n_pixels=W * H, flags=miro.MR_TRACE_INCOHERENT, weights=kw, pixels=kp, spp=spp)
    want = np.zeros((W * H, 3), np.float64)
    np.add.at(want, kp.cpu().numpy().astype(np.int64), kw.cpu().numpy().astype(np.float64) * per_ray.astype(np.float64) / spp)
    n_hits = int((khits[:, 1].view(torch.int32) != -1).sum().item())
    print("%d children, %d hits, max %.4g, worst error %.3g" % (m, n_hits, want.max(), np.abs(rgb - want).max()))
    assert counted == 2 * n_hits and want.max() > 0
    assert np.allclose(rgb, want, rtol=RTOL, atol=ATOL_OF_MAX * float(want.max()))
    # both lights are in it: the sum differs from either light alone
    only_disc = shade_lights(scene, kids, khits, m, lights[:1], n_pixels=W * H, weights=kw, pixels=kp, spp=spp)[1]
    assert only_disc.max() > 0 and (per_ray >= only_disc).all() and (per_ray > only_disc).any()


@pytest.mark.gpu
def test_render_specular_over_a_light_list(miro):
    """The driver: with the description's point light as a one-entry list, every level is trace -> mr_shade_lights -> generators
    and the frame equals render_specular's own (two orders of the same atomics, test_specular.py:175) with the same ray counts
    per level; with the room's disc light the floor under the light is lit, everything outside the disc's cylinder is black
    before the photon term, and final_gather from a map traced from the same light adds the indirect light."""
    import torch
    from miro_amd import frame, scenes
    scene, desc = product_scene_of(miro, "photon_room")
    W, H = 160, 128
    fr = frame.FrameRenderer(scene, desc, W, H)
    fr.generate()
    levels = fr.render_specular(depth=3)
    torch.cuda.synchronize()
    ref = fr.d_rgb.clone()
    point = dict(position=desc["light"], color=(1.0, 1.0, 1.0), wattage=desc["wattage"])
    levels2 = fr.render_specular(depth=3, lights=[point])
    torch.cuda.synchronize()
    print("levels", levels, "max", float(ref.max()), "worst difference", float((fr.d_rgb - ref).abs().max()))
    assert levels2 == levels and len(levels) == 4 and levels[1][0] > 0
    assert torch.allclose(fr.d_rgb, ref, rtol=1e-6, atol=1e-7 * float(ref.max()))
    with pytest.raises(ValueError):
        fr.render_specular(depth=3, lights=[point], fused=True)
    # ---- the disc light: direct light, then the photon term
    fr.render_specular(depth=0, lights=desc["lights"])
    torch.cuda.synchronize()
    direct = fr.d_rgb.cpu().numpy().copy()
    P = torch.empty((fr.n, 3), dtype=torch.float32, device="cuda")
    scene.hit_attrs(fr.d_hits, fr.n, P, None, d_rays=fr.d_rays)
    P = P.cpu().numpy().astype(np.float64)
    prim = fr.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    disc = desc["disc_light"]
    r2 = (P[:, 0] - disc["position"][0]) ** 2 + (P[:, 2] - disc["position"][2]) ** 2
    floor = (prim & PLANE_BIT) != 0
    clear = np.ones(len(P), bool)
    for o in desc["objects"]:
        if o[0] == "sphere":                            # not under a sphere (the shadow ray looks one unit up)
            clear &= (P[:, 0] - o[1][0]) ** 2 + (P[:, 2] - o[1][2]) ** 2 > (o[2] + 0.05) ** 2
    lit = floor & clear & (r2 < 0.9 * disc["radius"] ** 2)
    outside = (prim != MISS) & (r2 > 1.1 * disc["radius"] ** 2)
    assert lit.sum() > 50 and outside.sum() > 1000
    assert (direct[lit].min(axis=1) > 0).all() and (direct[outside] == 0).all()
    pm = miro.PhotonMap(40000)
    res = scene.trace_photons(pm, disc, 20000, 400000)
    assert res["stored"] >= 20000
    pm.balance()
    fr.final_gather(pm, None, nphotons=50, max_dist=0.5)
    torch.cuda.synchronize()
    total = fr.d_rgb.cpu().numpy()
    assert np.isfinite(total).all() and (total >= direct).all() and (total[outside].max(axis=1) > 0).mean() > 0.25


@pytest.mark.gpu
def test_shade_lights_replays_from_a_captured_graph(miro):
    """One call captured on a stream (torch.cuda.graph) and replayed twice gives the first call's d_ray_rgb: the call only
    enqueues."""
    import torch
    from miro_amd import scenes
    scene, desc = product_scene_of(miro, "photon_room")
    tr = Traced(miro, scene, desc, 128, 96)
    scene.set_lights(scenes.SCENES["photon_room_two_lights"]["lights"])
    first = torch.zeros((tr.n, 3), dtype=torch.float32, device="cuda")
    scene.shade_lights(tr.rays, tr.hits, tr.n, None, d_ray_rgb=first)
    torch.cuda.synchronize()
    assert float(first.max()) > 0
    out = torch.zeros((tr.n, 3), dtype=torch.float32, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scene.shade_lights(tr.rays, tr.hits, tr.n, None, d_ray_rgb=out, stream=side)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        scene.shade_lights(tr.rays, tr.hits, tr.n, None, d_ray_rgb=out, stream=torch.cuda.current_stream())
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)
