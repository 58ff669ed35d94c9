"""Textured Phong materials: UV coordinates of a hit (csrc/mr_uv.h), checker and image textures (csrc/mr_texture.h), the
textured forms of mr_shade_lights / mr_shade_accumulate (csrc/mr_textures.hip) and the OBJ loader's texture coordinates.

The oracle has no textures.  Expected values are float32 numpy restatements of the reference's lines, written here and
importing nothing from the product's lookup code: Plane.cpp:50-60, Sphere.cpp:83-95, Triangle.cpp:172-222, Texture.h:112-133,
Texture.cpp:23-28,161-185, TriangleMeshLoad.cpp:81-111,154-158,198-250.  The hit point P comes from mr_hit_attrs, which
tests/test_objects.py and tests/test_gpu_parity.py hold to the oracle.  The shading tests lean on the UNTEXTURED kernels of the
same calls (tests/test_lights.py ties them to the oracle): with A = the untextured result for Phong(kd = 1, ks, kt) and B the one
for kd = 0 (the highlights alone), the textured result is (A - B) * tex / m + B per ray and channel, m = clamp(1 - ks - kt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_budget  # noqa: E402

F = np.float32
PI = F(3.1415926535897932384626433832795028841972)
MISS = 0xFFFFFFFF
PLANE_BIT = 0x80000000
NONE = 0xFFFFFFFF
N_RAYS = 3 * 256 + 37                    # three whole workgroups and a partial one


# ---------------------------------------------------------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------------------------------------------------------
def std_max(a, b):
    """std::max(a, b) = a < b ? b : a (a NaN first argument stays)"""
    return np.where(a < b, b, a).astype(F)


def std_min(a, b):
    """std::min(a, b) = b < a ? b : a"""
    return np.where(b < a, b, a).astype(F)


def uv_plane(P):
    return np.stack([P[:, 0], P[:, 2]], axis=1).astype(F)


def uv_sphere(P, centre):
    """Sphere.cpp:83-95; atan2 / asin: the double functions rounded to float (what tests/test_environment.py shows mm_atan2f /
    mm_asinf to be), `+ 0.5` in double."""
    d = (P - np.asarray(centre, F)).astype(F)
    inv = F(1) / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = (d * inv[:, None]).astype(F)
    at = np.arctan2(d[:, 0].astype(np.float64), d[:, 2].astype(np.float64)).astype(F)
    u = ((at / (F(2) * PI)).astype(np.float64) + 0.5).astype(F)
    with np.errstate(invalid="ignore"):
        a = np.arcsin(d[:, 1].astype(np.float64)).astype(F)
    a = std_max(np.full_like(a, -1), std_min(np.full_like(a, 1), a))
    v = ((a / PI).astype(np.float64) + 0.5).astype(F)
    return np.stack([u, v], axis=1)


def uv_triangle(P, A, B, C, tA, tB, tC):
    """Triangle.cpp:186-222 for arrays of hits: A, B, C the triangle's vertices and tA, tB, tC its texture coordinates, per hit"""
    P, A, B, C = (np.asarray(x, F) for x in (P, A, B, C))
    BmA, CmA = (B - A).astype(F), (C - A).astype(F)
    nx = BmA[:, 1] * CmA[:, 2] - BmA[:, 2] * CmA[:, 1]
    ny = BmA[:, 2] * CmA[:, 0] - BmA[:, 0] * CmA[:, 2]
    nz = BmA[:, 0] * CmA[:, 1] - BmA[:, 1] * CmA[:, 0]
    i = np.where(nx > nz, 2, 0)
    j = np.where(nx > nz, 1, np.where(ny > nz, 2, 1))
    p = (P - A).astype(F)
    r = np.arange(len(P))
    det = lambda a, b, c, d: (a * d - b * c).astype(F)                                       # noqa: E731  (Triangle.cpp:16)
    detPC = det(p[r, i], CmA[r, i], p[r, j], CmA[r, j])
    detBP = det(BmA[r, i], p[r, i], BmA[r, j], p[r, j])
    detBC = det(BmA[r, i], CmA[r, i], BmA[r, j], CmA[r, j])
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = std_max((detPC / detBC).astype(F), F(0))
        gamma = std_max((detBP / detBC).astype(F), F(0))
    alpha = std_max((F(1) - (beta + gamma)).astype(F), F(0))
    uv = (alpha[:, None] * tA + beta[:, None] * tB).astype(F) + (gamma[:, None] * tC).astype(F)
    return uv.astype(F), (i, j)


def checker(uv, color1, color2, scale):
    """Texture.h:125-132 (non-negative scale: the C and numpy remainders agree)"""
    uv = np.asarray(uv, F)
    s = F(scale)
    a, b = np.abs(s * uv[:, 0]).astype(F), np.abs(s * uv[:, 1]).astype(F)
    a = np.where(uv[:, 0] < 0, a + s, a).astype(F)
    b = np.where(uv[:, 1] < 0, b + s, b).astype(F)
    even = (a.astype(np.int32) + b.astype(np.int32)) % 2 == 0
    return np.where(even[:, None], np.asarray(color1, F), np.asarray(color2, F)).astype(F)


def image_lookup(uv, img, hdr):
    """Texture.cpp:161-185 on an image [H, W, 3] (row 0 = bottom scanline); returns (rgb, inside) -- inside: the reference's
    own arithmetic stays in the image"""
    img = np.asarray(img, F)
    h, w = img.shape[:2]
    uv = np.asarray(uv, F)

    def axis(n, c):
        p = (F(n) * c).astype(F)
        ok = np.abs(p) < 2147483520.0
        i1 = np.where(ok, p, 0).astype(np.int32)                                              # (int) truncates
        i2 = i1 + 1
        i1w, i2w = np.fmod(i1, n), np.fmod(i2, n)                                              # C's %
        err = (p - i1w.astype(F)).astype(F)
        return i1w, i2w, err, ok & (i1w >= 0) & (i2w >= 0)

    x1, x2, xe, okx = axis(w, uv[:, 0])
    y1, y2, ye, oky = axis(h, uv[:, 1])
    ok = okx & oky
    x1, x2, y1, y2 = (np.where(ok, a, 0) for a in (x1, x2, y1, y2))
    xe, ye = xe[:, None], ye[:, None]
    f = ((img[y1, x1] * (1 - xe) + img[y1, x2] * xe) * (1 - ye) + (img[y2, x1] * (1 - xe) + img[y2, x2] * xe) * ye).astype(F)
    if hdr:
        mx = F(-1e15)
        mx = max(mx, img.max())
        with np.errstate(invalid="ignore"):
            a = (np.power((f / mx).astype(np.float64), 0.5).astype(F) * F(1.5)).astype(F)
        f = np.where(F(1) < a, F(1), a).astype(F)
    f[~ok] = 0
    return f, ok


def restated_obj_texcoords(path):
    """TriangleMeshLoad.cpp:81-111,154-158,198-250 for the texture side: (texcoords [n, 2], indices [faces, 3]); a corner
    without a texture index in a file that has vt records is index 0 (the reference leaves it uninitialised)."""
    t, ti = [], []
    for line in open(path):
        line = line[:79]
        if line.startswith("vt"):
            x, y = line[2:].split()[:2]
            t.append((F(x), F(y)))
        elif line.startswith("f"):
            row = []
            for word in line[1:].split()[:3]:
                parts = word.split("/")
                k = int(parts[1]) if len(parts) > 1 and parts[1] else 0
                row.append(k - 1 if k else 0)
            ti.append(row)
    if not t:
        return np.zeros((0, 2), F), np.full((len(ti), 3), NONE, np.uint32)
    return np.asarray(t, F), np.asarray(ti, np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: restatement self-checks, setters, loader
# ---------------------------------------------------------------------------------------------------------------------------
def test_checker_restatement_on_a_hand_worked_grid():
    """Unit squares alternate from (0, 0) = color1; a negative u is folded by |u| + scale, so [-1, 0) x [0, 1) -- |u| in (0, 1]
    plus 1 -> 1 -- is color2 and mirrors the square right of the axis shifted by one."""
    c1, c2 = (1, 0, 0), (0, 0, 1)
    pts = np.array([[0.5, 0.5], [1.5, 0.5], [1.5, 1.5], [0.5, 2.5], [-0.5, 0.5], [-1.5, 0.5], [-0.5, -0.5], [2.25, 0.25]], F)
    want = [c1, c2, c1, c1, c2, c1, c1, c1]
    assert np.array_equal(checker(pts, c1, c2, 1), np.array(want, F))
    # scale 10: squares of 0.1; (0.25, 0.05) -> (int)2.5 + (int)0.5 = 2 -> color1; (0.35, 0.05) -> 3 -> color2
    assert np.array_equal(checker(np.array([[0.25, 0.05], [0.35, 0.05]], F), c1, c2, 10), np.array([c1, c2], F))
    # scale 0.5: squares of 2
    assert np.array_equal(checker(np.array([[1.5, 0.5], [2.5, 0.5], [-0.5, 0.5]], F), c1, c2, 0.5), np.array([c1, c2, c1], F))


def test_sphere_restatement_clamps_the_angle_not_v():
    """asin(dir.y) is clamped to +-1 RADIAN: the poles give v = 0.5 +- 1 / PI, not 0 and 1."""
    c = np.zeros(3, F)
    P = np.array([[0, 1, 0], [0, -1, 0], [0, 0, 1], [1, 0, 0], [0, 0.5, 0.8660254]], F)
    uv = uv_sphere(P, c)
    lo, hi = F(0.5 - 1 / np.pi), F(0.5 + 1 / np.pi)
    assert abs(uv[0, 1] - hi) < 1e-6 and abs(uv[1, 1] - lo) < 1e-6
    assert uv[2, 1] == F(0.5) and uv[2, 0] == F(0.5) and abs(uv[3, 0] - 0.75) < 1e-6
    assert abs(uv[4, 1] - (0.5 + (np.pi / 6) / np.pi)) < 1e-6
    assert (uv[:, 1] >= lo).all() and (uv[:, 1] <= hi).all()


def _host_scene(miro):
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.add_triangle([0, 0, 1, 1, 0, 1, 0, 1, 1], [0, 0, 1] * 3)
    s.build(4, host_only=True)
    return s


def test_set_texcoords_validation_keeps_the_earlier_table(miro):
    s = _host_scene(miro)
    L = miro.lib()
    t0 = np.array([[0, 0], [1, 0], [0, 1]], F)
    i0 = np.array([[0, 1, 2], [NONE, NONE, NONE]], np.uint32)
    s.set_texcoords(t0, i0)

    def unchanged():
        t, ti = s.get_texcoords()
        return np.array_equal(t, t0) and np.array_equal(ti, i0)

    assert unchanged()
    from miro_amd.binding import _f32p, _u32p
    bad_t = np.array([[0, 0], [np.nan, 0], [0, 1]], F)
    assert L.mr_scene_set_texcoords(None, _f32p(t0), 3, _u32p(i0)) == -1
    assert L.mr_scene_set_texcoords(s.h, None, 3, _u32p(i0)) == -1 and unchanged()
    assert L.mr_scene_set_texcoords(s.h, _f32p(t0), 3, None) == -1 and unchanged()
    assert L.mr_scene_set_texcoords(s.h, _f32p(bad_t), 3, _u32p(i0)) == -1 and unchanged()
    for bad in ([[0, 1, 3], [NONE] * 3], [[0, 1, 2], [NONE, 0, NONE]]):
        bi = np.array(bad, np.uint32)
        assert L.mr_scene_set_texcoords(s.h, _f32p(t0), 3, _u32p(bi)) == -1 and unchanged()
    s.set_texcoords(None, None)
    t, ti = s.get_texcoords()
    assert len(t) == 0 and (ti == NONE).all()


def test_set_textures_validation_keeps_the_earlier_table(miro):
    """Every error of mr_scene_set_textures is MR_ERR_INVALID and leaves the earlier table in place -- seen through the one
    host-side trace a table leaves: while it exists mr_scene_set_materials is refused with MR_ERR_STATE."""
    from miro_amd import binding
    s = _host_scene(miro)
    L = miro.lib()
    mats = [((1, 1, 1), (0.25, 0, 0), (0, 0.5, 0), 1.0, 1.0), ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 1.0, 1.0)]
    # a material_texture without a material table
    with pytest.raises(miro.MiroError) as e:
        s.set_textures([dict(color1=(1, 1, 1), color2=(0, 0, 0), scale=1.0)], [0])
    assert e.value.status == -1
    s.set_materials(mats, [0, 1])
    s.set_textures([dict(color1=(1, 1, 1), color2=(0, 0, 0), scale=2.0)], [0, NONE])

    def table_still_there():
        with pytest.raises(miro.MiroError) as e:
            s.set_materials(mats, [0, 1])
        return e.value.status == -5

    assert table_still_there()
    img = np.full((2, 2, 3), 0.5, F)

    def desc(**kw):
        d = binding.TextureDesc()
        d.kind = kw.get("kind", binding.MR_TEX_CHECKER)
        d.color1[:] = kw.get("color1", (1, 1, 1))
        d.color2[:] = kw.get("color2", (0, 0, 0))
        d.scale = kw.get("scale", 1.0)
        if "pixels" in kw:
            d.pixels = binding._f32p(kw["pixels"])
        d.W, d.H, d.hdr = kw.get("W", 0), kw.get("H", 0), kw.get("hdr", 0)
        for k, v in enumerate(kw.get("reserved", ())):
            d.reserved[k] = v
        return d

    nan_img = img.copy()
    nan_img[1, 0, 2] = np.inf
    mt = np.array([0, NONE], np.uint32)
    bad = [desc(kind=7), desc(reserved=(0, 0, 1)), desc(color1=(np.nan, 0, 0)), desc(color2=(0, np.inf, 0)), desc(scale=np.nan),
           desc(kind=1, pixels=img, W=0, H=2), desc(kind=1, pixels=img, W=2, H=0), desc(kind=1, pixels=nan_img, W=2, H=2),
           desc(kind=1, W=2, H=2), desc(kind=1, pixels=img, W=2, H=2, hdr=2)]
    for d in bad:
        arr = (binding.TextureDesc * 1)(d)
        assert L.mr_scene_set_textures(s.h, arr, 1, binding._u32p(mt)) == -1, L.mr_last_error()
        assert table_still_there()
    good = (binding.TextureDesc * 1)(desc())
    assert L.mr_scene_set_textures(None, good, 1, binding._u32p(mt)) == -1
    assert L.mr_scene_set_textures(s.h, None, 1, binding._u32p(mt)) == -1 and table_still_there()
    many = (binding.TextureDesc * 17)(*[desc() for _ in range(17)])
    assert L.mr_scene_set_textures(s.h, many, 17, binding._u32p(mt)) == -1 and table_still_there()
    assert L.mr_scene_set_textures(s.h, good, 1, binding._u32p(np.array([1, NONE], np.uint32))) == -1 and table_still_there()
    s.set_textures([])                                                   # n_textures = 0 clears it
    s.set_materials(mats, [0, 1])


def test_obj_loader_keeps_texture_coordinates(miro, tmp_path):
    """A file with v/t, v/t/n and v//n faces: texture coordinates and indices are the restated loader's; vertices and normals
    are what the same file gives without its vt records and texture indices (the loader's pinned output, test_host_parity.py)."""
    with_t = ("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0.5\nvn 0 0 1\nvn 0 1 0\nvt 0 0\nvt 1 0\nvt 0.25 0.75\nvt 1 1\n"
              "f 1/1 2/2 3/3\nf 2/2/1 4/4/2 3/3/1\nf 1//1 3//1 4//2\n")
    without = ("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0.5\nvn 0 0 1\nvn 0 1 0\n"
               "f 1 2 3\nf 2//1 4//2 3//1\nf 1//1 3//1 4//2\n")
    a, b = tmp_path / "t.obj", tmp_path / "n.obj"
    a.write_text(with_t)
    b.write_text(without)
    s, r = miro.Scene(), miro.Scene()
    s.add_triangle([5, 5, 5, 6, 5, 5, 5, 6, 5], [0, 0, 1] * 3)          # an object in front of the mesh: it has none
    r.add_triangle([5, 5, 5, 6, 5, 5, 5, 6, 5], [0, 0, 1] * 3)
    assert s.add_obj(str(a)) == 3 and r.add_obj(str(b)) == 3
    for x, y in zip(s.arrays(), r.arrays()):
        assert x.tobytes() == y.tobytes()
    t, ti = s.get_texcoords()
    want_t, want_ti = restated_obj_texcoords(str(a))
    assert np.array_equal(t, want_t) and len(t) == 4
    assert (ti[0] == NONE).all() and np.array_equal(ti[1:], want_ti)
    assert np.array_equal(want_ti, np.array([[0, 1, 2], [1, 3, 2], [0, 0, 0]], np.uint32))
    t2, ti2 = r.get_texcoords()
    assert len(t2) == 0 and (ti2 == NONE).all()
    s.add_obj(str(a))                                                    # a second mesh: indices move by the first one's count
    assert np.array_equal(s.get_texcoords()[1][4:], want_ti + 4)


def test_texture_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_textures.hip (its remarks live in build/mr_textures.remarks.txt, which test_build_budget.py does not
    read): no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer waves per SIMD than its record in
    tests/golden/kernel_budget_textures.json, written from the build whose GPU tests were green.  The textured light-list
    kernels keep their sibling's amdgpu_waves_per_eu(6, 8) contract: at least 6 waves per SIMD, in all 12 variants."""
    cur = kernel_budget.unit_kernels("mr_textures")
    lights = [k for k in cur if "shade_lights_tex_kernel" in k]
    assert len(lights) == 12 and len(cur) == 15
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_textures.json", also_main=False)
    for name in lights:
        assert cur[name]["waves_per_simd"] >= 6, (name, cur[name])


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
KS, KT = (0.25, 0.0, 0.125), (0.0, 0.125, 0.125)
M = tuple(F(1) - F(a) - F(b) for a, b in zip(KS, KT))                   # clamp(1 - ks - kt), positive in every channel
CENTRE, RADIUS = (0.0, 1.0, 0.0), 1.0
# a mesh with texture coordinates: one triangle facing each axis (every arm of Triangle.cpp:197-200: +x -> (2, 1), +y -> (0, 2),
# +z -> (0, 1)), one whose normal has negative components only (-> (0, 1) although |n.x| is the largest), one oblique
TEX_V = np.array([[3, 0.2, -1], [3, 0.2, 1], [3, 2.2, 0],          # cross = (+4, 0, 0)
                  [-4, 0.5, -1], [-4, 0.5, 1], [-2, 0.5, 0],       # cross = (0, +4, 0)  (B - A = +z, C - A = +x, +1z)
                  [-1, 0.2, -3], [1, 0.2, -3], [0, 2.2, -3],       # cross = (0, 0, +4)
                  [-3, 0.3, 3], [-3, 2.3, 2], [-1, 0.3, 2.5],      # all components negative
                  [1.5, 0.2, 2.5], [3.0, 0.4, 3.5], [2.0, 2.0, 2.0]], F)
TEX_T = np.array([[0, 0], [1, 0], [0.5, 1], [0.1, 0.2], [0.9, 0.1], [0.4, 0.8], [2, 2], [3, 2], [2.5, 3.5], [0.3, 0.3], [0.7, 0.2],
                  [0.5, 0.9], [0, 1], [1, 1], [0.5, 0]], F)
PLAIN_V = np.array([[-2, 0.3, -2.5], [-0.5, 0.3, -2.5], [-1.2, 1.8, -2.0]], F)     # the mesh without texture coordinates
OCCLUDER = ((1.2, 2.6, 0.6), 0.5)                                                   # a refractive sphere between floor and lights
LIGHTS = [dict(position=(2.0, 6.0, 1.0), color=(1.0, 0.9, 0.8), wattage=400.0),
          dict(position=(-1.0, 7.0, -0.5), normal=(0.0, -2.0, 0.0), color=(0.8, 0.9, 1.0), wattage=3.0, radius=6.0)]
IMG = (np.random.default_rng(7).uniform(0.05, 1.0, (3, 5, 3))).astype(F)           # the sphere's image, 5 x 3


class Room:
    """One plane (material 0), one sphere (1), a mesh with texture coordinates (2), one without (3), a refractive sphere (4)"""

    def __init__(self, miro):
        s = miro.Scene(0)
        self.sphere = s.add_sphere(CENTRE, RADIUS)
        n5 = len(TEX_V) // 3
        s.add_arrays(TEX_V, np.tile(np.array([[0, 1, 0]], F), (len(TEX_V), 1)), np.arange(len(TEX_V)).reshape(-1, 3),
                     np.arange(len(TEX_V)).reshape(-1, 3))                 # objects 1 ... n5
        self.plain = 1 + n5
        s.add_arrays(PLAIN_V, np.tile(np.array([[0, 1, 0]], F), (3, 1)), [[0, 1, 2]], [[0, 1, 2]])
        self.occluder = s.add_sphere(*OCCLUDER)
        s.add_plane((0, 1, 0), (0, 0, 0), 0)
        self.n_obj = 1 + n5 + 1 + 1
        self.prim_material = np.array([1] + [2] * n5 + [3] + [4], np.uint32)
        ti = np.full((self.n_obj, 3), NONE, np.uint32)
        ti[1:1 + n5] = np.arange(len(TEX_T)).reshape(-1, 3)
        self.ti = ti
        s.build(4)
        s.set_texcoords(TEX_T, ti)
        s.set_lights(LIGHTS)
        self.scene, self.n_tex_tris = s, n5
        self.plain_phong(1.0)

    def materials(self, kd):
        spec = lambda k: ((k, k, k), KS, KT, 20.0, 1.3)                                        # noqa: E731
        return [spec(kd), spec(kd), spec(kd), ((0.5, 0.25, 0.75), (0, 0, 0), (0, 0, 0), 1.0, 1.0),
                ((0.1, 0.1, 0.1), (0, 0, 0), (0.8, 0.8, 0.8), 1.0, 1.5)]

    def plain_phong(self, kd):
        self.scene.set_textures([])
        self.scene.set_materials(self.materials(kd), self.prim_material)

    TEXTURES = [dict(color1=(1.0, 0.5, 0.25), color2=(0.125, 0.25, 0.5), scale=1.0), dict(pixels=IMG, hdr=0),
                dict(color1=(0.25, 1.0, 0.5), color2=(1.0, 0.125, 0.75), scale=10.0)]

    def textured(self, textures=None, kd=0.3):
        """floor: checker 0, sphere: image 1, textured mesh: checker 2; whatever kd the materials were given"""
        self.scene.set_textures([])
        self.scene.set_materials(self.materials(kd), self.prim_material)
        self.scene.set_textures(self.TEXTURES if textures is None else textures, [0, 1, 2, NONE, NONE])


def random_rays(miro, n, seed):
    """from a shell above the room towards points spread over it; one in eight leaves the scene upwards, one in eight aims at
    a random point of one of the six triangles in turn, one in eight at the sphere"""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-5, 5, n), rng.uniform(2.5, 7, n), rng.uniform(-5, 5, n)], axis=1)
    tgt = np.stack([rng.uniform(-5, 5, n), rng.uniform(-0.5, 2.5, n), rng.uniform(-5, 5, n)], axis=1)
    tgt[::8, 1] = 12.0
    tris = np.concatenate([TEX_V, PLAIN_V]).astype(np.float64).reshape(-1, 3, 3)
    for c, k in enumerate(range(1, n, 8)):
        b = rng.dirichlet((1, 1, 1))
        tgt[k] = b @ tris[c % len(tris)]
    for k in range(2, n, 8):
        tgt[k] = np.asarray(CENTRE) + rng.uniform(-0.6, 0.6, 3)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.zeros(n, miro.RAY_DTYPE)
    for k, name in enumerate(("ox", "oy", "oz")):
        rays[name] = o[:, k]
    for k, name in enumerate(("dx", "dy", "dz")):
        rays[name] = d[:, k]
    rays["tmin"], rays["tmax"] = 1e-4, 1e30
    return rays


class Batch:
    def __init__(self, miro, room, seed=3, n=N_RAYS, rays=None):
        import torch
        self.n = n
        rays = random_rays(miro, n, seed) if rays is None else rays
        self.rays = torch.from_numpy(rays.view(F).reshape(n, 8).copy()).cuda()
        self.hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        room.scene.trace_device(self.rays, n, self.hits)
        P = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        room.scene.hit_attrs(self.hits, n, P, None, d_rays=self.rays)
        torch.cuda.synchronize()
        self.P = P.cpu().numpy()
        self.prim = self.hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]

    def uv(self, room):
        import torch
        uv = torch.full((self.n, 2), 7.0, dtype=torch.float32, device="cuda")
        room.scene.hit_uv(self.rays, self.hits, self.n, uv)
        torch.cuda.synchronize()
        return uv

    def tex_of(self, room, textures, material_texture):
        """mr_texture_lookup(mr_hit_uv(hit)) per ray by its material's texture; m (the material's own colour) elsewhere"""
        import torch
        uv = self.uv(room)
        mat = np.where(self.prim == MISS, 0, np.where(self.prim & PLANE_BIT, 0, room.prim_material[np.minimum(self.prim, room.n_obj - 1)]))
        out = np.zeros((self.n, 3), F)
        out[:] = np.array(M, F)
        for m_id, t_id in enumerate(material_texture):
            if t_id == NONE:
                continue
            rgb = torch.empty((self.n, 3), dtype=torch.float32, device="cuda")
            room.scene.texture_lookup(t_id, uv, self.n, rgb)
            torch.cuda.synchronize()
            sel = (mat == m_id) & (self.prim != MISS)
            out[sel] = rgb.cpu().numpy()[sel]
        return out, mat


@pytest.fixture(scope="module")
def room(miro):
    return Room(miro)


@pytest.fixture(scope="module")
def batch(miro, room):
    return Batch(miro, room)


@pytest.mark.gpu
def test_hit_uv_against_the_restatement(miro, room, batch):
    """Plane and triangle hits bit-equal (pure + - * /), every arm of the axis rule taken, (0, 0) for the mesh without texture
    coordinates and for misses, sphere hits within rtol 1e-5 / atol 1e-7 and inside the clamp's range."""
    uv = batch.uv(room).cpu().numpy()
    prim, P = batch.prim, batch.P
    miss = prim == MISS
    plane = (prim & PLANE_BIT) != 0
    plane &= ~miss
    sph = prim == room.sphere
    occ = prim == room.occluder
    tri = ~miss & ~plane & (prim >= 1) & (prim < 1 + room.n_tex_tris)
    plain = prim == room.plain
    print("hits: plane %d sphere %d occluder %d textured triangles %d plain %d miss %d" % (plane.sum(), sph.sum(), occ.sum(), tri.sum(),
                                                                                          plain.sum(), miss.sum()))
    assert plane.sum() > 100 and sph.sum() > 20 and tri.sum() > 20 and miss.sum() > 20
    assert uv[plane].tobytes() == uv_plane(P[plane]).tobytes()
    assert (uv[miss] == 0).all() and (uv[plain] == 0).all()
    k = prim[tri] - 1
    want, (i, j) = uv_triangle(P[tri], TEX_V[3 * k], TEX_V[3 * k + 1], TEX_V[3 * k + 2], TEX_T[3 * k], TEX_T[3 * k + 1], TEX_T[3 * k + 2])
    assert uv[tri].tobytes() == want.tobytes()
    arms = set(zip(i.tolist(), j.tolist()))
    assert arms == {(2, 1), (0, 2), (0, 1)}, arms
    assert set(np.unique(k).tolist()) >= {0, 1, 2, 3}, np.unique(k)                 # each axis and the all-negative normal were hit
    for which, (c, r) in ((sph, (CENTRE, RADIUS)), (occ, OCCLUDER)):
        want = uv_sphere(P[which], c)
        assert np.allclose(uv[which], want, rtol=1e-5, atol=1e-7)
        assert (uv[which][:, 1] >= F(0.5 - 1 / np.pi) - 1e-6).all() and (uv[which][:, 1] <= F(0.5 + 1 / np.pi) + 1e-6).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 10.0, 0.5])
def test_checker_lookup_is_bit_equal(miro, room, scale):
    import torch
    n = 100000
    uv = np.random.default_rng(11).uniform(-8, 8, (n, 2)).astype(F)
    c1, c2 = (1.0, 0.5, 0.25), (0.125, 0.25, 0.5)
    room.textured([dict(color1=c1, color2=c2, scale=scale)] * 3)
    d_uv = torch.from_numpy(uv).cuda()
    rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    room.scene.texture_lookup(0, d_uv, n, rgb, cnt)
    torch.cuda.synchronize()
    want = checker(uv, c1, c2, scale)
    assert rgb.cpu().numpy().tobytes() == want.tobytes()
    assert int(cnt.item()) == 0 and 0.4 < (want[:, 0] == 1.0).mean() < 0.6
    bad = np.array([[np.nan, 0.5], [0.5, np.inf], [3e9, 0.5], [1.5, 0.5]], F)      # the first three: undefined -> color1, counted
    rgb = torch.empty((4, 3), dtype=torch.float32, device="cuda")
    room.scene.texture_lookup(0, torch.from_numpy(bad).cuda(), 4, rgb, cnt)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 3
    assert (rgb.cpu().numpy()[:3] == np.array(c1, F)).all()
    assert rgb.cpu().numpy()[3].tobytes() == checker(bad[3:], c1, c2, scale).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 2), (5, 3)])
@pytest.mark.parametrize("hdr", [0, 1])
def test_image_lookup(miro, room, shape, hdr):
    """Sizes 2 x 2 and 5 x 3 over [0, 3)^2 (both axes wrap), u == 1 exactly (extrapolates), then negative and NaN coordinates:
    0, and counted exactly.  Beyond the first period the error term -- taken from the WRAPPED index -- exceeds 1 and the blend
    extrapolates below 0, where tonemapValue's pow gives NaN (std::min keeps it): the same lanes must be NaN on both sides (the
    blend itself is the same float32 bits)."""
    import torch
    w, h = shape
    rng = np.random.default_rng(100 * w + hdr)
    img = rng.uniform(0.05, 2.0 if hdr else 1.0, (h, w, 3)).astype(F)
    n = 20000
    uv = rng.uniform(0, 3, (n, 2)).astype(F)
    uv[0], uv[1], uv[2] = (1.0, 0.25), (0.25, 1.0), (1.0, 1.0)
    want, inside = image_lookup(uv, img, hdr)
    assert inside.all()                                                  # the restatement alone never leaves the image: nothing is excluded
    room.textured([dict(pixels=img, hdr=hdr)] * 3)
    rgb = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    room.scene.texture_lookup(1, torch.from_numpy(uv).cuda(), n, rgb, cnt)
    torch.cuda.synchronize()
    got = rgb.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and (hdr or not nan.any()) and nan.mean() < 0.5
    err, top = np.abs(got - want)[~nan], np.nanmax(want)
    print("image %dx%d hdr %d: max abs err %.3g (max value %.3g, NaN %d)" % (w, h, hdr, err.max(), top, nan.sum()))
    assert int(cnt.item()) == 0
    assert (err <= 1e-5 * np.abs(want[~nan]) + 1e-7 * top).all()
    bad = uv[:1000].copy()
    bad[::2, 0] = -bad[::2, 0] - 0.01
    bad[1::5, 1] = np.nan
    n_bad = int(((bad[:, 0] < 0) | np.isnan(bad[:, 1])).sum())
    rgb = torch.full((1000, 3), 5.0, dtype=torch.float32, device="cuda")
    room.scene.texture_lookup(1, torch.from_numpy(bad).cuda(), 1000, rgb, cnt)
    torch.cuda.synchronize()
    got = rgb.cpu().numpy()
    undefined = (bad[:, 0] < 0) | np.isnan(bad[:, 1])
    assert int(cnt.item()) == n_bad and (got[undefined] == 0).all()
    w2, _ = image_lookup(bad[~undefined], img, hdr)
    assert np.allclose(got[~undefined], w2, rtol=1e-5, atol=1e-7 * top, equal_nan=True)


def _shade_lights(room, batch):
    import torch
    out = torch.zeros((batch.n, 3), dtype=torch.float32, device="cuda")
    room.scene.shade_lights(batch.rays, batch.hits, batch.n, None, d_ray_rgb=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.gpu
def test_white_checker_is_plain_white_phong(miro, room, batch):
    """A checker with both colours (1, 1, 1) on TexturedPhong(ks = kt = 0): mr_shade_lights' d_ray_rgb bit-equal to the same
    scene with plain white Phong (one point and one disc light)."""
    white = lambda: [((1, 1, 1), (0, 0, 0), (0, 0, 0), 20.0, 1.0)] * 4 + [room.materials(1.0)[4]]      # noqa: E731
    room.scene.set_textures([])
    room.scene.set_materials(white(), room.prim_material)
    plain = _shade_lights(room, batch)
    room.scene.set_textures([dict(color1=(1, 1, 1), color2=(1, 1, 1), scale=3.0)], [0, 0, 0, NONE, NONE])
    tex = _shade_lights(room, batch)
    assert plain.max() > 0 and tex.tobytes() == plain.tobytes()


def _compose(A, B, tex):
    return ((A - B) * tex / np.array(M, F) + B).astype(F)


@pytest.mark.gpu
def test_shade_lights_textured(miro, room, batch):
    """Checker floor, image sphere and a checkered mesh under two lights and a refractive occluder: the textured d_ray_rgb is
    (A - B) * tex / m + B per ray and channel, rtol 1e-5, atol 1e-6 max(A); and it differs from A by more than 1 %."""
    room.plain_phong(1.0)
    A = _shade_lights(room, batch)
    room.plain_phong(0.0)
    B = _shade_lights(room, batch)
    room.textured()
    T = _shade_lights(room, batch)
    tex, mat = batch.tex_of(room, Room.TEXTURES, [0, 1, 2, NONE, NONE])
    plain = (mat >= 3) | (batch.prim == MISS)
    want = np.where(plain[:, None], A, _compose(A, B, tex))
    err = np.abs(T - want)
    print("shade_lights: max(A) %.4g, max abs err %.3g, max |T - A| %.3g, rays lit %d" % (A.max(), err.max(), np.abs(T - A).max(), (A.max(axis=1) > 0).sum()))
    assert (A.max(axis=1) > 0).sum() > 200 and (B.max(axis=1) > 0).sum() > 0
    assert (err <= 1e-5 * np.abs(want) + 1e-6 * A.max()).all()
    assert np.abs(T - A).max() > 0.01 * A.max()


@pytest.mark.gpu
def test_shade_accumulate_textured(miro, room, batch):
    """The same composition through mr_gen_shadow_rays -> mr_trace_indirect -> mr_shade_accumulate with one point light, one
    addition per pixel (spp = 1: deterministic)."""
    import torch
    s, n = room.scene, batch.n
    lt = LIGHTS[0]

    def chain():
        sh_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        sh_hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        src = torch.empty(n, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        s.gen_shadow_rays(batch.rays, batch.hits, n, lt["position"], sh_rays, src, cnt)
        s.trace_indirect(sh_rays, cnt, n, sh_hits)
        s.shade_accumulate(batch.rays, batch.hits, None, None, n, sh_rays, sh_hits, src, cnt, lt["position"], lt["wattage"], rgb,
                           color=lt["color"])
        torch.cuda.synchronize()
        return rgb.cpu().numpy()

    room.plain_phong(1.0)
    A = chain()
    room.plain_phong(0.0)
    B = chain()
    room.textured()
    T = chain()
    tex, mat = batch.tex_of(room, Room.TEXTURES, [0, 1, 2, NONE, NONE])
    plain = (mat >= 3) | (batch.prim == MISS)
    want = np.where(plain[:, None], A, _compose(A, B, tex))
    err = np.abs(T - want)
    print("shade_accumulate: max(A) %.4g, max abs err %.3g, max |T - A| %.3g" % (A.max(), err.max(), np.abs(T - A).max()))
    assert (A.max(axis=1) > 0).sum() > 200
    assert (err <= 1e-5 * np.abs(want) + 1e-6 * A.max()).all()
    assert np.abs(T - A).max() > 0.01 * A.max()


FRAME = dict(eye=(0.0, 2.5, 7.0), lookat=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0), fov=45.0, light=(3.0, 8.0, 4.0), wattage=900.0)
FRAME_KS = (0.5, 0.5, 0.5)


def _frame_scene(miro):
    s = miro.Scene(0)
    s.add_sphere((0.0, 1.2, 0.0), 1.2)
    s.add_triangle([-3, 0.1, -2, -1.5, 0.1, -2, -2.2, 1.5, -2], [0, 0, 1] * 3)
    s.add_plane((0, 1, 0), (0, 0, 0), 0)
    s.build(4)
    return s


def _frame_materials(kd):
    return [((kd, kd, kd), (0.25, 0.25, 0.25), (0, 0, 0), 20.0, 1.0), ((0, 0, 0), FRAME_KS, (0, 0, 0), 20.0, 1.0),
            ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 1.0, 1.0)]


@pytest.mark.gpu
def test_refusals_on_a_textured_scene(miro):
    """mr_render_direct, mr_shade_direct, mr_trace_level and mr_trace_photons: MR_ERR_STATE while the scene has a texture table,
    and they work again once it is cleared."""
    import torch
    from miro_amd import binding
    s = _frame_scene(miro)
    s.set_materials(_frame_materials(1.0), [1, 2])
    W, H = 16, 12
    n = W * H
    cam = binding.make_camera(FRAME["eye"], FRAME["lookat"], FRAME["up"], FRAME["fov"])
    f32 = dict(dtype=torch.float32, device="cuda")
    rays, hits, sh_rays, sh_hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32), torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
    src, cnt = torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    rgb = torch.zeros((n, 3), **f32)
    s.gen_eye_rays(cam, W, H, rays)
    s.trace_device(rays, n, hits)
    s.gen_shadow_rays(rays, hits, n, FRAME["light"], sh_rays, src, cnt)
    s.trace_indirect(sh_rays, cnt, n, sh_hits)
    disc = dict(position=(0.0, 6.0, 0.0), normal=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0), wattage=10.0, radius=1.0)

    def calls():
        yield "render_direct", lambda: s.render_direct(cam, W, H, rgb, FRAME["light"], FRAME["wattage"])
        yield "shade_direct", lambda: s.shade_direct(rays, hits, n, sh_hits, src, cnt, FRAME["light"], FRAME["wattage"], rgb)
        yield "trace_level", lambda: s.trace_level(rays, None, None, None, n, rgb, FRAME["light"], FRAME["wattage"])
        yield "trace_photons", lambda: s.trace_photons(miro.PhotonMap(2000), disc, 100, 2000)

    s.set_textures([dict(color1=(1, 1, 1), color2=(0, 0, 0), scale=1.0)], [0, NONE, NONE])
    for name, call in calls():
        with pytest.raises(miro.MiroError) as e:
            call()
        assert e.value.status == -5 and ("mr_shade_lights" in str(e.value) or "textures" in str(e.value)), (name, str(e.value))
    s.set_textures([])
    for name, call in calls():
        call()
    torch.cuda.synchronize()
    assert float(rgb.max()) > 0


@pytest.mark.gpu
def test_textured_frame_through_render_specular(miro):
    """64 x 48, 4 spp, depth 2, fused="auto" (must not raise: a textured scene takes the batched path): a mirror sphere over the
    checker plane, so that secondary rays see textured hits too.  The frame equals the per-ray composition (A - B) * tex / m + B
    summed with the rays' weights over the levels, A and B from the untextured kernels."""
    import torch
    from miro_amd import frame
    s = _frame_scene(miro)
    prim_material = [1, 2]
    checker_tex = [dict(color1=(1.0, 0.25, 0.125), color2=(0.125, 0.5, 1.0), scale=1.0)]
    m = F(1) - F(0.25)
    W, H, spp, depth = 64, 48, 4, 2
    s.set_materials(_frame_materials(0.4), prim_material)
    s.set_textures(checker_tex, [0, NONE, NONE])
    fr = frame.FrameRenderer(s, FRAME, W, H, spp=spp)
    fr.generate()
    per_level = fr.render_specular(depth=depth, fused="auto")
    torch.cuda.synchronize()
    got = fr.d_rgb.cpu().numpy().copy()
    assert len(per_level) == depth + 1 and per_level[1][0] > 0

    # the same levels by hand: per-ray L of the untextured kernels (one point light: the chain's bits) and per-ray lookups
    s.set_lights([dict(position=FRAME["light"], color=(1.0, 1.0, 1.0), wattage=FRAME["wattage"])])
    want = np.zeros((W * H, 3), np.float64)
    rays, weights, pixels, n = fr.d_rays, None, None, fr.n
    f32 = dict(dtype=torch.float32, device="cuda")
    seen_secondary_floor = 0
    for level in range(depth + 1):
        hits = torch.empty((n, 4), **f32)
        s.trace_device(rays, n, hits)
        L = {}
        for kd in (1.0, 0.0):
            s.set_textures([])
            s.set_materials(_frame_materials(kd), prim_material)
            out = torch.zeros((n, 3), **f32)
            s.shade_lights(rays, hits, n, None, d_ray_rgb=out)
            torch.cuda.synchronize()
            L[kd] = out.cpu().numpy()
        s.set_textures(checker_tex, [0, NONE, NONE])
        uv, tex = torch.empty((n, 2), **f32), torch.empty((n, 3), **f32)
        s.hit_uv(rays, hits, n, uv)
        s.texture_lookup(0, uv, n, tex)
        torch.cuda.synchronize()
        prim = hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
        floor = (prim != MISS) & ((prim & PLANE_BIT) != 0)
        if level > 0:
            seen_secondary_floor += int(floor.sum())
        comp = np.where(floor[:, None], (L[1.0] - L[0.0]) * tex.cpu().numpy() / m + L[0.0], L[1.0]).astype(np.float64)
        w = weights.cpu().numpy().astype(np.float64) if weights is not None else np.ones((n, 3))
        pix = pixels.cpu().numpy().astype(np.int64) if pixels is not None else np.arange(n) // spp
        np.add.at(want, pix, comp * w / spp)
        if level == depth:
            break
        out_rays, out_w = torch.empty((3 * n, 8), **f32), torch.empty((3 * n, 3), **f32)
        out_pix = torch.empty(3 * n, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        s.gen_secondary_rays(rays, hits, weights, pixels, n, out_rays, out_w, out_pix, cnt, spp=spp)
        n = int(cnt.item())
        rays, weights, pixels = out_rays[:n], out_w[:n], out_pix[:n]
    assert seen_secondary_floor > 100
    err = np.abs(got - want)
    print("frame: max %.4g, max abs err %.3g" % (want.max(), err.max()))
    assert (err <= 1e-5 * np.abs(want) + 1e-6 * want.max()).all()
    # and the texture shows: the untextured frame differs
    s.set_textures([])
    s.set_materials(_frame_materials(1.0), prim_material)
    fr.render_specular(depth=depth, fused="auto")
    torch.cuda.synchronize()
    assert np.abs(fr.d_rgb.cpu().numpy() - got).max() > 0.01 * got.max()
