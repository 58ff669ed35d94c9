"""mr_scene_set_environment / mr_shade_environment -- what a ray that leaves the scene is worth: Scene::getEnvironmentMap
(Scene.cpp:338-342,657-688) over LoadedTexture (Texture.cpp:23-28,52-91,161-185), in csrc/mr_environment.hip.

The checker is a restatement of the cited lines written here in numpy float32, one operation per rounding (the constructor's
blur in np.longdouble, as the reference accumulates it).  It imports nothing from the product's lookup code; atan2 / asin are
numpy's double functions rounded to float, which the first test shows to be mm_atan2f / mm_asinf of include/miro_math.h bit
for bit.  PARITY UNPINNED: the reference cannot be built here and publishes no numbers for its environment; the checker is a
restatement written from the cited lines."""
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
PI = F(3.1415926535897932384626433832795028841972)              # Miro.h:10
MISS = 0xFFFFFFFF
RTOL, ATOL_OF_MAX = 1e-5, 1e-7                                  # the project's tolerance for shaded values (test_lights.py)
ROT = (float(PI / F(3) + F(0.05)), float(PI / F(8)))             # assignment3.cpp:51
IMG_W, IMG_H = 256, 128
LOWRES_WIDTH = 24                                               # Texture.h:297


# ---- the restatement -----------------------------------------------------------------------------------------------------
def synthetic_hdr(seed=168, W=IMG_W, H=IMG_H):
    """A seeded float image [H, W, 3]: a smooth sky gradient, noise, and a few texels in the hundreds (a sun)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([0.3 + 0.5 * y / H, 0.4 + 0.3 * np.sin(x / 17.0) ** 2, 0.2 + 0.6 * x / W], 2) + rng.rand(H, W, 3) ** 4 * 2.0
    for _ in range(6):
        img[rng.randint(H), rng.randint(W)] = 150.0 + 400.0 * rng.rand(3)
    return np.ascontiguousarray(img, F)


def restate_constructor(img, swap=True):
    """LoadedTexture::LoadedTexture (Texture.cpp:34-91) for a FIT_RGBF image: (m_maxIntensity, low-res image)."""
    h, w = img.shape[:2]
    max_intensity = F(max(F(-1e15), img.max()))                                       # :34-50
    lrw, lrh = LOWRES_WIDTH, int(F(LOWRES_WIDTH) * (F(h) / F(w)))                     # :53
    bw, bh = w // lrw, h // lrh
    low = np.zeros((lrh, lrw, 3), F)
    sigma = F(1)
    norm = 1.0 / (2.0 * float(PI) * float(sigma))                                     # :80, in double
    for i in range(lrh):
        for j in range(lrw):
            midX, midY = bw * j + bw // 2, bh * i + bh // 2                           # :70-71
            jj = np.arange(bw * j, min(bw * j + bw, w))
            ii = np.arange(bh * i, min(bh * i + bh, h))
            x, y = (jj - midX).astype(F)[None, :], (ii - midY).astype(F)[:, None]
            e = np.exp(-(x * x + y * y) / (F(2) * sigma))                             # exp(float)
            g = (norm * e.astype(np.float64)).astype(np.longdouble)
            acc = (g[:, :, None] * img[ii[0]:ii[-1] + 1, jj[0]:jj[-1] + 1].astype(np.longdouble)).sum(axis=(0, 1))
            c = acc.astype(F)
            low[i, j] = (c[0], c[2], c[1]) if swap else c                             # setPixel, FIT_RGBF (:118-124)
    return max_intensity, low


def restate_coords(d, rot):
    """Scene.cpp:665-676: (u, v, fold, wrap) of directions d [n, 3] float32"""
    with np.errstate(invalid="ignore"):
        at = np.arctan2(d[:, 0].astype(np.float64), d[:, 2].astype(np.float64)).astype(F)
        phi = (at + F(rot[0])) + PI                                                   # :665
        theta = np.arcsin(d[:, 1].astype(np.float64)).astype(F) + F(rot[1])           # :666
        fold = theta > PI / F(2)                                                      # :667
        phi = np.where(fold, phi + PI, phi)
        theta = np.where(fold, theta - F(2) * (theta - PI / F(2)), theta)
        wrap = phi > F(2) * PI                                                        # :672
        phi = np.where(wrap, phi - F(2) * PI, phi)
        u = phi / (F(2) * PI)                                                         # :675
        v = ((theta / PI).astype(np.float64) + 0.5).astype(F)                         # :676
    assert u.dtype == F and v.dtype == F
    return u, v, fold, wrap


def restate_axis(w, c):
    """Texture.cpp:170-178 for one axis: (i1, i2, error, undefined)"""
    with np.errstate(invalid="ignore"):
        p = F(w) * c
        undefined = ~(np.abs(p) < F(2147483520.0))
        t = np.trunc(np.where(undefined, F(0), p)).astype(np.int64)
        i1, i2 = np.fmod(t, w), np.fmod(t + 1, w)                                     # C's % : the sign of the dividend
        err = p - i1.astype(F)                                                        # :174, from the WRAPPED index
        undefined |= (i1 < 0) | (i2 < 0)
    return np.where(undefined, 0, i1), np.where(undefined, 0, i2), err, undefined


def restate_lookup(img, max_intensity, u, v):
    """LoadedTexture::lookup (Texture.cpp:161-185) + tonemapValue (:27): (value [n, 3], undefined, fragile)"""
    h, w = img.shape[:2]
    x1, x2, xe, ux = restate_axis(w, u)
    y1, y2, ye, uy = restate_axis(h, v)
    undefined = ux | uy
    xe, ye = xe[:, None], ye[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        f = (img[y1, x1] * (1 - xe) + img[y1, x2] * xe) * (1 - ye) + (img[y2, x1] * (1 - xe) + img[y2, x2] * xe) * ye    # :181
        a = np.power(f / F(max_intensity), F(0.5)) * F(1.5)
        val = np.where(F(1) < a, F(1), a).astype(F)                                   # std::min(a, 1.0f)
    assert f.dtype == F
    val[undefined] = 0                                                                # defined here; undefined in the reference
    ulp = F(2.0 ** -23)
    fragile = (np.abs(u - F(1)) <= 2 * ulp) | (np.abs(v - F(1)) <= 2 * ulp)           # where the wrapped-error quirk switches on
    return val, undefined, fragile & ~undefined


def restate_environment(d, rot, img, max_intensity):
    u, v, fold, wrap = restate_coords(d, rot)
    val, undefined, fragile = restate_lookup(img, max_intensity, u, v)
    return val, dict(undefined=undefined, fragile=fragile, fold=fold, wrap=wrap, u=u, v=v)


def direction_of(rays):
    return np.stack([rays["dx"], rays["dy"], rays["dz"]], 1).astype(F)


def ray_set(miro, n_random=1000000, seed=168):
    """Seeded rays around the unit sphere of the `sphere` scene (uniform unit directions) plus that scene's eye rays."""
    from helpers import random_rays
    from miro_amd import scenes
    rays = random_rays(miro.RAY_DTYPE, n_random, (-1, -1, -1), (1, 1, 1), seed)
    d = scenes.SCENES["sphere"]
    W = H = 256
    eye, look, up = (np.asarray(d[k], np.float64) for k in ("eye", "lookat", "up"))
    wv = eye - look
    wv /= np.linalg.norm(wv)
    uv = np.cross(up, wv)
    uv /= np.linalg.norm(uv)
    vv = np.cross(wv, uv)
    t = np.tan(np.radians(d["fov"]) / 2)
    ys, xs = np.mgrid[0:H, 0:W]
    dirs = (((xs + 0.5) / W * 2 - 1) * t * W / H)[..., None] * uv + (((ys + 0.5) / H * 2 - 1) * t)[..., None] * vv - wv
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    cam = np.zeros(W * H, miro.RAY_DTYPE)
    cam["ox"], cam["oy"], cam["oz"] = eye
    cam["dx"], cam["dy"], cam["dz"] = dirs.reshape(-1, 3).astype(F).T
    cam["tmax"] = 1e12
    # sixteen rays beside the scene whose |d.y| exceeds 1 by an ulp (asin gives NaN: an undefined lookup), sixteen straight up / down
    odd = np.zeros(32, miro.RAY_DTYPE)
    odd["ox"], odd["oy"], odd["oz"], odd["tmax"] = 5.0, 5.0, 5.0, 1e12
    odd["dy"][:16] = np.where(np.arange(16) % 2 == 0, 1, -1) * np.nextafter(F(1), F(2))
    odd["dy"][16:] = np.where(np.arange(16) % 2 == 0, 1, -1)
    odd["dx"] = np.linspace(-1e-4, 1e-4, 32).astype(F)
    return np.concatenate([rays, cam, odd])


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def host_scene(miro):
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.build(4, host_only=True)
    return s


def test_environment_entries_are_exported_and_declared(miro, tmp_path):
    from miro_amd import binding
    L = miro.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "miro_hip.h")).read(), flags=re.S)
    for name in ("mr_scene_set_environment", "mr_scene_get_environment", "mr_shade_environment"):
        assert hasattr(L, name) and name in miro.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, src), name
    assert binding.MR_ENV_LOWRES == 1 << 16 and re.search(r"MR_ENV_LOWRES\s*=\s*1u\s*<<\s*16", src)
    prog = ('#include "miro_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%d %d %d\\n", '
            '(int)sizeof(mr_environment_desc), (int)offsetof(mr_environment_desc, pixels), (int)offsetof(mr_environment_desc, rotation)); return 0; }\n')
    exe = str(tmp_path / "sizeof_env_desc")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=prog.encode(), check=True)
    size, off_px, off_rot = (int(x) for x in subprocess.check_output([exe]).split())
    D = binding.EnvironmentDesc
    assert (size, off_px, off_rot) == (C.sizeof(D), D.pixels.offset, D.rotation.offset) == (64, 16, 32)


def test_mm_atan2f_and_mm_asinf_are_the_rounded_double_functions(tmp_path):
    """400 000 seeded argument pairs through a g++ program that includes miro_math.h: mm_atan2f(a, b) and mm_asinf(a) equal
    np.arctan2 / np.arcsin evaluated in double and rounded to float -- all four quadrants, the axes, +-0, |a| = 1, and
    |a| > 1 -> NaN for asin."""
    exe = str(tmp_path / "env_math")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "env_math.cpp"), "-o", exe])
    rng = np.random.RandomState(168)
    n = 400000
    pairs = np.empty((n, 2), F)
    k = n // 4
    pairs[:k] = rng.randn(k, 2)                                                # every quadrant, all magnitudes around 1
    pairs[k:2 * k] = rng.uniform(-1, 1, (k, 2))                                # asin's whole domain
    dirs = rng.randn(k, 3)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pairs[2 * k:3 * k] = dirs[:, :2]                                           # components of unit directions
    pairs[3 * k:] = rng.randn(n - 3 * k, 2) * 10.0 ** rng.uniform(-30, 30, (n - 3 * k, 1))
    special = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, np.nextafter(F(1), F(2)), -np.nextafter(F(1), F(2)), np.nextafter(F(1), F(0)),
               1e-40, -1e-40, 2.0, -3.0, 1e30, -1e30, float(2 ** 0.5 - 1)]
    grid = np.array([(a, b) for a in special for b in special], F)
    pairs[-len(grid):] = grid
    a, b = pairs[:, 0], pairs[:, 1]
    assert ((a > 0) & (b > 0)).any() and ((a > 0) & (b < 0)).any() and ((a < 0) & (b > 0)).any() and ((a < 0) & (b < 0)).any()
    assert ((a == 0) & (b != 0)).any() and ((b == 0) & (a != 0)).any() and ((a == 0) & (b == 0)).any()
    assert (np.signbit(a) & (a == 0)).any() and (np.abs(a) == 1).any() and (np.abs(a) > 1).sum() > 1000
    pin, pout = str(tmp_path / "pairs.bin"), str(tmp_path / "out.bin")
    pairs.tofile(pin)
    subprocess.check_call([exe, pin, pout])
    got = np.fromfile(pout, F).reshape(n, 2)
    with np.errstate(invalid="ignore"):
        want_atan2 = np.arctan2(a.astype(np.float64), b.astype(np.float64)).astype(F)
        want_asin = np.arcsin(a.astype(np.float64)).astype(F)
    assert np.isnan(want_asin[np.abs(a) > 1]).all() and not np.isnan(want_asin[np.abs(a) <= 1]).any()
    assert np.array_equal(got[:, 0], want_atan2)
    assert np.array_equal(got[:, 1], want_asin, equal_nan=True)
    assert np.array_equal(np.signbit(got[:, 0]), np.signbit(want_atan2))                   # atan2(-0, x > 0) = -0 included
    assert np.array_equal(np.signbit(got[:, 1])[np.abs(a) <= 1], np.signbit(want_asin)[np.abs(a) <= 1])


def test_set_environment_restates_the_loadedtexture_constructor(miro):
    """On a host_only scene (no device is touched): the image and its maximum come back exactly; the low-res image is 24 x 12
    and matches the restatement of Texture.cpp:52-91 within rtol 1e-6 (expf in libm vs numpy may differ by an ulp) WITH green
    and blue exchanged, and does not match it without the exchange."""
    s = host_scene(miro)
    assert s.get_environment(0) == (None, 0.0) and s.get_environment(1) == (None, 0.0)
    img = synthetic_hdr()
    assert (img > 100).sum() >= 6
    s.set_environment(bg_color=(0.1, 0.2, 0.3), pixels=img, rotation=ROT)
    full, mx = s.get_environment(0)
    assert full.shape == (IMG_H, IMG_W, 3) and np.array_equal(full, img) and mx == float(img.max())
    low, mx1 = s.get_environment(1)
    want_max, want = restate_constructor(img)
    _, unswapped = restate_constructor(img, swap=False)
    print("low-res %s, max %.6g, worst relative error %.3g" % (low.shape, mx, np.abs(low / want - 1).max()))
    assert low.shape == (12, LOWRES_WIDTH, 3) and mx1 == mx == float(want_max)
    assert np.allclose(low, want, rtol=1e-6, atol=0)
    assert not np.allclose(low, unswapped, rtol=1e-3, atol=0)
    # un-normalised: a block of a constant image sums to the Gaussian's own mass, not to the constant
    s.set_environment(pixels=np.full((48, 96, 3), 2.0, F))
    low, mx = s.get_environment(1)
    mass = restate_constructor(np.full((48, 96, 3), 1.0, F))[1][0, 0, 0]
    assert low.shape == (12, 24, 3) and mx == 2.0 and np.allclose(low, 2.0 * mass, rtol=1e-6) and abs(mass - 1.0) > 1e-3
    s.clear_environment()
    assert s.get_environment(0) == (None, 0.0)
    # before the build, and kept across it
    t = miro.Scene()
    t.set_environment(pixels=img)
    t.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    t.build(4, host_only=True)
    assert np.array_equal(t.get_environment(0)[0], img)


def test_environment_argument_errors(miro):
    """Every invalid description: MR_ERR_INVALID with a message, and the scene keeps its previous environment;
    mr_shade_environment on a host_only or unbuilt scene: MR_ERR_STATE, never a CPU path."""
    from miro_amd import binding
    L = miro.lib()
    s = host_scene(miro)
    img = synthetic_hdr()
    s.set_environment(bg_color=(0.5, 0.25, 0.125), pixels=img, rotation=ROT)
    before = s.get_environment(0), s.get_environment(1)

    def desc(pixels=img, bg=(0, 0, 0), rot=(0.0, 0.0), reserved=(0,) * 6):
        d = binding.EnvironmentDesc()
        d.bg_color[:] = bg
        d.rotation[:] = rot
        d.reserved[:] = reserved
        if pixels is not None:
            d.H, d.W = pixels.shape[:2]
            d.pixels = pixels.ctypes.data_as(C.POINTER(C.c_float))
        return d

    inf, nan = float("inf"), float("nan")
    bad_px = img.copy()
    bad_px[7, 9, 1] = nan
    inf_px = img.copy()
    inf_px[0, 0, 0] = inf
    cases = [(desc(reserved=(0, 0, 0, 1, 0, 0)), b"reserved"), (desc(reserved=(5, 0, 0, 0, 0, 0)), b"reserved"),
             (desc(bg=(0, nan, 0)), b"finite"), (desc(bg=(inf, 0, 0), pixels=None), b"finite"),
             (desc(rot=(nan, 0.0)), b"finite"), (desc(rot=(0.0, inf)), b"finite"),
             (desc(pixels=bad_px), b"finite"), (desc(pixels=inf_px), b"finite"),
             (desc(pixels=np.ones((12, 23, 3), F)), b"width"), (desc(pixels=np.ones((5, 256, 3), F)), b"height 0"),
             (desc(rot=(-0.001, 0.0)), b"rotation[0]"), (desc(rot=(6.3, 0.0)), b"rotation[0]"),
             (desc(rot=(0.0, -0.001)), b"rotation[1]"), (desc(rot=(0.0, 1.58)), b"rotation[1]"),
             (desc(pixels=None, rot=(7.0, 0.0)), b"rotation[0]")]
    for d, word in cases:
        assert L.mr_scene_set_environment(s.h, C.byref(d)) == binding.MR_ERR_INVALID, word
        assert word in L.mr_last_error(), (word, L.mr_last_error())
        after = s.get_environment(0), s.get_environment(1)
        assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(after, before)), word
    assert L.mr_scene_set_environment(None, C.byref(desc())) == binding.MR_ERR_INVALID
    assert L.mr_scene_get_environment(s.h, 2, None, None, None, None) == binding.MR_ERR_INVALID
    # the limits themselves are inside
    s.set_environment(pixels=np.ones((12, 24, 3), F), rotation=(float(F(2) * PI), float(PI / F(2))))
    dummy = C.c_void_p(16)
    assert L.mr_shade_environment(s.h, dummy, dummy, None, None, None, 4, 1, 0, dummy, None, None, None) == binding.MR_ERR_STATE
    assert b"CPU" in L.mr_last_error() or b"device" in L.mr_last_error()
    assert L.mr_shade_environment(None, dummy, dummy, None, None, None, 4, 1, 0, dummy, None, None, None) == binding.MR_ERR_INVALID
    t = miro.Scene()
    t.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    assert L.mr_shade_environment(t.h, dummy, dummy, None, None, None, 4, 1, 0, dummy, None, None, None) == binding.MR_ERR_STATE


def test_restatement_self_checks(miro):
    """The checker against things that are not itself: directions through texel centres land in those texels; the fold and the
    2 pi wrap both occur in the GPU test's ray set; the rays it calls fragile (u or v within 2 ulp of 1) or undefined are at
    most 0.1 % of that set."""
    img = synthetic_hdr()
    h, w = img.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    u0, v0 = (xs.ravel() + 0.5) / w, (ys.ravel() + 0.5) / h
    a, theta = 2 * np.pi * u0 - np.pi, (v0 - 0.5) * np.pi                               # phi = atan2(d.x, d.z) + PI, no rotation
    d = np.stack([np.sin(a) * np.cos(theta), np.sin(theta), np.cos(a) * np.cos(theta)], 1).astype(F)
    u, v, fold, wrap = restate_coords(d, (0.0, 0.0))
    x1, _, xe, ux = restate_axis(w, u)
    y1, _, ye, uy = restate_axis(h, v)
    assert not (ux | uy).any() and not fold.any()
    assert np.array_equal(x1, xs.ravel()) and np.array_equal(y1, ys.ravel())
    assert np.abs(xe - 0.5).max() < 1e-3 and np.abs(ye - 0.5).max() < 1e-3
    # a constant image looks up to the tone-mapped constant wherever the blend interpolates
    val, undefined, _ = restate_lookup(np.full((h, w, 3), 4.0, F), F(16.0), u, v)
    assert not undefined.any() and np.allclose(val, 0.75, rtol=1e-6)
    # at v == 1 the index wraps and the error term is h: the blend extrapolates (the quirk is restated, not repaired)
    _, _, ye1, _ = restate_axis(h, np.array([1.0], F))
    assert ye1[0] == h
    rays = ray_set(miro)
    mx, _ = restate_constructor(img)
    val, info = restate_environment(direction_of(rays), ROT, img, mx)
    left_out = int((info["fragile"] | info["undefined"]).sum())
    print("ray set: %d rays, fold %d, wrap %d, fragile %d, undefined %d" % (len(rays), info["fold"].sum(), info["wrap"].sum(),
                                                                            info["fragile"].sum(), info["undefined"].sum()))
    assert len(rays) >= 1000000 and info["fold"].sum() > 1000 and info["wrap"].sum() > 1000 and info["undefined"].sum() == 16
    assert left_out <= 1e-3 * len(rays)
    keep = ~info["undefined"]
    assert np.isfinite(val[keep]).all() and val.max() <= 1.0 and val[keep].min() >= 0.0
    assert val.std() > 100 * RTOL * val.mean()                                         # the image varies far above the tolerance


def test_environment_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_environment.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer waves
    per SIMD than BOTH its own record (tests/golden/kernel_budget_environment.json, written from the build whose GPU tests were
    green) AND the worst value among the kernels of tests/golden/kernel_budget.json.  The unit's remarks live in
    build/mr_environment.remarks.txt, which test_build_budget.py does not read."""
    cur = kernel_budget.unit_kernels("mr_environment")
    assert len(cur) == 8 and all("shade_environment_kernel" in k for k in cur)
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_environment.json")


def build_shim_environment(tmp_path, miro):
    exe = str(tmp_path / "shim_environment")
    lib_dir = os.path.dirname(miro.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "cse168-raytracer_amd", "host"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "shim_environment.cpp"), "-L", lib_dir, "-lmiro_hip", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_shim_environment_program_compiles_with_plain_gxx(tmp_path, miro):
    exe = build_shim_environment(tmp_path, miro)
    assert subprocess.run([exe], capture_output=True).returncode == 2          # usage


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
class Batch:
    """The ray set on the device, traced by mr_trace in the `sphere` scene"""

    def __init__(self, miro, rays=None):
        import torch
        from helpers import product_scene
        self.scene = product_scene(miro, "sphere")
        self.rays = ray_set(miro) if rays is None else rays
        self.n = len(self.rays)
        self.d_rays = torch.from_numpy(self.rays.view(F).reshape(-1, 8)).cuda()
        self.d_hits = torch.empty((self.n, 4), dtype=torch.float32, device="cuda")
        self.scene.trace_device(self.d_rays, self.n, self.d_hits)
        torch.cuda.synchronize()
        self.hits = self.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)
        self.miss = self.hits["prim"] == MISS

    def shade(self, flags=0, lowres=None, n_pixels=None, weights=None, pixels=None, spp=1, rgb=True):
        """(d_rgb, d_ray_rgb, counts) as numpy arrays"""
        import torch
        n = self.n
        d_rgb = torch.zeros((n // spp if n_pixels is None else n_pixels, 3), dtype=torch.float32, device="cuda") if rgb else None
        ray_rgb = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device="cuda")                 # one sentinel row after the end
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.scene.shade_environment(self.d_rays, self.d_hits, n, d_rgb, d_weights=weights, d_pixels=pixels, d_lowres=lowres, spp=spp,
                                     flags=flags, d_ray_rgb=ray_rgb, d_counts=cnt)
        torch.cuda.synchronize()
        out = ray_rgb.cpu().numpy()
        assert (out[n] == -7.0).all(), "d_ray_rgb was written beyond 3n floats"
        return d_rgb.cpu().numpy() if rgb else None, out[:n].copy(), cnt.cpu().numpy().tolist()


@pytest.mark.gpu
def test_ray_values_match_the_restatement(miro):
    """d_ray_rgb of >= 1 M rays (hits and misses) under a non-zero rotation, full resolution, MR_ENV_LOWRES and a per-ray mask:
    hits give exactly 0, d_counts equals the restatement's miss and undefined counts, and the non-fragile misses match within
    rtol 1e-5, atol 1e-7 of the maximum (powf)."""
    import torch
    from miro_amd import binding
    img = synthetic_hdr()
    b = Batch(miro)
    assert b.n >= 1000000 and 0.05 * b.n < b.miss.sum() < 0.95 * b.n
    b.scene.set_environment(bg_color=(0.3, 0.2, 0.1), pixels=img, rotation=ROT)
    low_img, mx = b.scene.get_environment(1)
    d = direction_of(b.rays)
    want_full, info = restate_environment(d, ROT, img, F(mx))
    want_low, info_low = restate_environment(d, ROT, low_img, F(mx))
    assert np.array_equal(info["undefined"], info_low["undefined"])
    rng = np.random.RandomState(3)
    mask = (rng.rand(b.n) < 0.4).astype(np.uint8) * rng.randint(1, 255, b.n).astype(np.uint8)
    modes = [("full", 0, None, want_full), ("lowres", binding.MR_ENV_LOWRES, None, want_low),
             ("mask", 0, torch.from_numpy(mask).cuda(), np.where((mask != 0)[:, None], want_low, want_full))]
    for name, flags, lowres, want in modes:
        _, got, counts = b.shade(flags=flags, lowres=lowres, rgb=False)
        undefined = info["undefined"] & b.miss
        keep = b.miss & ~info["fragile"] & ~info["undefined"]
        scale = float(want[keep].max())
        excess = np.abs(got[keep].astype(np.float64) - want[keep]) - RTOL * np.abs(want[keep])
        print("%s: %d misses of %d rays, %d undefined, %d fragile left out, scale %.4g, worst excess over rtol %.3g (atol %.3g)" % (
            name, b.miss.sum(), b.n, undefined.sum(), (b.miss & info["fragile"]).sum(), scale, excess.max(), ATOL_OF_MAX * scale))
        assert counts == [int(b.miss.sum()), int(undefined.sum())]
        assert (got[~b.miss] == 0).all() and (got[undefined] == 0).all()
        assert (b.miss & (info["fragile"] | info["undefined"])).sum() <= 1e-3 * b.n
        assert np.allclose(got[keep], want[keep], rtol=RTOL, atol=ATOL_OF_MAX * scale)
    assert not np.allclose(want_full[b.miss], want_low[b.miss], rtol=1e-2)               # the two images are told apart


@pytest.mark.gpu
def test_colour_only(miro):
    """Without an image every miss's d_ray_rgb is bg_color bit for bit; on a 1-spp frame the pixels of missing primaries are
    bg_color bit for bit and every other pixel equals the frame rendered without an environment, byte for byte."""
    import torch
    from miro_amd import binding, frame, scenes
    bg = np.array([0.3, 0.2, 0.1], F)
    b = Batch(miro, ray_set(miro, 100000))
    b.scene.set_environment(bg_color=bg)
    rgb, got, counts = b.shade(flags=binding.MR_ENV_LOWRES)
    assert counts == [int(b.miss.sum()), 0] and b.miss.any() and (~b.miss).any()
    assert np.array_equal(got[b.miss].view(np.uint32), np.repeat(bg[None, :], b.miss.sum(), 0).view(np.uint32))
    assert (got[~b.miss] == 0).all() and np.array_equal(rgb.view(np.uint32), got.view(np.uint32))
    desc = scenes.SCENES["sphere"]
    fr = frame.FrameRenderer(b.scene, desc, 160, 128)
    fr.generate()
    fr.render_specular(depth=2)
    torch.cuda.synchronize()
    plain = fr.d_rgb.cpu().numpy().copy()
    fr.render_specular(depth=2, environment=dict(bg_color=bg))
    torch.cuda.synchronize()
    with_bg = fr.d_rgb.cpu().numpy()
    hits = torch.empty((fr.n, 4), dtype=torch.float32, device="cuda")
    b.scene.trace_device(fr.d_rays, fr.n, hits)
    miss = hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"] == MISS
    assert miss.any() and (~miss).any() and (plain[miss] == 0).all()
    assert np.array_equal(with_bg[miss].view(np.uint32), np.repeat(bg[None, :], miss.sum(), 0).view(np.uint32))
    assert with_bg[~miss].tobytes() == plain[~miss].tobytes()


@pytest.mark.gpu
def test_weighted_accumulation(miro):
    """Random weights and a pixel map with runs of equal pixels: d_rgb equals the float64 sum of weight * d_ray_rgb / spp per
    pixel within the float-atomic tolerance of test_level.py (rtol 1e-5, atol 1e-6 of the maximum)."""
    import torch
    b = Batch(miro, ray_set(miro, 300000))
    b.scene.set_environment(pixels=synthetic_hdr(), rotation=ROT)
    rng = np.random.RandomState(11)
    n_pixels, spp = 5000, 4
    runs = rng.randint(1, 40, b.n)
    pix = np.repeat(rng.randint(0, n_pixels, b.n), runs)[:b.n].astype(np.int32)
    w = rng.rand(b.n, 3).astype(F) * 2
    for weights, pixels in ((w, pix), (None, pix), (w, None), (None, None)):
        npx = n_pixels if pixels is not None else (b.n + spp - 1) // spp
        rgb, per_ray, _ = b.shade(n_pixels=npx, spp=spp, weights=torch.from_numpy(weights).cuda() if weights is not None else None,
                                  pixels=torch.from_numpy(pixels).cuda() if pixels is not None else None)
        want = np.zeros((npx, 3), np.float64)
        np.add.at(want, pixels.astype(np.int64) if pixels is not None else np.arange(b.n) // spp,
                  (weights.astype(np.float64) if weights is not None else 1.0) * per_ray.astype(np.float64) / spp)
        scale = float(want.max())
        print("weights %s pixels %s: max %.4g, worst error %.3g" % (weights is not None, pixels is not None, scale, np.abs(rgb - want).max()))
        assert scale > 0 and np.allclose(rgb, want, rtol=1e-5, atol=1e-6 * scale)


def mirror_spheres(miro):
    """The scene of tests/test_objects.py::test_mirror_spheres_over_a_plane"""
    from test_specular import phong
    mats = [phong((0.3, 0.3, 0.3), ks=(0.7, 0.7, 0.7), shininess=float("inf")),
            phong((1, 1, 1), kt=(0.9, 0.9, 0.9), shininess=5.0, index=1.5),
            phong((0.8, 0.2, 0.2))]
    s = miro.Scene()
    prim_mat = []
    for i, (c, r) in enumerate([((-1.2, 0, 0), 1.0), ((1.2, 0, 0.3), 1.0), ((0, -0.5, -2.0), 0.5)]):
        s.add_sphere(c, r)
        prim_mat.append(1 if i == 2 else 0)
    s.add_plane([0, 1, 0], [0, -1, 0], 2)
    s.add_triangle([-4, -1, 3, 4, -1, 3, 0, 5, 3], [0, 0, -1] * 3)
    prim_mat.append(2)
    s.set_materials(mats, np.asarray(prim_mat, np.uint32))
    s.build(4)
    desc = dict(eye=(0.0, 1.0, -6.0), lookat=(0.0, 0.0, 0.0), up=(0, 1, 0), fov=45.0, light=(3.0, 8.0, -6.0), wattage=600.0)
    return s, desc


@pytest.mark.gpu
def test_whole_frame_under_a_sky(miro):
    """render_specular(depth=3, environment=image) on the mirror spheres minus the same frame without an environment is the sum
    over the four levels of weight * restated value / spp of the rays that missed (the test drives mr_trace and
    mr_gen_secondary_rays itself for each level's rays, hits, weights and pixels), within 2e-4 of the frame's maximum
    (test_specular.py); and a pixel inside a sphere's silhouette is lit by nothing but the environment."""
    import torch
    from miro_amd import frame
    scene, desc = mirror_spheres(miro)
    # the light moved behind the spheres: with test_objects.py's light every pixel whose mirror reflection reaches the sky is
    # also lit directly, and none could be "lit by the environment alone" (23 dark pixels, all reflecting the shadowed floor;
    # here 149 dark pixels of 982 see the sky in the mirror -- counted with the oracle)
    desc = dict(desc, light=(0.0, 8.0, 2.5))
    img = synthetic_hdr()
    W, H, spp, depth = 96, 64, 2, 3
    fr = frame.FrameRenderer(scene, desc, W, H, spp=spp)
    fr.generate()
    levels0 = fr.render_specular(depth=depth)
    torch.cuda.synchronize()
    plain = fr.d_rgb.cpu().numpy().astype(np.float64)
    levels1 = fr.render_specular(depth=depth, environment=dict(pixels=img, rotation=ROT))
    torch.cuda.synchronize()
    sky = fr.d_rgb.cpu().numpy().astype(np.float64)
    assert levels0 == levels1 and len(levels1) == depth + 1
    mx = F(scene.get_environment(0)[1])
    want = np.zeros((W * H, 3), np.float64)
    rays, weights, pixels, n = fr.d_rays, None, None, fr.n
    left_out = 0
    first_prim = None
    for level in range(depth + 1):
        hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        scene.trace_device(rays, n, hits, miro.MR_TRACE_INCOHERENT if level else 0)
        h = hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)
        if level == 0:
            first_prim = h["prim"].copy()
        r = rays.cpu().numpy().reshape(-1, 8)
        val, info = restate_environment(np.ascontiguousarray(r[:, 4:7]), ROT, img, mx)
        miss = h["prim"] == MISS
        left_out += int((miss & (info["fragile"] | info["undefined"])).sum())
        wt = weights.cpu().numpy().astype(np.float64) if weights is not None else np.ones((n, 3))
        px = pixels.cpu().numpy().astype(np.int64) if pixels is not None else np.arange(n) // spp
        np.add.at(want, px[miss], wt[miss] * val[miss].astype(np.float64) / spp)
        print("level %d: %d rays, %d misses" % (level, n, miss.sum()))
        assert n == levels1[level][0]
        if level == depth:
            break
        out_rays = torch.empty((3 * n, 8), dtype=torch.float32, device="cuda")
        out_w = torch.empty((3 * n, 3), dtype=torch.float32, device="cuda")
        out_pix = torch.empty(3 * n, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        scene.gen_secondary_rays(rays, hits, weights, pixels, n, out_rays, out_w, out_pix, cnt, spp=spp)
        n = int(cnt.item())
        rays, weights, pixels = out_rays[:n].contiguous(), out_w[:n].contiguous(), out_pix[:n].contiguous()
    scale = float(sky.max())
    err = np.abs((sky - plain) - want)
    print("frame max %.4g, environment part max %.4g, worst error %.3g (bound %.3g), %d fragile rays" % (scale, want.max(), err.max(), 2e-4 * scale, left_out))
    assert left_out == 0 and want.max() > 0.05
    assert err.max() <= 2e-4 * scale
    on_sphere = (first_prim.reshape(W * H, spp) < 2).all(axis=1)                       # both samples on a mirror sphere
    only_sky = on_sphere & (plain.max(axis=1) == 0) & (sky.max(axis=1) > 0)
    print("%d pixels inside a mirror sphere's silhouette are lit by the environment alone" % only_sky.sum())
    assert only_sky.any()


@pytest.mark.gpu
def test_driver_refusals_and_the_untouched_default(miro):
    """fused with an environment: ValueError; an image with MR_PATH_DIFFUSE mixed with other kinds: ValueError (a plain colour is
    fine, and so is MR_PATH_DIFFUSE alone); environment=None issues the calls it always issued -- no mr_shade_environment --
    and the frame's bytes are those of the same call before any environment existed."""
    import torch
    from miro_amd import binding, frame
    scene, desc = mirror_spheres(miro)
    fr = frame.FrameRenderer(scene, desc, 96, 64)
    fr.generate()
    calls = []
    for name in ("trace_device", "gen_shadow_rays", "trace_indirect", "shade_accumulate", "gen_secondary_rays", "shade_environment",
                 "trace_level", "shade_lights", "gen_path_rays", "trace_grouped"):
        def wrap(f, name=name):
            def g(*a, **k):
                calls.append(name)
                return f(*a, **k)
            return g
        setattr(scene, name, wrap(getattr(scene, name)))
    fr.render_specular(depth=2)
    torch.cuda.synchronize()
    before, seq_before = fr.d_rgb.cpu().numpy().tobytes(), list(calls)
    env = dict(pixels=synthetic_hdr(), rotation=ROT)
    with pytest.raises(ValueError):
        fr.render_specular(depth=2, environment=env, fused=True)
    with pytest.raises(ValueError):
        fr.render_specular(depth=2, environment=env, fused="auto")
    all_kinds = binding.MR_PATH_MIRROR | binding.MR_PATH_REFRACT | binding.MR_PATH_DIFFUSE
    with pytest.raises(ValueError):
        fr.render_specular(depth=2, environment=env, path_tracing=True, path_kinds=all_kinds)
    del calls[:]
    fr.render_specular(depth=1, environment=dict(bg_color=(0.1, 0.1, 0.1)), path_tracing=True, path_kinds=all_kinds)
    assert calls.count("shade_environment") == 2
    fr.render_specular(depth=1, environment=env, path_tracing=True, path_kinds=binding.MR_PATH_DIFFUSE)
    torch.cuda.synchronize()
    assert np.isfinite(fr.d_rgb.cpu().numpy()).all()
    # the scene now HAS an environment; None still means "a miss is worth 0"
    del calls[:]
    fr.render_specular(depth=2)
    torch.cuda.synchronize()
    assert calls == seq_before and "shade_environment" not in calls
    # float atomics: two runs of one frame agree to the order of the additions only where a pixel receives several
    after = np.frombuffer(fr.d_rgb.cpu().numpy().tobytes(), F)
    assert np.allclose(after, np.frombuffer(before, F), rtol=1e-6, atol=1e-7 * float(after.max()))
    fr1 = frame.FrameRenderer(scene, desc, 96, 64)
    fr1.generate()
    fr1.render_specular(depth=0)
    torch.cuda.synchronize()
    a = fr1.d_rgb.cpu().numpy().tobytes()
    fr1.render_specular(depth=0, environment=None)
    torch.cuda.synchronize()
    assert fr1.d_rgb.cpu().numpy().tobytes() == a                                      # one addition per pixel: byte-identical


@pytest.mark.gpu
def test_shade_environment_replays_from_a_captured_graph(miro):
    """Once the device copy of the image exists, one call captured on a stream and replayed gives the first call's d_ray_rgb."""
    import torch
    b = Batch(miro, ray_set(miro, 50000))
    b.scene.set_environment(pixels=synthetic_hdr(), rotation=ROT)
    first = torch.zeros((b.n, 3), dtype=torch.float32, device="cuda")
    b.scene.shade_environment(b.d_rays, b.d_hits, b.n, None, d_ray_rgb=first)
    torch.cuda.synchronize()
    assert float(first.max()) > 0
    out = torch.zeros((b.n, 3), dtype=torch.float32, device="cuda")
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.scene.shade_environment(b.d_rays, b.d_hits, b.n, None, d_ray_rgb=out, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        b.scene.shade_environment(b.d_rays, b.d_hits, b.n, None, d_ray_rgb=out, stream=torch.cuda.current_stream())
    for _ in range(2):
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first)


@pytest.mark.gpu
def test_shim_sets_the_environment_like_the_python_path(tmp_path, miro):
    """A g++ program sets colour, image and rotation through miro::Scene and shades one batch: its d_ray_rgb is the Python
    path's, byte for byte -- with the image (full and low-res) and with the colour alone."""
    from miro_amd import binding, scenes
    exe = build_shim_environment(tmp_path, miro)
    img = synthetic_hdr()
    b = Batch(miro, ray_set(miro, 60000))
    img_path, rays_path, out_path = str(tmp_path / "sky.bin"), str(tmp_path / "rays.bin"), str(tmp_path / "out.bin")
    img.tofile(img_path)
    b.rays.tofile(rays_path)
    bg = (0.25, 0.5, 0.75)
    for image, lowres in ((True, 0), (True, 1), (False, 0)):
        b.scene.set_environment(bg_color=bg, pixels=img if image else None, rotation=ROT)
        _, want, _ = b.shade(flags=binding.MR_ENV_LOWRES if lowres else 0, rgb=False)
        r = subprocess.run([exe, scenes._model("sphere.obj"), img_path if image else "-", str(IMG_W), str(IMG_H), repr(ROT[0]), repr(ROT[1]),
                            ",".join(str(x) for x in bg), rays_path, out_path, str(lowres)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        got = np.fromfile(out_path, F).reshape(-1, 3)
        assert want.max() > 0 and got.tobytes() == want.tobytes(), (image, lowres)
